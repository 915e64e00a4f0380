// engine/host_nearest.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_nearest / igd_hip_nearest_dev / igd_hip_nearest_sets: the nearest record per dataset within a window (nearest_dev.hpp)
// igd_hip_nearest_signed / igd_hip_nearest_signed_dev / igd_hip_nearest_hist: the same with a side, and the histogram of the
// signed distances per set and dataset
// ------------------------------------------------------------------------------------------
// The device form takes one engine batch of resident regions and writes resident rows: one launch (the wide form: a fill of
// the rows with 0xff before it and, when dmin is wanted, igd_nearest_rowmin behind it), asynchronous on the caller's stream.
// The host form takes host arrays in CHUNKS of at most igd_hip_max_batch() regions AND at most IGD_NEAREST_ROW_BYTES of device
// rows (4 nFiles bytes per region: 7.6 KB at 1 900 files, 35 000 regions per chunk: chunk_step); run_region_chunks
// (host_common.hpp) stages the regions of a chunk, the body here runs the device form on the engine's stream and sends the rows
// back into the caller's arrays at their place.
// The sets form is run_set_groups (below; also the driver of host_flank.hpp, host_map.hpp, host_permute_nearest.hpp): GROUPS of whole sets whose three result rows (3 x (nFiles + 1) x 8 bytes
// per set) fit sets_row_bytes(), the regions of a group in the same chunks, a slice table of at most IGD_NEAREST_SLICE regions
// of one set per slice; the chunk functor here launches the row kernel and igd_nearest_reduce, which adds the rows into the
// group's three resident matrices.  The rows never leave the device.
// The signed forms are the same bodies (nearest_rows_dev, nearest_rows_host; the same chunk functor) with SIGNED = true: the
// rows hold signed distances, the wide form's second kernel is igd_nearest_rowdecode and always runs, and the reduction is
// igd_nearest_hist into ONE resident matrix of (ne + 1) x (nFiles + 1) words per set, with the slices cut as for
// igd_nearest_reduce: at most IGD_NEAREST_SLICE = 256 regions, so the kernel's u32 LDS counters hold at most 256.
// The image is slice_image(db, IGD_HIP_RULE_FLAT, v): the re-tiled copy when there is one, visited under rule FLAT.
#define IGD_NEAREST_ROW_BYTES ((int64_t)256 << 20)   // device rows of one chunk (of the order of IGD_MEMBER_ROW_BYTES)
#define IGD_NEAREST_SLICE 256                        // regions per slice of igd_nearest_reduce: 64 per wave

// The TEST-ONLY variable IGD_HIP_NEAREST_ROW_BYTES (read once per process, as IGD_HIP_MAX_BATCH) lowers the budget so that
// small fixtures cross the row seam.
static int64_t nearest_row_bytes(void)
{
    static const int64_t m = env_positive("IGD_HIP_NEAREST_ROW_BYTES", IGD_NEAREST_ROW_BYTES);
    return m;
}

// workgroups igd_nearest_rows is launched with for nq regions (each of IGD_SETS_WG / IGD_WAVE waves; a wave meets a second
// region only when nq exceeds the grid's waves)
extern "C" int32_t igd_hip_nearest_grid(int64_t nq) { return items_grid(nq, IGD_SETS_WG / IGD_WAVE); }

static int nearest_window_bad(const char *who, int32_t window)
{
    if (igd_hip_nearest_window_valid(window)) return 0;
    snprintf(g_err, sizeof g_err, "%s: window %d outside 0 .. %d", who, (int)window, (int)IGD_HIP_NEAREST_MAX_WINDOW);
    return 1;
}

// one engine batch of resident regions into resident rows (igd_hip_nearest_dev; SIGNED: igd_hip_nearest_signed_dev)
template <bool SIGNED>
static int nearest_rows_dev(const char *who, igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq,
                            int32_t window, int32_t v, int32_t *d_dist, int32_t *d_dmin, void *stream)
{
    if (nearest_window_bad(who, window)) return IGD_HIP_ERR_ARG;
    if (!db || nq < 0 || nq > max_batch() || (nq > 0 && (!d_ichr || !d_qs || !d_qe || (!d_dist && db->nFiles > 0)))) {
        snprintf(g_err, sizeof g_err, "%s: bad argument (batch limit %lld regions)", who, (long long)max_batch());
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = stream ? (hipStream_t)stream : db->stream;
    const int64_t nF = db->nFiles;
    if (nF == 0) {                                       // rows of no words; no region has a dataset near it
        if (d_dmin && !SIGNED) HIPCHK(hipMemsetAsync(d_dmin, 0xff, (size_t)nq * 4, st));
        if (d_dmin && SIGNED) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d_dmin, IGD_HIP_NEAREST_NO_RECORD, (size_t)nq, st));
        return IGD_HIP_OK;
    }
    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    const bool lds = nF <= IGD_NEAREST_LDS_FILES;
    const int grid = igd_hip_nearest_grid(nq);
    const size_t ldsB = lds ? (size_t)((IGD_SETS_WG / IGD_WAVE) * nF) * 4 : 0;
    const int n = (int)nq;
    if (!lds) HIPCHK(hipMemsetAsync(d_dist, 0xff, (size_t)(nq * nF) * 4, st));       // the wide form minimises into rows of "none"
    with_flags(im.useV, lds, [&](auto V, auto L) {
        igd_nearest_rows<V(), L(), SIGNED><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, d_ichr, d_qs, d_qe, n, window, im.krule, v, d_dist, d_dmin);
    });
    HIPCHK(hipGetLastError());
    if (!lds && SIGNED) {                                // (the rows hold keys: decoded whether sdmin is wanted or not)
        igd_nearest_rowdecode<<<grid, IGD_SETS_WG, 0, st>>>(d_dist, n, (int)nF, d_dmin);
        HIPCHK(hipGetLastError());
    } else if (!lds && d_dmin) {
        igd_nearest_rowmin<<<grid, IGD_SETS_WG, 0, st>>>(d_dist, n, (int)nF, d_dmin);
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_nearest_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq,
                                   int32_t window, int32_t v, int32_t *d_dist, int32_t *d_dmin, void *stream)
{
    return nearest_rows_dev<false>("igd_hip_nearest_dev", db, d_ichr, d_qs, d_qe, nq, window, v, d_dist, d_dmin, stream);
}

extern "C" int igd_hip_nearest_signed_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq,
                                          int32_t window, int32_t v, int32_t *d_sdist, int32_t *d_sdmin, void *stream)
{
    return nearest_rows_dev<true>("igd_hip_nearest_signed_dev", db, d_ichr, d_qs, d_qe, nq, window, v, d_sdist, d_sdmin, stream);
}

// the rows and dmin[] of one chunk of regions
static int ensure_nearest_ws(igd_hip_db *db, int64_t words, int64_t rows)
{
    int rc = dev_grow(db, &db->d_nrDist, &db->nrDistCap, words);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_nrMin, &db->nrMinCap, rows);
    return rc;
}

// host arrays in chunks (igd_hip_nearest; SIGNED: igd_hip_nearest_signed)
template <bool SIGNED>
static int nearest_rows_host(const char *who, igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                             int32_t window, int32_t v, int32_t *dist, int32_t *dmin)
{
    if (nearest_window_bad(who, window)) return IGD_HIP_ERR_ARG;
    if (!db || nq < 0 || (nq > 0 && (!ichr || !qs || !qe || (!dist && db->nFiles > 0)))) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    const int64_t nF = db->nFiles;
    if (nF == 0) {
        if (dmin && !SIGNED) memset(dmin, 0xff, (size_t)nq * 4);
        if (dmin && SIGNED) for (int64_t i = 0; i < nq; i++) dmin[i] = IGD_HIP_NEAREST_NO_RECORD;
        return IGD_HIP_OK;
    }
    return run_region_chunks(db, ichr, qs, qe, nq, chunk_step(nearest_row_bytes(), nF * 4), [&](int64_t c0, int64_t m, hipStream_t st) {
        int rc = ensure_nearest_ws(db, m * nF, m);
        if (rc == IGD_HIP_OK) rc = nearest_rows_dev<SIGNED>(who, db, db->d_qc, db->d_qs, db->d_qe, m, window, v, db->d_nrDist, dmin ? db->d_nrMin : nullptr, st);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(dist + c0 * nF, db->d_nrDist, (size_t)(m * nF) * 4, hipMemcpyDeviceToHost, st));
        if (dmin) HIPCHK(hipMemcpyAsync(dmin + c0, db->d_nrMin, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    });
}

extern "C" int igd_hip_nearest(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window,
                               int32_t v, int32_t *dist, int32_t *dmin)
{
    return nearest_rows_host<false>("igd_hip_nearest", db, ichr, qs, qe, nq, window, v, dist, dmin);
}

extern "C" int igd_hip_nearest_signed(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window,
                                      int32_t v, int32_t *sdist, int32_t *sdmin)
{
    return nearest_rows_host<true>("igd_hip_nearest_signed", db, ichr, qs, qe, nq, window, v, sdist, sdmin);
}

// The group driver of the resident set statistics: igd_hip_nearest_sets, igd_hip_nearest_hist, igd_hip_flank_reldist,
// igd_hip_map_sets and igd_hip_nearest_sets_fused (the arguments are checked, there are regions and files).  Per set there are
// nMat result rows of matRow 64-bit words, kept in d_grpStat as nMat matrices of rows x matRow words: GROUPS of whole sets are
// taken while they fit sets_row_bytes(); their regions go through in chunks of `step` regions -- a set may be cut by a chunk,
// its statistics are sums over regions.  Per chunk the regions go to the staging buffers, the chunk's part of every set it
// meets is cut into slices of at most sliceLen regions (0: sets_slice_len(chunk)), the table goes to d_grpSlices, and
// chunk(grid, ns, rows, m, st) sees to its own row workspace and launches its kernels, which add the chunk into the matrices:
// grid is that of a reduction over nCols columns and ns slices (reduce_grid_y), rows the sets of the group, m the regions of
// the chunk.  Then the stream is waited for (the slice table is the host's vector; the staging buffers are reused).  Matrix i
// is copied out to outs[i] (may be NULL) once per group.
template <typename Chunk>
static int run_set_groups(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                          int64_t step, int64_t sliceLen, int nMat, int64_t matRow, int64_t *const *outs, int64_t nCols, Chunk &&chunk)
{
    int rc;
    const int64_t rowCap = sets_row_bytes() / (nMat * matRow * 8) > 0 ? sets_row_bytes() / (nMat * matRow * 8) : 1;
    const int gx = (int)((nCols + IGD_WAVE - 1) / IGD_WAVE);
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    for (int32_t k0 = 0; k0 < nsets;) {
        // one group: sets [k0, k1), regions [set_off[k0], set_off[k1])
        const int32_t k1 = (int32_t)(nsets - k0 < rowCap ? nsets : k0 + rowCap);
        const int64_t rows = k1 - k0, matWords = rows * matRow;
        if ((rc = dev_grow(db, &db->d_grpStat, &db->grpStatCap, nMat * matWords)) != IGD_HIP_OK) return rc;
        HIPCHK(hipMemsetAsync(db->d_grpStat, 0, (size_t)(nMat * matWords) * 8, st));
        int32_t k = k0;
        for (int64_t c0 = set_off[k0]; c0 < set_off[k1]; c0 += step) {
            const int64_t m = set_off[k1] - c0 < step ? set_off[k1] - c0 : step;
            const int64_t len = sliceLen ? sliceLen : sets_slice_len(m);
            slices.clear();
            while (set_off[k + 1] <= c0) k++;
            for (int32_t j = k; j < k1 && set_off[j] < c0 + m; j++)
                push_slices(slices, j - k0, set_off[j] > c0 ? set_off[j] : c0, set_off[j + 1] < c0 + m ? set_off[j + 1] : c0 + m, len, c0);
            const int ns = (int)slices.size();
            rc = dev_grow(db, &db->d_grpSlices, &db->grpSliceCap, (int64_t)ns);
            if (rc == IGD_HIP_OK) rc = stage_queries(db, ichr, qs, qe, c0, m);
            if (rc != IGD_HIP_OK) return rc;
            HIPCHK(hipMemcpyAsync(db->d_grpSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
            if ((rc = chunk(dim3((unsigned)gx, (unsigned)reduce_grid_y(gx, ns)), ns, rows, m, st)) != IGD_HIP_OK) return rc;
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
        for (int i = 0; i < nMat; i++)
            if (outs[i]) HIPCHK(hipMemcpyAsync(outs[i] + (int64_t)k0 * matRow, db->d_grpStat + i * matWords, (size_t)matWords * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        k0 = k1;
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_nearest_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                    int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    if (nearest_window_bad("igd_hip_nearest_sets", window)) return IGD_HIP_ERR_ARG;
    if (!db || nsets < 0 || (nsets > 0 && !set_off)) {
        snprintf(g_err, sizeof g_err, "igd_hip_nearest_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_nearest_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles, nC = nF + 1;
    int64_t *outs[3] = {n_within, n_overlap, sum_dist};
    if (set_off[nsets] == 0 || nF == 0) {                // every statistic is 0: no region, or no dataset to be near
        for (int64_t *o : outs) if (o) memset(o, 0, (size_t)nsets * (size_t)nC * 8);
        return IGD_HIP_OK;
    }
    return run_set_groups(db, ichr, qs, qe, set_off, nsets, chunk_step(nearest_row_bytes(), nF * 4), IGD_NEAREST_SLICE, 3, nC, outs, nC,
                          [&](dim3 grid, int ns, int64_t rows, int64_t m, hipStream_t st) {
        int rc2 = ensure_nearest_ws(db, m * nF, m);
        if (rc2 == IGD_HIP_OK) rc2 = nearest_rows_dev<false>("igd_hip_nearest_sets", db, db->d_qc, db->d_qs, db->d_qe, m, window, v, db->d_nrDist, db->d_nrMin, st);
        if (rc2 != IGD_HIP_OK) return rc2;
        igd_nearest_reduce<<<grid, IGD_SETS_WG, 0, st>>>(db->d_nrDist, db->d_nrMin, (int)nF, db->d_grpSlices, ns, (u64 *)db->d_grpStat, rows * nC);
        return IGD_HIP_OK;
    });
}

extern "C" int igd_hip_nearest_hist(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                    int32_t nsets, int32_t window, int32_t v, const int32_t *edges, int32_t ne, int64_t *hist)
{
    if (nearest_window_bad("igd_hip_nearest_hist", window)) return IGD_HIP_ERR_ARG;
    if (!igd_hip_nearest_edges_valid(edges, ne)) {
        snprintf(g_err, sizeof g_err, "igd_hip_nearest_hist: edges must be 1 .. %d strictly ascending int32", (int)IGD_HIP_NEAREST_MAX_EDGES);
        return IGD_HIP_ERR_ARG;
    }
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !hist))) {
        snprintf(g_err, sizeof g_err, "igd_hip_nearest_hist: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_nearest_hist", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles, nC = nF + 1, matRow = (int64_t)(ne + 1) * nC;
    if (set_off[nsets] == 0 || nF == 0) {                // no region, or no dataset to be near: no region is in a bin
        memset(hist, 0, (size_t)nsets * (size_t)matRow * 8);
        return IGD_HIP_OK;
    }
    HIPCHK(hipSetDevice(db->device));
    if ((rc = dev_grow(db, &db->d_nrEdges, &db->nrEdgesCap, (int64_t)IGD_HIP_NEAREST_MAX_EDGES)) != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(db->d_nrEdges, edges, (size_t)ne * 4, hipMemcpyHostToDevice, db->stream));
    int64_t *outs[1] = {hist};
    return run_set_groups(db, ichr, qs, qe, set_off, nsets, chunk_step(nearest_row_bytes(), nF * 4), IGD_NEAREST_SLICE, 1, matRow, outs, nC,
                          [&](dim3 grid, int ns, int64_t, int64_t m, hipStream_t st) {
        int rc2 = ensure_nearest_ws(db, m * nF, m);
        if (rc2 == IGD_HIP_OK) rc2 = nearest_rows_dev<true>("igd_hip_nearest_hist", db, db->d_qc, db->d_qs, db->d_qe, m, window, v, db->d_nrDist, db->d_nrMin, st);
        if (rc2 != IGD_HIP_OK) return rc2;
        igd_nearest_hist<<<grid, IGD_SETS_WG, 0, st>>>(db->d_nrDist, db->d_nrMin, (int)nF, db->d_grpSlices, ns, db->d_nrEdges, (int)ne, (u64 *)db->d_grpStat);
        return IGD_HIP_OK;
    });
}
