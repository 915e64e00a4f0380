// engine/host_permute_nearest.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_nearest_sets_fused / igd_hip_permute_nearest: the set statistics of the nearest record per dataset through
// igd_nearest_slices (nearest_fused_dev.hpp), and their permutation null
// ------------------------------------------------------------------------------------------
// igd_hip_nearest_sets_fused has igd_hip_nearest_sets' contract (host_nearest.hpp) and its driver, run_set_groups
// (host_common.hpp): GROUPS of whole sets whose three result rows fit sets_row_bytes(), their regions in chunks of
// igd_hip_max_batch() -- there are no distance rows, so no row budget and no row workspace -- every chunk's part of every set
// cut into slices of sets_slice_len(chunk) regions, ONE launch per chunk with support_launch's grid rule, the three matrices
// copied out once per group.
// igd_hip_permute_nearest runs in run_perm_chunks (host_permute.hpp: refusals, upload, chunks, the wait) with the three
// matrices as its rows, 3 * (nFiles + 1) * 8 bytes per permutation: the slice table has one row per permutation of a chunk, is
// built and uploaded once, and a shorter last chunk uses its prefix; per chunk a memset of the chunk's three matrices, the
// fused kernel, an asynchronous copy of the chunk's rows into a buffer of this file.  The null distribution itself comes back,
// int64[nperm + 1][nFiles + 1] three times: the statistic of interest is a ratio of two of them per permutation.  On an error
// nothing of the caller's is written.
// Databases with more files than IGD_NEAREST_FUSED_LDS_FILES: the first calls igd_hip_nearest_sets; the second runs
// igd_hip_nearest_dev + igd_nearest_reduce over the same staged regions (nearest_rows_reduce below), in pieces within the
// row budget of igd_hip_nearest, with a wait per piece.  The results are the same integers.
// The matrices and slice tables are the group driver's workspaces (db->d_grpStat, d_grpSlices).
static_assert(IGD_SETS_SLICE_MAX < 65536, "igd_nearest_slices packs n_within and n_overlap of one slice into 16 bits each");

extern "C" int32_t igd_hip_nearest_fused_max_files(void) { return IGD_NEAREST_FUSED_LDS_FILES; }

// workgroups igd_nearest_slices is launched with for nslices slices: a workgroup takes a second slice only past IGD_SETS_GRID
extern "C" int32_t igd_hip_nearest_fused_grid(int64_t nslices) { return items_grid(nslices, 1); }

// igd_nearest_slices over `ns` slices of the table at db->d_grpSlices into the matrices at db->d_grpStat
static int nearest_fused_launch(igd_hip_db *db, const SliceImage &im, const int32_t *c, const int32_t *s, const int32_t *e, int ns,
                                int32_t window, int32_t v, int64_t matWords)
{
    const size_t ldsB = IGD_NEAREST_FUSED_LDS_BYTES(db->nFiles);
    const int grid = igd_hip_nearest_fused_grid(ns);
    auto go = [&](auto V) {
        if (ldsB > (size_t)65536)                        // (more dynamic LDS than a launch gets unasked)
            (void)hipFuncSetAttribute((const void *)igd_nearest_slices<V()>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
        igd_nearest_slices<V()><<<grid, IGD_SETS_WG, ldsB, db->stream>>>(im.view, c, s, e, db->d_grpSlices, ns, window, im.krule, v,
                                                                        (u64 *)db->d_grpStat, matWords);
    };
    if (im.useV) go(std::true_type{});
    else go(std::false_type{});
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

extern "C" int igd_hip_nearest_sets_fused(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                          int32_t nsets, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    if (nearest_window_bad("igd_hip_nearest_sets_fused", window)) return IGD_HIP_ERR_ARG;
    if (!db || nsets < 0 || (nsets > 0 && !set_off)) {
        snprintf(g_err, sizeof g_err, "igd_hip_nearest_sets_fused: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_nearest_sets_fused", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles, nC = nF + 1;
    if (nF > IGD_NEAREST_FUSED_LDS_FILES)                 // no wide form: the rows route
        return igd_hip_nearest_sets(db, ichr, qs, qe, set_off, nsets, window, v, n_within, n_overlap, sum_dist);
    int64_t *outs[3] = {n_within, n_overlap, sum_dist};
    if (set_off[nsets] == 0 || nF == 0) {                // every statistic is 0: no region, or no dataset to be near
        for (int64_t *o : outs) if (o) memset(o, 0, (size_t)nsets * (size_t)nC * 8);
        return IGD_HIP_OK;
    }
    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    // (slice length 0: sets_slice_len(chunk); the kernel has a grid rule of its own, nearest_fused_launch)
    return run_set_groups(db, ichr, qs, qe, set_off, nsets, max_batch(), 0, 3, nC, outs, nC, [&](dim3, int ns, int64_t rows, int64_t, hipStream_t) {
        return nearest_fused_launch(db, im, db->d_qc, db->d_qs, db->d_qe, ns, window, v, rows * nC);
    });
}

// Databases too wide for igd_nearest_slices: `rows` rows of nq resident regions each (c, s, e; row r = regions [r nq, (r + 1) nq))
// through igd_hip_nearest_dev and igd_nearest_reduce into the matrices at db->d_grpStat, in pieces of igd_hip_nearest's chunk_step()
// regions -- a piece may cut a row, the statistics are sums over regions -- with slices of IGD_NEAREST_SLICE and a wait per
// piece.  (The chunk body of run_set_groups over RESIDENT regions cut by nq, not staged ones cut by set_off: it stays its own loop.)
static int nearest_rows_reduce(igd_hip_db *db, const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t nq,
                               int32_t window, int32_t v, int64_t matWords)
{
    const int64_t nF = db->nFiles, nC = nF + 1, total = rows * nq, step = chunk_step(nearest_row_bytes(), nF * 4);
    const int gx = (int)((nC + IGD_WAVE - 1) / IGD_WAVE);
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    for (int64_t c0 = 0; c0 < total; c0 += step) {
        const int64_t m = total - c0 < step ? total - c0 : step;
        slices.clear();
        for (int64_t r = c0 / nq; r < rows && r * nq < c0 + m; r++)
            push_slices(slices, (int32_t)r, r * nq > c0 ? r * nq : c0, (r + 1) * nq < c0 + m ? (r + 1) * nq : c0 + m, IGD_NEAREST_SLICE, c0);
        const int ns = (int)slices.size();
        int rc = ensure_nearest_ws(db, m * nF, m);
        if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_grpSlices, &db->grpSliceCap, (int64_t)ns);
        if (rc == IGD_HIP_OK) rc = igd_hip_nearest_dev(db, c + c0, s + c0, e + c0, m, window, v, db->d_nrDist, db->d_nrMin, st);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(db->d_grpSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        igd_nearest_reduce<<<dim3((unsigned)gx, (unsigned)reduce_grid_y(gx, ns)), IGD_SETS_WG, 0, st>>>(db->d_nrDist, db->d_nrMin, (int)nF, db->d_grpSlices, ns,
                                                                                  (u64 *)db->d_grpStat, matWords);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));                // (the slice table is the host's vector)
    }
    return IGD_HIP_OK;
}

// the body of igd_hip_permute_nearest_ws and, with a pool and no ctg_len, of igd_hip_permute_nearest_rs
static int permute_nearest_run(const char *who, igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const PermSpec &sp, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    if (nearest_window_bad(who, window)) return IGD_HIP_ERR_ARG;
    if (perm_args_refused(who, db, ichr, qs, qe, nq, sp, false)) return IGD_HIP_ERR_ARG;
    const int64_t nF = db->nFiles, nC = nF + 1, nperm = sp.nperm, R = nperm + 1;
    int64_t *const outs[3] = {n_within, n_overlap, sum_dist};
    if (nq == 0 || nF == 0) {                            // every statistic is 0: no region, or no dataset to be near
        for (int64_t *o : outs) if (o) memset(o, 0, (size_t)R * (size_t)nC * 8);
        return IGD_HIP_OK;
    }

    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    const bool fused = nF <= IGD_NEAREST_FUSED_LDS_FILES;
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    std::vector<int64_t> res((size_t)(3 * R * nC));
    int64_t perRow = 0;
    auto prepare = [&](int64_t pc, int64_t sliceLen, int64_t perRow_) -> int {
        perRow = perRow_;
        if (fused) slices = perm_row_slices(pc, nq, sliceLen);
        int rc = dev_grow(db, &db->d_grpStat, &db->grpStatCap, 3 * pc * nC);
        if (rc == IGD_HIP_OK && fused) rc = dev_grow(db, &db->d_grpSlices, &db->grpSliceCap, pc * perRow);
        return rc;
    };
    // `rows` rows counted from the region arrays (c, s, e) into zeroed matrices, which go to rows [r0, r0 + rows) of res
    auto count = [&](const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t r0) -> int {
        const int64_t matWords = rows * nC;
        if (r0 == 0 && fused) HIPCHK(hipMemcpyAsync(db->d_grpSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(db->d_grpStat, 0, (size_t)(3 * matWords) * 8, st));
        const int rc = fused ? nearest_fused_launch(db, im, c, s, e, (int)(rows * perRow), window, v, matWords)
                             : nearest_rows_reduce(db, c, s, e, rows, nq, window, v, matWords);
        if (rc != IGD_HIP_OK) return rc;
        for (int i = 0; i < 3; i++)
            HIPCHK(hipMemcpyAsync(res.data() + (i * R + r0) * nC, db->d_grpStat + i * matWords, (size_t)matWords * 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    };
    const int rc = run_perm_chunks(db, ichr, qs, qe, nq, sp, 3 * nC * 8, prepare, count);
    if (rc != IGD_HIP_OK) return rc;
    for (int i = 0; i < 3; i++)
        if (outs[i]) memcpy(outs[i], res.data() + (size_t)i * (size_t)(R * nC), (size_t)(R * nC) * 8);
    return IGD_HIP_OK;
}

extern "C" int igd_hip_permute_nearest_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                          const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v,
                                          int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist, const igd_hip_workspace *ws)
{
    const PermSpec sp{ctg_len, mode, seed, nperm, ws, nullptr, nullptr};
    return permute_nearest_run("igd_hip_permute_nearest", db, ichr, qs, qe, nq, sp, window, v, n_within, n_overlap, sum_dist);
}

extern "C" int igd_hip_permute_nearest_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                          const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool,
                                          uint64_t seed, int64_t nperm, int32_t window, int32_t v, int64_t *n_within, int64_t *n_overlap,
                                          int64_t *sum_dist)
{
    const PermPool pool{pool_ichr, pool_qs, pool_qe, npool};
    const PermSpec sp{nullptr, IGD_HIP_PERM_RESAMPLE, seed, nperm, nullptr, nullptr, &pool};
    return permute_nearest_run("igd_hip_permute_nearest_rs", db, ichr, qs, qe, nq, sp, window, v, n_within, n_overlap, sum_dist);
}

extern "C" int igd_hip_permute_nearest(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                       const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int32_t window, int32_t v,
                                       int64_t *n_within, int64_t *n_overlap, int64_t *sum_dist)
{
    return igd_hip_permute_nearest_ws(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, window, v, n_within, n_overlap, sum_dist, nullptr);
}
