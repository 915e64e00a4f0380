// engine/host_map.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_map / igd_hip_map_dev / igd_hip_map_sets: the values of the overlapping records per region and dataset (map_dev.hpp)
// ------------------------------------------------------------------------------------------
// The shape of host_nearest.hpp.  The device form takes one engine batch of resident regions and writes resident rows: one
// launch (the wide form: fills of the rows before it and, but for SUM, igd_map_rowfix behind it), asynchronous on the caller's
// stream.  The host form takes host arrays in CHUNKS of at most igd_hip_max_batch() regions AND at most IGD_MAP_ROW_BYTES of
// device rows (4 nFiles bytes per region under COUNT, 12 nFiles otherwise: 22.8 KB at 1 900 files, 11 700 regions per chunk:
// chunk_step); run_region_chunks (host_common.hpp) stages the regions of a chunk, the body here runs the device form on the
// engine's stream and sends the rows back into the caller's arrays at their place.
// The sets form is run_set_groups (host_nearest.hpp): GROUPS of whole sets whose three result rows (3 x nFiles x 8 bytes per
// set) fit sets_row_bytes(), the regions of a group in the same chunks, a slice table of at most IGD_MAP_SLICE regions of one
// set per slice; the chunk functor here runs the device form and igd_map_reduce, which adds the rows into the group's three
// resident matrices (the handle's d_grpStat and d_grpSlices, shared with the nearest family).  The rows never leave the
// device.  Under COUNT there are no agg rows at all: agg_sum is summed from the counts.
// The image is slice_image(db, IGD_HIP_RULE_FLAT, v): the re-tiled copy when there is one, visited under rule FLAT.
#define IGD_MAP_ROW_BYTES ((int64_t)256 << 20)       // device rows of one chunk (IGD_NEAREST_ROW_BYTES)
#define IGD_MAP_SLICE 256                            // regions per slice of igd_map_reduce: 64 per wave

// The TEST-ONLY variable IGD_HIP_MAP_ROW_BYTES (read once per process, as IGD_HIP_MAX_BATCH) lowers the budget so that small
// fixtures cross the row seam.
static int64_t map_row_bytes(void)
{
    static const int64_t m = env_positive("IGD_HIP_MAP_ROW_BYTES", IGD_MAP_ROW_BYTES);
    return m;
}

// workgroups igd_map_rows is launched with for nq regions (each of IGD_SETS_WG / IGD_WAVE waves; a wave meets a second region
// only when nq exceeds the grid's waves)
extern "C" int32_t igd_hip_map_grid(int64_t nq) { return items_grid(nq, IGD_SETS_WG / IGD_WAVE); }

// an unknown op, or an op that reads values on a database without them
static int map_op_bad(const char *who, const igd_hip_db *db, int op)
{
    if (!igd_hip_map_op_valid(op)) {
        snprintf(g_err, sizeof g_err, "%s: no such op %d", who, op);
        return 1;
    }
    if (db && op != IGD_HIP_MAP_COUNT && db->gType != 1) {
        snprintf(g_err, sizeof g_err, "%s: sum, min and max need a database with values (gType 1)", who);
        return 1;
    }
    return 0;
}

template <bool V, bool L>
static void map_launch(int op, int grid, size_t ldsB, hipStream_t st, const DbView &view, const int32_t *d_ichr, const int32_t *d_qs,
                       const int32_t *d_qe, int n, int krule, int v, int32_t *d_count, int64_t *d_agg)
{
    switch (op) {
    case IGD_HIP_MAP_COUNT: igd_map_rows<V, IGD_HIP_MAP_COUNT, L><<<grid, IGD_SETS_WG, ldsB, st>>>(view, d_ichr, d_qs, d_qe, n, krule, v, d_count, d_agg); break;
    case IGD_HIP_MAP_SUM: igd_map_rows<V, IGD_HIP_MAP_SUM, L><<<grid, IGD_SETS_WG, ldsB, st>>>(view, d_ichr, d_qs, d_qe, n, krule, v, d_count, d_agg); break;
    case IGD_HIP_MAP_MIN: igd_map_rows<V, IGD_HIP_MAP_MIN, L><<<grid, IGD_SETS_WG, ldsB, st>>>(view, d_ichr, d_qs, d_qe, n, krule, v, d_count, d_agg); break;
    default: igd_map_rows<V, IGD_HIP_MAP_MAX, L><<<grid, IGD_SETS_WG, ldsB, st>>>(view, d_ichr, d_qs, d_qe, n, krule, v, d_count, d_agg); break;
    }
}

extern "C" int igd_hip_map_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int op, int32_t v,
                               int32_t *d_count, int64_t *d_agg, void *stream)
{
    if (map_op_bad("igd_hip_map_dev", db, op)) return IGD_HIP_ERR_ARG;
    if (!db || nq < 0 || nq > max_batch() ||
        (nq > 0 && (!d_ichr || !d_qs || !d_qe || (db->nFiles > 0 && (!d_count || (!d_agg && op != IGD_HIP_MAP_COUNT)))))) {
        snprintf(g_err, sizeof g_err, "igd_hip_map_dev: bad argument (batch limit %lld regions)", (long long)max_batch());
        return IGD_HIP_ERR_ARG;
    }
    const int64_t nF = db->nFiles;
    if (nq == 0 || nF == 0) return IGD_HIP_OK;           // (rows of no words)
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = stream ? (hipStream_t)stream : db->stream;
    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    const bool lds = nF <= map_lds_files(op);
    const int grid = igd_hip_map_grid(nq);
    const size_t ldsB = lds ? (size_t)((IGD_SETS_WG / IGD_WAVE) * nF) * (size_t)map_lds_file_bytes(op) : 0;
    const size_t cells = (size_t)(nq * nF);
    if (!lds) {                                          // the wide form folds into rows of "nothing yet"
        HIPCHK(hipMemsetAsync(d_count, 0, cells * 4, st));
        if (op != IGD_HIP_MAP_COUNT) HIPCHK(hipMemsetAsync(d_agg, op == IGD_HIP_MAP_MIN ? 0x7f : op == IGD_HIP_MAP_MAX ? 0x80 : 0, cells * 8, st));
    }
    with_flags(im.useV, lds, [&](auto V, auto L) {
        map_launch<V(), L()>(op, grid, ldsB, st, im.view, d_ichr, d_qs, d_qe, (int)nq, im.krule, v, d_count, d_agg);
    });
    HIPCHK(hipGetLastError());
    if (!lds && d_agg && op != IGD_HIP_MAP_SUM) {
        const int fg = (int)items_grid((int64_t)cells, 4 * IGD_SETS_WG);
        if (op == IGD_HIP_MAP_COUNT) igd_map_rowfix<IGD_HIP_MAP_COUNT><<<fg, IGD_SETS_WG, 0, st>>>(d_count, d_agg, cells);
        else igd_map_rowfix<IGD_HIP_MAP_MIN><<<fg, IGD_SETS_WG, 0, st>>>(d_count, d_agg, cells);
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}

// the count and agg rows of one chunk of regions
static int ensure_map_ws(igd_hip_db *db, int64_t cells, bool withAgg)
{
    int rc = dev_grow(db, &db->d_mpCount, &db->mpCountCap, cells);
    if (rc == IGD_HIP_OK && withAgg) rc = dev_grow(db, &db->d_mpAgg, &db->mpAggCap, cells);
    return rc;
}

extern "C" int igd_hip_map(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int op, int32_t v,
                           int32_t *count, int64_t *agg)
{
    if (map_op_bad("igd_hip_map", db, op)) return IGD_HIP_ERR_ARG;
    if (!db || nq < 0 || (nq > 0 && (!ichr || !qs || !qe || (db->nFiles > 0 && (!count || (!agg && op != IGD_HIP_MAP_COUNT)))))) {
        snprintf(g_err, sizeof g_err, "igd_hip_map: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    const int64_t nF = db->nFiles;
    if (nq == 0 || nF == 0) return IGD_HIP_OK;
    const bool withAgg = agg != nullptr;
    return run_region_chunks(db, ichr, qs, qe, nq, chunk_step(map_row_bytes(), nF * (withAgg ? 12 : 4)), [&](int64_t c0, int64_t m, hipStream_t st) {
        int rc = ensure_map_ws(db, m * nF, withAgg);
        if (rc == IGD_HIP_OK) rc = igd_hip_map_dev(db, db->d_qc, db->d_qs, db->d_qe, m, op, v, db->d_mpCount, withAgg ? db->d_mpAgg : nullptr, st);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(count + c0 * nF, db->d_mpCount, (size_t)(m * nF) * 4, hipMemcpyDeviceToHost, st));
        if (withAgg) HIPCHK(hipMemcpyAsync(agg + c0 * nF, db->d_mpAgg, (size_t)(m * nF) * 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    });
}

extern "C" int igd_hip_map_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                int32_t nsets, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    if (map_op_bad("igd_hip_map_sets", db, op)) return IGD_HIP_ERR_ARG;
    if (!db || nsets < 0 || (nsets > 0 && !set_off)) {
        snprintf(g_err, sizeof g_err, "igd_hip_map_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_map_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles;
    int64_t *outs[3] = {n_hit, pairs, agg_sum};
    if (set_off[nsets] == 0 || nF == 0) {                // every statistic is 0: no region, or no dataset
        for (int64_t *o : outs) if (o) memset(o, 0, (size_t)nsets * (size_t)nF * 8);
        return IGD_HIP_OK;
    }
    const bool withAgg = op != IGD_HIP_MAP_COUNT;
    return run_set_groups(db, ichr, qs, qe, set_off, nsets, chunk_step(map_row_bytes(), nF * (withAgg ? 12 : 4)), IGD_MAP_SLICE, 3, nF, outs, nF,
                          [&](dim3 grid, int ns, int64_t rows, int64_t m, hipStream_t st) {
        int rc2 = ensure_map_ws(db, m * nF, withAgg);
        if (rc2 == IGD_HIP_OK) rc2 = igd_hip_map_dev(db, db->d_qc, db->d_qs, db->d_qe, m, op, v, db->d_mpCount, withAgg ? db->d_mpAgg : nullptr, st);
        if (rc2 != IGD_HIP_OK) return rc2;
        igd_map_reduce<<<grid, IGD_SETS_WG, 0, st>>>(db->d_mpCount, withAgg ? db->d_mpAgg : nullptr, (int)nF, db->d_grpSlices, ns, (u64 *)db->d_grpStat, rows * nF);
        return IGD_HIP_OK;
    });
}
