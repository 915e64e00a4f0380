// engine/host_permute_map.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_map_sets_fused / igd_hip_permute_map: the set statistics of the overlapping records' values per dataset through
// igd_map_slices (map_fused_dev.hpp), and their permutation null
// ------------------------------------------------------------------------------------------
// The shape of host_permute_nearest.hpp.  igd_hip_map_sets_fused has igd_hip_map_sets' contract (host_map.hpp) and its driver,
// run_set_groups (host_nearest.hpp): GROUPS of whole sets whose three result rows fit sets_row_bytes(), their regions in chunks
// of igd_hip_max_batch() -- there are no count or agg rows, so no row budget and no row workspace -- every chunk's part of every
// set cut into slices of sets_slice_len(chunk) regions, ONE launch per chunk, the three matrices copied out once per group.
// igd_hip_permute_map runs in run_perm_chunks (host_permute.hpp: upload, chunks, the wait) with the three matrices as its rows,
// 3 * nFiles * 8 bytes per permutation: the slice table has one row per permutation of a chunk, is built and uploaded once, and
// a shorter last chunk uses its prefix; per chunk a memset of the chunk's three matrices, the fused kernel, an asynchronous copy
// of the chunk's rows into a buffer of this file.  The null distribution itself comes back, int64[nperm + 1][nFiles] three
// times: the statistic of interest is a ratio of two of them per permutation.  On an error nothing of the caller's is written.
// Databases with more files than igd_hip_map_fused_max_files(op): the first calls igd_hip_map_sets; the second runs
// igd_hip_map_dev + igd_map_reduce over the same resident regions (map_rows_reduce below), in pieces within map_row_bytes(),
// with a wait per piece.  The results are the same integers.
// The matrices and slice tables are the group driver's workspaces (db->d_grpStat, d_grpSlices).
static_assert(IGD_SETS_SLICE_MAX < 65536, "igd_map_slices counts the regions of one slice with a record in a 32-bit LDS word");

extern "C" int32_t igd_hip_map_fused_max_files(int op) { return igd_hip_map_op_valid(op) ? map_fused_max_files(op) : 0; }

// workgroups igd_map_slices is launched with for nslices slices: a workgroup takes a second slice only past IGD_SETS_GRID
extern "C" int32_t igd_hip_map_fused_grid(int64_t nslices) { return items_grid(nslices, 1); }

template <bool V, int OP>
static int map_fused_launch_op(igd_hip_db *db, const SliceImage &im, const int32_t *c, const int32_t *s, const int32_t *e, int ns, int32_t v,
                               int64_t matWords)
{
    const size_t ldsB = IGD_MAP_FUSED_LDS_BYTES(db->nFiles, OP);
    if (ldsB > (size_t)65536)                            // (more dynamic LDS than a launch gets unasked)
        HIPCHK(hipFuncSetAttribute((const void *)igd_map_slices<V, OP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB));
    igd_map_slices<V, OP><<<igd_hip_map_fused_grid(ns), IGD_SETS_WG, ldsB, db->stream>>>(im.view, c, s, e, db->d_grpSlices, ns, im.krule, v,
                                                                                       (u64 *)db->d_grpStat, matWords);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

// igd_map_slices over `ns` slices of the table at db->d_grpSlices into the matrices at db->d_grpStat (nFiles within the op's limit)
static int map_fused_launch(igd_hip_db *db, const SliceImage &im, const int32_t *c, const int32_t *s, const int32_t *e, int ns, int op,
                            int32_t v, int64_t matWords)
{
    auto go = [&](auto V) {
        switch (op) {
        case IGD_HIP_MAP_COUNT: return map_fused_launch_op<V(), IGD_HIP_MAP_COUNT>(db, im, c, s, e, ns, v, matWords);
        case IGD_HIP_MAP_SUM: return map_fused_launch_op<V(), IGD_HIP_MAP_SUM>(db, im, c, s, e, ns, v, matWords);
        case IGD_HIP_MAP_MIN: return map_fused_launch_op<V(), IGD_HIP_MAP_MIN>(db, im, c, s, e, ns, v, matWords);
        default: return map_fused_launch_op<V(), IGD_HIP_MAP_MAX>(db, im, c, s, e, ns, v, matWords);
        }
    };
    return im.useV ? go(std::true_type{}) : go(std::false_type{});
}

extern "C" int igd_hip_map_sets_fused(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                      int32_t nsets, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    if (map_op_bad("igd_hip_map_sets_fused", db, op)) return IGD_HIP_ERR_ARG;
    if (!db || nsets < 0 || (nsets > 0 && !set_off)) {
        snprintf(g_err, sizeof g_err, "igd_hip_map_sets_fused: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_map_sets_fused", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles;
    if (nF > map_fused_max_files(op))                    // no wide form: the rows route
        return igd_hip_map_sets(db, ichr, qs, qe, set_off, nsets, op, v, n_hit, pairs, agg_sum);
    int64_t *outs[3] = {n_hit, pairs, agg_sum};
    if (set_off[nsets] == 0 || nF == 0) {                // every statistic is 0: no region, or no dataset
        for (int64_t *o : outs) if (o) memset(o, 0, (size_t)nsets * (size_t)nF * 8);
        return IGD_HIP_OK;
    }
    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    // (slice length 0: sets_slice_len(chunk); the kernel has a grid rule of its own, map_fused_launch)
    return run_set_groups(db, ichr, qs, qe, set_off, nsets, max_batch(), 0, 3, nF, outs, nF, [&](dim3, int ns, int64_t rows, int64_t, hipStream_t) {
        return map_fused_launch(db, im, db->d_qc, db->d_qs, db->d_qe, ns, op, v, rows * nF);
    });
}

// Databases too wide for igd_map_slices: `rows` rows of nq resident regions each (c, s, e; row r = regions [r nq, (r + 1) nq))
// through igd_hip_map_dev and igd_map_reduce into the matrices at db->d_grpStat, in pieces of igd_hip_map's chunk_step() regions
// -- a piece may cut a row, the statistics are sums over regions -- with slices of IGD_MAP_SLICE and a wait per piece: the
// pattern of nearest_rows_reduce (host_permute_nearest.hpp).
static int map_rows_reduce(igd_hip_db *db, const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t nq, int op, int32_t v,
                           int64_t matWords)
{
    const bool withAgg = op != IGD_HIP_MAP_COUNT;
    const int64_t nF = db->nFiles, total = rows * nq, step = chunk_step(map_row_bytes(), nF * (withAgg ? 12 : 4));
    const int gx = (int)((nF + IGD_WAVE - 1) / IGD_WAVE);
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    for (int64_t c0 = 0; c0 < total; c0 += step) {
        const int64_t m = total - c0 < step ? total - c0 : step;
        slices.clear();
        for (int64_t r = c0 / nq; r < rows && r * nq < c0 + m; r++)
            push_slices(slices, (int32_t)r, r * nq > c0 ? r * nq : c0, (r + 1) * nq < c0 + m ? (r + 1) * nq : c0 + m, IGD_MAP_SLICE, c0);
        const int ns = (int)slices.size();
        int rc = ensure_map_ws(db, m * nF, withAgg);
        if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_grpSlices, &db->grpSliceCap, (int64_t)ns);
        if (rc == IGD_HIP_OK) rc = igd_hip_map_dev(db, c + c0, s + c0, e + c0, m, op, v, db->d_mpCount, withAgg ? db->d_mpAgg : nullptr, st);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(db->d_grpSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        igd_map_reduce<<<dim3((unsigned)gx, (unsigned)reduce_grid_y(gx, ns)), IGD_SETS_WG, 0, st>>>(db->d_mpCount, withAgg ? db->d_mpAgg : nullptr, (int)nF,
                                                                                              db->d_grpSlices, ns, (u64 *)db->d_grpStat, matWords);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));                // (the slice table is the host's vector)
    }
    return IGD_HIP_OK;
}

// the body of igd_hip_permute_map_ws and, with a pool and no ctg_len, of igd_hip_permute_map_rs
static int permute_map_run(const char *who, igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                           const PermSpec &sp, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    if (map_op_bad(who, db, op)) return IGD_HIP_ERR_ARG;
    if (perm_args_refused(who, db, ichr, qs, qe, nq, sp, false)) return IGD_HIP_ERR_ARG;
    const int64_t nF = db->nFiles, nperm = sp.nperm, R = nperm + 1;
    int64_t *const outs[3] = {n_hit, pairs, agg_sum};
    if (nq == 0 || nF == 0) {                            // every statistic is 0: no region, or no dataset
        for (int64_t *o : outs) if (o) memset(o, 0, (size_t)R * (size_t)nF * 8);
        return IGD_HIP_OK;
    }

    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    const bool fused = nF <= map_fused_max_files(op);
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    std::vector<int64_t> res((size_t)(3 * R * nF));
    int64_t perRow = 0;
    auto prepare = [&](int64_t pc, int64_t sliceLen, int64_t perRow_) -> int {
        perRow = perRow_;
        if (fused) slices = perm_row_slices(pc, nq, sliceLen);
        int rc = dev_grow(db, &db->d_grpStat, &db->grpStatCap, 3 * pc * nF);
        if (rc == IGD_HIP_OK && fused) rc = dev_grow(db, &db->d_grpSlices, &db->grpSliceCap, pc * perRow);
        return rc;
    };
    // `rows` rows counted from the region arrays (c, s, e) into zeroed matrices, which go to rows [r0, r0 + rows) of res
    auto count = [&](const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t r0) -> int {
        const int64_t matWords = rows * nF;
        if (r0 == 0 && fused) HIPCHK(hipMemcpyAsync(db->d_grpSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(db->d_grpStat, 0, (size_t)(3 * matWords) * 8, st));
        const int rc = fused ? map_fused_launch(db, im, c, s, e, (int)(rows * perRow), op, v, matWords)
                             : map_rows_reduce(db, c, s, e, rows, nq, op, v, matWords);
        if (rc != IGD_HIP_OK) return rc;
        for (int i = 0; i < 3; i++)
            HIPCHK(hipMemcpyAsync(res.data() + (i * R + r0) * nF, db->d_grpStat + i * matWords, (size_t)matWords * 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    };
    const int rc = run_perm_chunks(db, ichr, qs, qe, nq, sp, 3 * nF * 8, prepare, count);
    if (rc != IGD_HIP_OK) return rc;
    for (int i = 0; i < 3; i++)
        if (outs[i]) memcpy(outs[i], res.data() + (size_t)i * (size_t)(R * nF), (size_t)(R * nF) * 8);
    return IGD_HIP_OK;
}

extern "C" int igd_hip_permute_map_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                      const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit,
                                      int64_t *pairs, int64_t *agg_sum, const igd_hip_workspace *ws)
{
    const PermSpec sp{ctg_len, mode, seed, nperm, ws, nullptr, nullptr};
    return permute_map_run("igd_hip_permute_map", db, ichr, qs, qe, nq, sp, op, v, n_hit, pairs, agg_sum);
}

extern "C" int igd_hip_permute_map_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                      const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                                      int64_t nperm, int op, int32_t v, int64_t *n_hit, int64_t *pairs, int64_t *agg_sum)
{
    const PermPool pool{pool_ichr, pool_qs, pool_qe, npool};
    const PermSpec sp{nullptr, IGD_HIP_PERM_RESAMPLE, seed, nperm, nullptr, nullptr, &pool};
    return permute_map_run("igd_hip_permute_map_rs", db, ichr, qs, qe, nq, sp, op, v, n_hit, pairs, agg_sum);
}

extern "C" int igd_hip_permute_map(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                   const int32_t *ctg_len, int mode, uint64_t seed, int64_t nperm, int op, int32_t v, int64_t *n_hit,
                                   int64_t *pairs, int64_t *agg_sum)
{
    return igd_hip_permute_map_ws(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, op, v, n_hit, pairs, agg_sum, nullptr);
}
