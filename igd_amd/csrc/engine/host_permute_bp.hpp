// engine/host_permute_bp.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_permute_bp / igd_hip_merge_slices_per_row: the permutation null of the base-pair overlap (the definitions are in
// include/igd_hip.h), on the resident hand-over of permute_bp_dev.hpp
// ------------------------------------------------------------------------------------------
// Runs in run_perm_chunks (host_permute.hpp: refusals, upload, chunks, the wait) with a merge in front of the counting kernel
// and nFiles * 8 bytes of rows per permutation (no row budget without files).  The offsets set_off[r] = r nq are written once,
// for pc + 1 rows, and row 0 and a shorter last chunk take a prefix of them.  Per chunk, without a wait or a host copy in
// between: merge_launches over the staged rows (host_merge.hpp; the handle's shared merge workspace, runs into this stage's own
// arrays db->d_pbRun / d_pbWord), igd_merge_slices, a memset of the chunk's rows, igd_sets_coverage with the launch logic of
// igd_hip_coverage_sets, igd_merge_row_bp, and asynchronous copies of the rows, covered[], set_bp[] and n_merged[] into a buffer
// of this file.  The caller's arrays are written behind the driver's wait, so on an error nothing is.  The wide form's tags are
// budgeted by the upper bound rows * nq: a wave numbers the runs it meets, and a row has at most nq.
// Every merge of a handle works in ONE workspace (host_merge.hpp): all of this is on the engine's stream, as
// igd_hip_merge_sets and igd_hip_jaccard_sets are, so the ordering rule holds.

// slice slots a row gets when pc rows of nq regions are handed over in one chunk (tests)
extern "C" int64_t igd_hip_merge_slices_per_row(int64_t pc, int64_t nq)
{
    if (pc < 1 || nq < 1 || pc > INT64_MAX / nq) return 0;
    const int64_t sliceLen = sets_slice_len(pc * nq);
    return (nq + sliceLen - 1) / sliceLen;
}

// the body of igd_hip_permute_bp_ws and, with a pool and no ctg_len, of igd_hip_permute_bp_rs (whose drawn rows drop what their own
// regions make them drop; n_dropped stays row 0's)
static int permute_bp_run(const char *who, igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                          const PermSpec &sp, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged, int64_t *n_dropped)
{
    if (perm_args_refused(who, db, ichr, qs, qe, nq, sp, rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) return IGD_HIP_ERR_ARG;
    const int64_t nF = db->nFiles, nC = nF + 1, R = sp.nperm + 1;
    if (nq == 0) {                                       // no region: no run, no base pair
        if (inter) memset(inter, 0, (size_t)R * (size_t)nC * 8);
        if (set_bp) memset(set_bp, 0, (size_t)R * 8);
        if (n_merged) memset(n_merged, 0, (size_t)R * 8);
        if (n_dropped) *n_dropped = 0;
        return IGD_HIP_OK;
    }

    // (TEST-ONLY: IGD_HIP_MERGE_GRID, read once per process as in merge_launches, gives the kernels of permute_bp_dev.hpp a second round)
    static const int64_t mergeGrid = env_positive("IGD_HIP_MERGE_GRID", IGD_MERGE_GRID);
    auto grid_of = [](int64_t items, int64_t per) { const int64_t g = (items + per - 1) / per; return (unsigned)(g < 1 ? 1 : g < mergeGrid ? g : mergeGrid); };
    const SliceImage im = slice_image(db, rule, v);
    const bool lds = nF <= IGD_COVERAGE_LDS_FILES;
    const int64_t maxGrid = lds ? IGD_SETS_GRID : wide_grid(IGD_COVERAGE_FRONT_BYTES, nF * 8 * (IGD_SETS_WG / IGD_WAVE));
    hipStream_t st = db->stream;
    // the call's results: cov[R][nF], any[R], set_bp[R], n_merged[R], n_dropped
    std::vector<int64_t> res((size_t)(R * nF + 3 * R + 1), 0);
    int64_t *hCov = res.data(), *hAny = hCov + R * nF, *hBp = hAny + R, *hRuns = hBp + R, *hDrop = hRuns + R;
    int64_t pc = 0, sliceLen = 0, perRow = 0;            // the driver's chunk: permutations, regions per slice, slice slots of one row
    auto prepare = [&](int64_t pc_, int64_t sliceLen_, int64_t perRow_) -> int {
        pc = pc_; sliceLen = sliceLen_; perRow = perRow_;
        MergeWs w;
        int rc = dev_grow(db, &db->d_pbRun, &db->pbRunCap, 3 * pc * nq);
        if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_pbWord, &db->pbWordCap, 5 * pc + 2);
        if (rc == IGD_HIP_OK) rc = sets_ws(db, pc * nF, pc, pc * perRow);
        if (rc == IGD_HIP_OK) rc = merge_ws(db, pc * nq, (int32_t)pc, false, &w);   // (the largest chunk: carved per chunk below)
        return rc;
    };
    // `rows` rows of nq regions each (c, s, e) merged, covered and summed; the results go to rows [r0, r0 + rows) of res.  Row 0
    // writes the offsets set_off[r] = r nq first, and takes the regions the merge dropped home.
    auto count = [&](const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t r0) -> int {
        const int64_t n = rows * nq;
        int32_t *mC = db->d_pbRun, *mS = mC + pc * nq, *mE = mS + pc * nq;
        int64_t *dSetOff = db->d_pbWord, *dMOff = dSetOff + pc + 1, *dDrop = dMOff + pc + 1, *dBp = dDrop + pc, *dRuns = dBp + pc;
        if (r0 == 0) {
            igd_merge_row_offsets<<<grid_of(pc + 1, IGD_MERGE_WG), IGD_MERGE_WG, 0, st>>>(nq, pc, dSetOff);
            HIPCHK(hipGetLastError());
        }
        const MergeWs cw = merge_layout(db->d_merge, n, (int32_t)rows, false);
        int rc = merge_launches(db, cw, c, s, e, dSetOff, (int32_t)rows, n, 0, mC, mS, mE, dMOff, nullptr, dDrop, st);
        if (rc != IGD_HIP_OK) return rc;
        if (nF > 0) {
            const int64_t ns = rows * perRow;
            unsigned tag0 = 0;
            if (!lds && (rc = coverage_fronts(db, maxGrid * (IGD_SETS_WG / IGD_WAVE) * nF, n, &tag0)) != IGD_HIP_OK) return rc;
            igd_merge_slices<<<grid_of(ns, IGD_MERGE_WG), IGD_MERGE_WG, 0, st>>>(dMOff, rows, perRow, sliceLen, db->d_setSlices);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
            HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
            if ((rc = coverage_launch(db, im, mC, mS, mE, (int)ns, (int)(ns < maxGrid ? ns : maxGrid), v, tag0)) != IGD_HIP_OK) return rc;
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hCov + r0 * nF, db->d_setRows, (size_t)(rows * nF) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(hAny + r0, db->d_setTot, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        }
        igd_merge_row_bp<<<grid_of(rows, IGD_MERGE_WG / WAVE), IGD_MERGE_WG, 0, st>>>(mS, mE, dMOff, rows, dBp, dRuns);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hBp + r0, dBp, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hRuns + r0, dRuns, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        if (r0 == 0) HIPCHK(hipMemcpyAsync(hDrop, dDrop, 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    };
    const int rc = run_perm_chunks(db, ichr, qs, qe, nq, sp, nF * 8, prepare, count);
    if (rc != IGD_HIP_OK) return rc;
    if (inter)
        for (int64_t r = 0; r < R; r++) {
            memcpy(inter + r * nC, hCov + r * nF, (size_t)nF * 8);
            inter[r * nC + nF] = hAny[r];
        }
    if (set_bp) memcpy(set_bp, hBp, (size_t)R * 8);
    if (n_merged) memcpy(n_merged, hRuns, (size_t)R * 8);
    if (n_dropped) *n_dropped = *hDrop;
    return IGD_HIP_OK;
}

extern "C" int igd_hip_permute_bp_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                                     int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp,
                                     int64_t *n_merged, int64_t *n_dropped, const igd_hip_workspace *ws)
{
    const PermSpec sp{ctg_len, mode, seed, nperm, ws, nullptr, nullptr};
    return permute_bp_run("igd_hip_permute_bp", db, ichr, qs, qe, nq, sp, v, rule, inter, set_bp, n_merged, n_dropped);
}

extern "C" int igd_hip_permute_bp_rs(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                     const int32_t *pool_ichr, const int32_t *pool_qs, const int32_t *pool_qe, int64_t npool, uint64_t seed,
                                     int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *n_merged,
                                     int64_t *n_dropped)
{
    const PermPool pool{pool_ichr, pool_qs, pool_qe, npool};
    const PermSpec sp{nullptr, IGD_HIP_PERM_RESAMPLE, seed, nperm, nullptr, nullptr, &pool};
    return permute_bp_run("igd_hip_permute_bp_rs", db, ichr, qs, qe, nq, sp, v, rule, inter, set_bp, n_merged, n_dropped);
}

extern "C" int igd_hip_permute_bp(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                                  int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp,
                                  int64_t *n_merged, int64_t *n_dropped)
{
    return igd_hip_permute_bp_ws(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter, set_bp, n_merged, n_dropped, nullptr);
}
