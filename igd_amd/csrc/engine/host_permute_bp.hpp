// engine/host_permute_bp.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_permute_bp / igd_hip_merge_slices_per_row: the permutation null of the base-pair overlap (the definitions are in
// include/igd_hip.h), on the resident hand-over of permute_bp_dev.hpp
// ------------------------------------------------------------------------------------------
// igd_hip_permute_support_ov's driver (host_permute.hpp) with a merge in front of the counting kernel.  The regions and ctg_len go
// up once (db->d_pmReg); the offsets set_off[r] = r nq are written once, for pc + 1 rows, and row 0 and a shorter last chunk
// take a prefix of them.  A chunk holds pc permutations with pc * nq <= igd_hip_max_batch() and pc * nFiles * 8 <=
// perm_row_bytes().  Per chunk, on the engine's stream and without a wait or a host copy in between: igd_permute_regions into
// the staging arrays (row 0: the regions themselves), merge_launches (host_merge.hpp; the handle's shared merge workspace,
// runs into this stage's own arrays db->d_pbRun / d_pbWord), igd_merge_slices, a memset of the chunk's rows, igd_sets_coverage
// with the launch logic of igd_hip_coverage_sets, igd_merge_row_bp, and asynchronous copies of the rows, covered[], set_bp[]
// and n_merged[] into a buffer of this file.  One wait at the end; the caller's arrays are written behind it, so on an error
// nothing is.  The wide form's tags are budgeted by the upper bound rows * nq: a wave numbers the runs it meets, and a row
// has at most nq.
// Every merge of a handle works in ONE workspace (host_merge.hpp): all of this is on the engine's stream, as
// igd_hip_merge_sets and igd_hip_jaccard_sets are, so the ordering rule holds.

// slice slots a row gets when pc rows of nq regions are handed over in one chunk (tests)
extern "C" int64_t igd_hip_merge_slices_per_row(int64_t pc, int64_t nq)
{
    if (pc < 1 || nq < 1 || pc > INT64_MAX / nq) return 0;
    const int64_t sliceLen = sets_slice_len(pc * nq);
    return (nq + sliceLen - 1) / sliceLen;
}

extern "C" int igd_hip_permute_bp_ws(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                                     int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp,
                                     int64_t *n_merged, int64_t *n_dropped, const igd_hip_workspace *ws)
{
    if (!db || nq < 0 || (nq > 0 && (!ichr || !qs || !qe)) || (!ctg_len && db->nCtg > 0) ||
        (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) || !perm_mode_ok(mode, ws)) {
        snprintf(g_err, sizeof g_err, "igd_hip_permute_bp: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nperm < 1 || nperm > IGD_HIP_PERM_MAX) {
        snprintf(g_err, sizeof g_err, "igd_hip_permute_bp: %lld permutations, not 1 .. %lld", (long long)nperm, (long long)IGD_HIP_PERM_MAX);
        return IGD_HIP_ERR_ARG;
    }
    if (nq > max_batch()) {
        snprintf(g_err, sizeof g_err, "igd_hip_permute_bp: %lld regions, more than %lld", (long long)nq, (long long)max_batch());
        return IGD_HIP_ERR_ARG;
    }
    for (int64_t i = 0; i < nq; i++) {
        const int32_t c = ichr[i];
        if (c < 0 || c >= db->nCtg) continue;
        const int64_t L = ctg_len[c];
        if (L < 1 || qs[i] < 0 || qe[i] < qs[i] || (int64_t)qe[i] > L) {
            snprintf(g_err, sizeof g_err, "igd_hip_permute_bp: region %lld = (%d, %d, %d) does not lie on its contig of length %lld",
                     (long long)i, (int)c, (int)qs[i], (int)qe[i], (long long)L);
            return IGD_HIP_ERR_ARG;
        }
    }
    if (perm_ws_refused("igd_hip_permute_bp", ws, ctg_len, db->nCtg, ichr, qs, qe, nq, true)) return IGD_HIP_ERR_ARG;
    const int64_t nF = db->nFiles, nC = nF + 1, R = nperm + 1;
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
    int64_t pc = max_batch() / nq;
    if (nF > 0) {
        const int64_t byRows = perm_row_bytes() / (nF * 8);
        if (byRows < pc) pc = byRows < 1 ? 1 : byRows;
    }
    if (nperm < pc) pc = nperm;
    const int64_t sliceLen = sets_slice_len(pc * nq);
    const int64_t perRow = (nq + sliceLen - 1) / sliceLen;                // slice slots of one row
    const int64_t maxGrid = lds ? IGD_SETS_GRID : wide_grid(IGD_COVERAGE_FRONT_BYTES, nF * 8 * (IGD_SETS_WG / IGD_WAVE));
    // the call's results: cov[R][nF], any[R], set_bp[R], n_merged[R], n_dropped
    std::vector<int64_t> res((size_t)(R * nF + 3 * R + 1), 0);
    int64_t *hCov = res.data(), *hAny = hCov + R * nF, *hBp = hAny + R, *hRuns = hBp + R, *hDrop = hRuns + R;

    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    MergeWs w;
    int rc = dev_grow(db, &db->d_pmReg, &db->pmRegCap, 3 * nq + db->nCtg);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_pbRun, &db->pbRunCap, 3 * pc * nq);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_pbWord, &db->pbWordCap, 5 * pc + 2);
    if (rc == IGD_HIP_OK) rc = ensure_qstage(db, pc * nq);
    if (rc == IGD_HIP_OK) rc = sets_ws(db, pc * nF, pc, pc * perRow);
    if (rc == IGD_HIP_OK) rc = merge_ws(db, pc * nq, (int32_t)pc, false, &w);       // (the largest chunk: carved per chunk below)
    PermPlace pl;
    if (rc == IGD_HIP_OK) rc = perm_place_upload(db, mode, ws, &pl);
    if (rc != IGD_HIP_OK) return rc;
    int32_t *rC = db->d_pmReg, *rS = rC + nq, *rE = rS + nq, *rL = rE + nq;
    int32_t *mC = db->d_pbRun, *mS = mC + pc * nq, *mE = mS + pc * nq;
    int64_t *dSetOff = db->d_pbWord, *dMOff = dSetOff + pc + 1, *dDrop = dMOff + pc + 1, *dBp = dDrop + pc, *dRuns = dBp + pc;
    HIPCHK(hipMemcpyAsync(rC, ichr, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(rS, qs, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(rE, qe, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    if (db->nCtg > 0) HIPCHK(hipMemcpyAsync(rL, ctg_len, (size_t)db->nCtg * 4, hipMemcpyHostToDevice, st));
    igd_merge_row_offsets<<<grid_of(pc + 1, IGD_MERGE_WG), IGD_MERGE_WG, 0, st>>>(nq, pc, dSetOff);
    HIPCHK(hipGetLastError());

    // `rows` rows of nq regions each (c, s, e) merged, covered and summed; the results go to rows [r0, r0 + rows) of res
    auto count = [&](const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t r0) -> int {
        const int64_t n = rows * nq;
        const MergeWs cw = merge_layout(db->d_merge, n, (int32_t)rows, false);
        int rc2 = merge_launches(db, cw, c, s, e, dSetOff, (int32_t)rows, n, 0, mC, mS, mE, dMOff, nullptr, dDrop, st);
        if (rc2 != IGD_HIP_OK) return rc2;
        if (nF > 0) {
            const int64_t ns = rows * perRow;
            unsigned tag0 = 0;
            if (!lds && (rc2 = coverage_fronts(db, maxGrid * (IGD_SETS_WG / IGD_WAVE) * nF, n, &tag0)) != IGD_HIP_OK) return rc2;
            igd_merge_slices<<<grid_of(ns, IGD_MERGE_WG), IGD_MERGE_WG, 0, st>>>(dMOff, rows, perRow, sliceLen, db->d_setSlices);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
            HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
            if ((rc2 = coverage_launch(db, im, mC, mS, mE, (int)ns, (int)(ns < maxGrid ? ns : maxGrid), v, tag0)) != IGD_HIP_OK) return rc2;
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hCov + r0 * nF, db->d_setRows, (size_t)(rows * nF) * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(hAny + r0, db->d_setTot, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        }
        igd_merge_row_bp<<<grid_of(rows, IGD_MERGE_WG / WAVE), IGD_MERGE_WG, 0, st>>>(mS, mE, dMOff, rows, dBp, dRuns);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hBp + r0, dBp, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hRuns + r0, dRuns, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    };

    if ((rc = count(rC, rS, rE, 1, 0)) != IGD_HIP_OK) return rc;         // the set as given
    HIPCHK(hipMemcpyAsync(hDrop, dDrop, 8, hipMemcpyDeviceToHost, st));
    for (int64_t p0 = 0; p0 < nperm; p0 += pc) {
        const int64_t n = nperm - p0 < pc ? nperm - p0 : pc;
        if ((rc = permute_launch(db, pl, rC, rS, rE, nq, rL, db->nCtg, (u64)seed, (u64)p0, n * nq, db->d_qc, db->d_qs, db->d_qe)) != IGD_HIP_OK) return rc;
        if ((rc = count(db->d_qc, db->d_qs, db->d_qe, n, 1 + p0)) != IGD_HIP_OK) return rc;
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
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

extern "C" int igd_hip_permute_bp(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, const int32_t *ctg_len,
                                  int mode, uint64_t seed, int64_t nperm, int32_t v, int rule, int64_t *inter, int64_t *set_bp,
                                  int64_t *n_merged, int64_t *n_dropped)
{
    return igd_hip_permute_bp_ws(db, ichr, qs, qe, nq, ctg_len, mode, seed, nperm, v, rule, inter, set_bp, n_merged, n_dropped, nullptr);
}
