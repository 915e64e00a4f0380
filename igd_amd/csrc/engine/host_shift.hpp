// engine/host_shift.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_shift_support / igd_hip_shift_regions: the support of a region set under rigid shifts (the local z-score)
// ------------------------------------------------------------------------------------------
// The shifts are a placement kind of the permutation driver (IGD_PERM_PLACE_SHIFT, host_permute.hpp): "permutation" j is the set
// moved by offsets[j], so run_perm_chunks stays the only chunk loop -- the same chunk arithmetic, the same uploads (the offsets go
// up behind the contig lengths), the slice table built and uploaded once with a shorter last chunk using its prefix.  What differs
// from the support null is what is done with a chunk's rows: nothing is folded, the rows and their totals are copied into two
// buffers of the call, asynchronously, and interleaved into the caller's matrix behind the driver's one wait.  The set as given
// is not counted (the driver's row 0 only uploads the slice table): a caller who wants it passes offset 0, which is a row like
// any other.

// THE REFUSALS OF THE TWO ENTRIES, in this order: a missing argument (extraBad: what else the entry calls one), the number of
// shifts, the first offset beyond +-2^30, more regions than a batch and -- validate -- the first region off its contig.  true,
// g_err set, prefixed with `who`.
static bool shift_args_refused(const char *who, const igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                               const int32_t *ctg_len, int32_t nctg, const int32_t *offsets, int64_t nshift, bool extraBad, bool validate)
{
    if (!db || nq < 0 || extraBad || nctg < 0 || (nq > 0 && (!ichr || !qs || !qe)) || (!ctg_len && nctg > 0) || !offsets) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return true;
    }
    if (nshift < 1 || nshift > IGD_HIP_SHIFT_MAX) {
        snprintf(g_err, sizeof g_err, "%s: %lld shifts, not 1 .. %lld", who, (long long)nshift, (long long)IGD_HIP_SHIFT_MAX);
        return true;
    }
    const int64_t j = igd_hip_shift_first_bad(offsets, nshift);
    if (j >= 0) {
        snprintf(g_err, sizeof g_err, "%s: offset %lld = %lld is beyond +-%lld", who, (long long)j, (long long)offsets[j],
                 (long long)IGD_HIP_SHIFT_MAX_OFFSET);
        return true;
    }
    if (nq > max_batch()) {
        snprintf(g_err, sizeof g_err, "%s: %lld regions, more than %lld", who, (long long)nq, (long long)max_batch());
        return true;
    }
    const int64_t i = validate ? igd_hip_perm_first_bad(ichr, qs, qe, nq, ctg_len, nctg) : -1;
    if (i >= 0)
        snprintf(g_err, sizeof g_err, "%s: region %lld = (%d, %d, %d) does not lie on its contig of length %lld", who, (long long)i,
                 (int)ichr[i], (int)qs[i], (int)qe[i], (long long)ctg_len[ichr[i]]);
    return i >= 0;
}

extern "C" int igd_hip_shift_support(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                     const int32_t *ctg_len, const int32_t *offsets, int64_t nshift, int32_t v, int rule, int64_t *shifted,
                                     const igd_hip_min_overlap *min_overlap)
{
    if (!igd_hip_min_overlap_valid(min_overlap)) {
        snprintf(g_err, sizeof g_err, "igd_hip_shift_support: min_overlap (%d bp, %d ppm, %d ppm) out of range", (int)min_overlap->min_bp,
                 (int)min_overlap->ppm_query, (int)min_overlap->ppm_record);
        return IGD_HIP_ERR_ARG;
    }
    const bool ov = igd_hip_min_overlap_active(min_overlap);
    const MinOv mo = min_ov_of(min_overlap);
    if (shift_args_refused("igd_hip_shift_support", db, ichr, qs, qe, nq, ctg_len, db ? db->nCtg : 0, offsets, nshift,
                           !shifted || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT), true))
        return IGD_HIP_ERR_ARG;
    const int64_t nF = db->nFiles, nC = nF + 1;
    if (nq == 0 || nF == 0) {
        memset(shifted, 0, (size_t)(nshift * nC) * 8);
        return IGD_HIP_OK;
    }

    const SliceImage im = slice_image(db, rule, v);
    const int64_t maxGrid = support_max_grid(db);
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    std::vector<int64_t> rowsHome((size_t)(nshift * nF)), totHome((size_t)nshift);
    int64_t perRow = 0;
    auto prepare = [&](int64_t pc, int64_t sliceLen, int64_t perRow_) -> int {
        perRow = perRow_;
        slices = perm_row_slices(pc, nq, sliceLen);
        int rc = sets_ws(db, pc * nF, pc, pc * perRow);
        if (rc == IGD_HIP_OK) rc = ensure_support_bits(db, maxGrid);
        return rc;
    };
    // row 0 of the driver: only the slice table goes up.  A chunk: `rows` zeroed rows counted from the staging arrays -- rows *
    // perRow slices, a prefix of the table -- and sent home as rows [r0 - 1, r0 - 1 + rows) of the call's two buffers.
    auto count = [&](const int32_t *c, const int32_t *s, const int32_t *e, int64_t rows, int64_t r0) -> int {
        if (r0 == 0) {
            HIPCHK(hipMemcpyAsync(db->d_setSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
            return IGD_HIP_OK;
        }
        const int ns = (int)(rows * perRow);
        const int grid = ns < maxGrid ? ns : (int)maxGrid;
        HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
        HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
        const int rc = support_launch(db, im, c, s, e, ns, grid, v, ov, mo);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(rowsHome.data() + (r0 - 1) * nF, db->d_setRows, (size_t)(rows * nF) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(totHome.data() + (r0 - 1), db->d_setTot, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    };
    const PermSpec sp{ctg_len, IGD_PERM_PLACE_SHIFT, 0, nshift, nullptr, offsets, nullptr};
    const int rc = run_perm_chunks(db, ichr, qs, qe, nq, sp, nF * 8, prepare, count);
    if (rc != IGD_HIP_OK) return rc;
    for (int64_t j = 0; j < nshift; j++) {
        memcpy(shifted + j * nC, rowsHome.data() + j * nF, (size_t)nF * 8);
        shifted[j * nC + nF] = totHome[(size_t)j];
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_shift_regions(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq,
                                     const int32_t *ctg_len, int32_t nctg, const int32_t *offsets, int64_t nshift, int32_t *out_qs,
                                     int32_t *out_qe)
{
    if (shift_args_refused("igd_hip_shift_regions", db, ichr, qs, qe, nq, ctg_len, nctg, offsets, nshift,
                           nq > 0 && nshift > 0 && (!out_qs || !out_qe), false))
        return IGD_HIP_ERR_ARG;
    if (nq > 0 && nshift > (int64_t)INT32_MAX / nq) {
        snprintf(g_err, sizeof g_err, "igd_hip_shift_regions: %lld shifts of %lld regions, more than 2^31 - 1 outputs", (long long)nshift,
                 (long long)nq);
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    const int64_t pc = max_batch() / nq < nshift ? max_batch() / nq : nshift;
    std::vector<int32_t> hs((size_t)(nshift * nq)), he((size_t)(nshift * nq));
    HIPCHK(hipSetDevice(db->device));
    int rc = ensure_qstage(db, pc * nq);
    PermPlace pl;
    if (rc == IGD_HIP_OK)
        rc = perm_place_upload(db, ichr, qs, qe, nq, nctg, PermSpec{ctg_len, IGD_PERM_PLACE_SHIFT, 0, nshift, nullptr, offsets, nullptr}, &pl);
    if (rc != IGD_HIP_OK) return rc;
    int32_t *const home[3] = {nullptr, hs.data(), he.data()}, *const out[3] = {nullptr, out_qs, out_qe};
    return perm_regions_home(db, pl, 0, 0, nshift, pc, home, out);
}
