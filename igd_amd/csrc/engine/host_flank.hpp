// engine/host_flank.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_flank / igd_hip_flank_dev / igd_hip_flank_reldist: the nearest record on each side per dataset within a window and the
// histogram of the relative distance per set and dataset (flank_dev.hpp; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// The three forms of host_nearest.hpp with two rows per region.  The device form: one launch of igd_flank_rows (the wide form:
// a fill of both rows with 0xff before it and igd_nearest_rowmin behind it for each minimum that is wanted), asynchronous on the
// caller's stream.  The host form: run_region_chunks (host_common.hpp) with chunks of chunk_step(nearest_row_bytes(), 8 nFiles)
// regions -- at most igd_hip_max_batch() regions and IGD_NEAREST_ROW_BYTES / (8 nFiles) -- whose rows lie in the workspace of
// igd_hip_nearest, d_nrDist (the up rows of the chunk, then its down rows) and d_nrMin (upmin, then downmin).  The sets form:
// run_set_groups (host_nearest.hpp), the driver of igd_hip_nearest_hist, with a chunk functor that launches igd_flank_rows and
// igd_flank_reldist, the reduction into ONE resident matrix of B x (nFiles + 1) words per set in d_grpStat; slices of at most
// IGD_NEAREST_SLICE = 256 regions, so the kernel's u32 LDS counters hold at most 256.
// The image is slice_image(db, IGD_HIP_RULE_FLAT, v), as for igd_hip_nearest.

static int flank_args_bad(const char *who, int32_t window, int measure)
{
    if (nearest_window_bad(who, window)) return 1;
    if (igd_hip_flank_measure_valid(measure)) return 0;
    snprintf(g_err, sizeof g_err, "%s: measure %d is neither IGD_HIP_FLANK_EDGES nor IGD_HIP_FLANK_MIDPOINTS", who, measure);
    return 1;
}

// one engine batch of resident regions into resident rows (the arguments are checked, nq > 0)
static int flank_rows_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int32_t window,
                          int measure, int32_t v, int32_t *d_up, int32_t *d_down, int32_t *d_upmin, int32_t *d_downmin, hipStream_t st)
{
    const int64_t nF = db->nFiles;
    if (nF == 0) {                                       // rows of no words; no region has a dataset on either side
        if (d_upmin) HIPCHK(hipMemsetAsync(d_upmin, 0xff, (size_t)nq * 4, st));
        if (d_downmin) HIPCHK(hipMemsetAsync(d_downmin, 0xff, (size_t)nq * 4, st));
        return IGD_HIP_OK;
    }
    const SliceImage im = slice_image(db, IGD_HIP_RULE_FLAT, v);
    const bool lds = nF <= IGD_FLANK_LDS_FILES;
    const int grid = igd_hip_nearest_grid(nq);
    const size_t ldsB = lds ? (size_t)(2 * (IGD_SETS_WG / IGD_WAVE) * nF) * 4 : 0;
    const int n = (int)nq;
    if (!lds) {                                          // the wide form minimises into rows of "none"
        HIPCHK(hipMemsetAsync(d_up, 0xff, (size_t)(nq * nF) * 4, st));
        HIPCHK(hipMemsetAsync(d_down, 0xff, (size_t)(nq * nF) * 4, st));
    }
    with_flags(im.useV, lds, [&](auto V, auto L) {
        if (measure == IGD_HIP_FLANK_MIDPOINTS)
            igd_flank_rows<V(), L(), true><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, d_ichr, d_qs, d_qe, n, window, im.krule, v, d_up, d_down, d_upmin, d_downmin);
        else
            igd_flank_rows<V(), L(), false><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, d_ichr, d_qs, d_qe, n, window, im.krule, v, d_up, d_down, d_upmin, d_downmin);
    });
    HIPCHK(hipGetLastError());
    if (!lds && d_upmin) {
        igd_nearest_rowmin<<<grid, IGD_SETS_WG, 0, st>>>(d_up, n, (int)nF, d_upmin);
        HIPCHK(hipGetLastError());
    }
    if (!lds && d_downmin) {
        igd_nearest_rowmin<<<grid, IGD_SETS_WG, 0, st>>>(d_down, n, (int)nF, d_downmin);
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_flank_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, int64_t nq, int32_t window,
                                 int measure, int32_t v, int32_t *d_up, int32_t *d_down, int32_t *d_upmin, int32_t *d_downmin, void *stream)
{
    if (flank_args_bad("igd_hip_flank_dev", window, measure)) return IGD_HIP_ERR_ARG;
    if (!db || nq < 0 || nq > max_batch() || (nq > 0 && (!d_ichr || !d_qs || !d_qe || ((!d_up || !d_down) && db->nFiles > 0)))) {
        snprintf(g_err, sizeof g_err, "igd_hip_flank_dev: bad argument (batch limit %lld regions)", (long long)max_batch());
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    return flank_rows_dev(db, d_ichr, d_qs, d_qe, nq, window, measure, v, d_up, d_down, d_upmin, d_downmin, stream ? (hipStream_t)stream : db->stream);
}

extern "C" int igd_hip_flank(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int32_t window,
                             int measure, int32_t v, int32_t *up, int32_t *down, int32_t *upmin, int32_t *downmin)
{
    if (flank_args_bad("igd_hip_flank", window, measure)) return IGD_HIP_ERR_ARG;
    if (!db || nq < 0 || (nq > 0 && (!ichr || !qs || !qe || ((!up || !down) && db->nFiles > 0)))) {
        snprintf(g_err, sizeof g_err, "igd_hip_flank: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0) return IGD_HIP_OK;
    const int64_t nF = db->nFiles;
    if (nF == 0) {
        if (upmin) memset(upmin, 0xff, (size_t)nq * 4);
        if (downmin) memset(downmin, 0xff, (size_t)nq * 4);
        return IGD_HIP_OK;
    }
    return run_region_chunks(db, ichr, qs, qe, nq, chunk_step(nearest_row_bytes(), nF * 8), [&](int64_t c0, int64_t m, hipStream_t st) {
        int rc = ensure_nearest_ws(db, 2 * m * nF, 2 * m);
        if (rc == IGD_HIP_OK) rc = flank_rows_dev(db, db->d_qc, db->d_qs, db->d_qe, m, window, measure, v, db->d_nrDist, db->d_nrDist + m * nF,
                                                  upmin ? db->d_nrMin : nullptr, downmin ? db->d_nrMin + m : nullptr, st);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(up + c0 * nF, db->d_nrDist, (size_t)(m * nF) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(down + c0 * nF, db->d_nrDist + m * nF, (size_t)(m * nF) * 4, hipMemcpyDeviceToHost, st));
        if (upmin) HIPCHK(hipMemcpyAsync(upmin + c0, db->d_nrMin, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        if (downmin) HIPCHK(hipMemcpyAsync(downmin + c0, db->d_nrMin + m, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        return IGD_HIP_OK;
    });
}

extern "C" int igd_hip_flank_reldist(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                     int32_t nsets, int32_t window, int measure, int32_t v, int32_t nbins, int64_t *hist)
{
    if (flank_args_bad("igd_hip_flank_reldist", window, measure)) return IGD_HIP_ERR_ARG;
    if (!igd_hip_flank_bins_valid(nbins)) {
        snprintf(g_err, sizeof g_err, "igd_hip_flank_reldist: %d bins outside 1 .. %d", (int)nbins, (int)IGD_HIP_FLANK_MAX_BINS);
        return IGD_HIP_ERR_ARG;
    }
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !hist))) {
        snprintf(g_err, sizeof g_err, "igd_hip_flank_reldist: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_flank_reldist", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles, nC = nF + 1, matRow = (int64_t)nbins * nC;
    if (set_off[nsets] == 0 || nF == 0) {                // no region, or no dataset on either side: no pair is flanked
        memset(hist, 0, (size_t)nsets * (size_t)matRow * 8);
        return IGD_HIP_OK;
    }
    int64_t *outs[1] = {hist};
    return run_set_groups(db, ichr, qs, qe, set_off, nsets, chunk_step(nearest_row_bytes(), nF * 8), IGD_NEAREST_SLICE, 1, matRow, outs, nC,
                          [&](dim3 grid, int ns, int64_t, int64_t m, hipStream_t st) {
        int rc2 = ensure_nearest_ws(db, 2 * m * nF, 2 * m);
        if (rc2 == IGD_HIP_OK) rc2 = flank_rows_dev(db, db->d_qc, db->d_qs, db->d_qe, m, window, measure, v, db->d_nrDist, db->d_nrDist + m * nF, db->d_nrMin,
                                                    db->d_nrMin + m, st);
        if (rc2 != IGD_HIP_OK) return rc2;
        igd_flank_reldist<<<grid, IGD_SETS_WG, 0, st>>>(db->d_nrDist, db->d_nrDist + m * nF, db->d_nrMin, db->d_nrMin + m, (int)nF, db->d_grpSlices, ns,
                                                        (int)nbins, (u64 *)db->d_grpStat);
        return IGD_HIP_OK;
    });
}
