// engine/host_rank.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_enrich_ranks: rank columns and Benjamini-Hochberg q-values of an enrichment table (igd_rank_rows, rank_dev.hpp)
// ------------------------------------------------------------------------------------------
// The table comes as three host matrices [nrows x ncols]; ncols is the caller's, not the database's.  Rows go through the
// kernel in CHUNKS of whole rows of at most IGD_RANK_CHUNK cells (a wider row alone), one launch per chunk on the engine's
// stream: the needed inputs up, the requested outputs straight into the caller's arrays at their place.  The workspace
// is the handle's enrichment workspace (d_fisher, dev_grow): per cell of a chunk 7 words -- three inputs, q, mean and
// four int32 rank rows -- and, for rows wider than IGD_RANK_LDS_COLS, the workgroups' sort slices (1.5 words per padded cell).
#define IGD_RANK_CHUNK ((int64_t)1 << 20)

// workgroups igd_rank_rows is launched with for nrows rows: a workgroup takes a second row only beyond the grid
extern "C" int32_t igd_hip_rank_grid(int64_t nrows)
{
    return (int32_t)(nrows < 1 ? 1 : nrows < IGD_SETS_GRID ? nrows : IGD_SETS_GRID);
}
// the widest row whose keys and indices the kernel keeps in LDS
extern "C" int32_t igd_hip_rank_lds_cols(void) { return IGD_RANK_LDS_COLS; }

extern "C" int igd_hip_enrich_ranks(igd_hip_db *db, const int64_t *support, const double *pvalue_log, const double *odds_ratio,
                                    int64_t nrows, int64_t ncols, double *qvalue_log, int32_t *rnk_sup, int32_t *rnk_pv,
                                    int32_t *rnk_or, int32_t *max_rnk, double *mean_rnk)
{
    const bool mm = max_rnk || mean_rnk;
    const int what = (rnk_sup || mm ? IGD_RANK_DO_SUP : 0) | (rnk_pv || qvalue_log || mm ? IGD_RANK_DO_PV : 0) |
                     (rnk_or || mm ? IGD_RANK_DO_OR : 0) | (qvalue_log ? IGD_RANK_DO_Q : 0) | (mm ? IGD_RANK_DO_MM : 0);
    if (!db || nrows < 0 || ncols < 0) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_ranks: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (ncols > IGD_RANK_MAX_COLS) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_ranks: %lld columns, more than 2^20", (long long)ncols);
        return IGD_HIP_ERR_ARG;
    }
    if (nrows == 0 || ncols == 0 || what == 0) return IGD_HIP_OK;
    if (((what & IGD_RANK_DO_SUP) && !support) || ((what & IGD_RANK_DO_PV) && !pvalue_log) || ((what & IGD_RANK_DO_OR) && !odds_ratio)) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_ranks: a requested output needs an input that is NULL");
        return IGD_HIP_ERR_ARG;
    }
    if (nrows > INT64_MAX / ncols) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_ranks: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (what & IGD_RANK_DO_PV)
        for (int64_t i = 0; i < nrows * ncols; i++)
            if (!(pvalue_log[i] >= 0.0)) {
                snprintf(g_err, sizeof g_err, "igd_hip_enrich_ranks: pvalue_log[%lld] is negative or NaN", (long long)i);
                return IGD_HIP_ERR_ARG;
            }
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    const int m = (int)ncols;
    int n = 1;
    while (n < m) n <<= 1;
    const bool lds = m <= IGD_RANK_LDS_COLS;
    const int64_t rowsPer = IGD_RANK_CHUNK / ncols > 0 ? IGD_RANK_CHUNK / ncols : 1;
    const int64_t step = nrows < rowsPer ? nrows : rowsPer, cells = step * ncols;
    const int32_t maxGrid = igd_hip_rank_grid(step);
    const int64_t sortWords = lds ? 0 : (int64_t)maxGrid * n + ((int64_t)maxGrid * n + 1) / 2;
    int rc = dev_grow(db, &db->d_fisher, &db->fisherCap, 7 * cells + sortWords);
    if (rc != IGD_HIP_OK) return rc;
    int64_t *dS = db->d_fisher;
    double *dP = (double *)(dS + cells), *dO = dP + cells, *dQ = dO + cells, *dMean = dQ + cells;
    int32_t *dRs = (int32_t *)(dMean + cells), *dRp = dRs + cells, *dRo = dRp + cells, *dMax = dRo + cells;
    u64 *dKey = (u64 *)(db->d_fisher + 7 * cells);       // (the four int32 rows are 2 words per cell)
    unsigned *dIdx = (unsigned *)(dKey + (int64_t)maxGrid * n);
    const size_t ldsB = IGD_RANK_SCR_BYTES + (lds ? (size_t)n * 12 : 0);
    if (ldsB > (size_t)65536)                            // (more dynamic LDS than a launch gets unasked)
        (void)hipFuncSetAttribute((const void *)igd_rank_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
    for (int64_t r0 = 0; r0 < nrows; r0 += step) {
        const int64_t rows = nrows - r0 < step ? nrows - r0 : step, c = rows * ncols, o = r0 * ncols;
        if (what & IGD_RANK_DO_SUP) HIPCHK(hipMemcpyAsync(dS, support + o, (size_t)c * 8, hipMemcpyHostToDevice, st));
        if (what & IGD_RANK_DO_PV) HIPCHK(hipMemcpyAsync(dP, pvalue_log + o, (size_t)c * 8, hipMemcpyHostToDevice, st));
        if (what & IGD_RANK_DO_OR) HIPCHK(hipMemcpyAsync(dO, odds_ratio + o, (size_t)c * 8, hipMemcpyHostToDevice, st));
        const int grid = igd_hip_rank_grid(rows);
        if (lds) igd_rank_rows<true><<<grid, IGD_SETS_WG, ldsB, st>>>(dS, dP, dO, rows, m, n, what, nullptr, nullptr, dQ, dRs, dRp, dRo, dMax, dMean);
        else igd_rank_rows<false><<<grid, IGD_SETS_WG, ldsB, st>>>(dS, dP, dO, rows, m, n, what, dKey, dIdx, dQ, dRs, dRp, dRo, dMax, dMean);
        HIPCHK(hipGetLastError());
        if (qvalue_log) HIPCHK(hipMemcpyAsync(qvalue_log + o, dQ, (size_t)c * 8, hipMemcpyDeviceToHost, st));
        if (rnk_sup) HIPCHK(hipMemcpyAsync(rnk_sup + o, dRs, (size_t)c * 4, hipMemcpyDeviceToHost, st));
        if (rnk_pv) HIPCHK(hipMemcpyAsync(rnk_pv + o, dRp, (size_t)c * 4, hipMemcpyDeviceToHost, st));
        if (rnk_or) HIPCHK(hipMemcpyAsync(rnk_or + o, dRo, (size_t)c * 4, hipMemcpyDeviceToHost, st));
        if (max_rnk) HIPCHK(hipMemcpyAsync(max_rnk + o, dMax, (size_t)c * 4, hipMemcpyDeviceToHost, st));
        if (mean_rnk) HIPCHK(hipMemcpyAsync(mean_rnk + o, dMean, (size_t)c * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}
