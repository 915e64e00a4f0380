// engine/host_enrich.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_fisher_tables / igd_hip_enrich_sets: Fisher's exact test over 2x2 tables (igd_fisher_cells, fisher_dev.hpp)
// ------------------------------------------------------------------------------------------
// The generic form takes four host arrays of table entries, the enrichment form query sets and a universe.  Both go through
// the cell kernel in CHUNKS of at most IGD_FISHER_CHUNK cells (48 bytes of device memory per cell: 48 MiB), one launch per
// chunk on the engine's stream, results copied straight into the caller's arrays at their place.  The workspace is the
// handle's (d_fisher), grown when a call needs more.
// The enrichment form is ONE igd_hip_support_sets call over nsets + 1 sets -- the caller's and, last, the universe, so the
// universe is counted once however many sets there are -- into rows of its own, which are copied to the caller's support /
// usupport (DEFINED, not added to); then the cell kernel reads the support rows chunk by chunk with usupport[] and n_k[]
// resident and forms b, c, d and the clamp flag itself.
#define IGD_FISHER_CHUNK ((int64_t)1 << 20)
#define IGD_FISHER_MAX_N ((int64_t)1 << 31)              // a table's N stays below this

// workgroups (of IGD_SETS_WG / IGD_WAVE waves) igd_fisher_cells is launched with for ncell cells: a wave takes a second cell
// only when ncell exceeds the grid's waves
extern "C" int32_t igd_hip_fisher_grid(int64_t ncell) { return items_grid(ncell, IGD_SETS_WG / IGD_WAVE); }

extern "C" int igd_hip_fisher_tables(igd_hip_db *db, const int64_t *a, const int64_t *b, const int64_t *c, const int64_t *d,
                                     int64_t ncell, double *pvalue_log, double *odds_ratio)
{
    if (!db || ncell < 0 || (ncell > 0 && (!a || !b || !c || !d || !pvalue_log))) {
        snprintf(g_err, sizeof g_err, "igd_hip_fisher_tables: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    for (int64_t i = 0; i < ncell; i++) {
        const bool neg = a[i] < 0 || b[i] < 0 || c[i] < 0 || d[i] < 0;
        const bool big = a[i] >= IGD_FISHER_MAX_N || b[i] >= IGD_FISHER_MAX_N || c[i] >= IGD_FISHER_MAX_N || d[i] >= IGD_FISHER_MAX_N;
        if (neg || big || a[i] + b[i] + c[i] + d[i] >= IGD_FISHER_MAX_N) {
            snprintf(g_err, sizeof g_err, "igd_hip_fisher_tables: table %lld (%lld %lld %lld %lld) has %s", (long long)i, (long long)a[i],
                     (long long)b[i], (long long)c[i], (long long)d[i], neg ? "a negative entry" : "N >= 2^31");
            return IGD_HIP_ERR_ARG;
        }
    }
    if (ncell == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    const int64_t step = ncell < IGD_FISHER_CHUNK ? ncell : IGD_FISHER_CHUNK;
    int rc = dev_grow(db, &db->d_fisher, &db->fisherCap, 6 * step);
    if (rc != IGD_HIP_OK) return rc;
    int64_t *dA = db->d_fisher, *dB = dA + step, *dC = dB + step, *dD = dC + step;
    double *dP = (double *)(dD + step), *dO = dP + step;
    for (int64_t c0 = 0; c0 < ncell; c0 += step) {
        const int64_t m = ncell - c0 < step ? ncell - c0 : step;
        HIPCHK(hipMemcpyAsync(dA, a + c0, (size_t)m * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dB, b + c0, (size_t)m * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dC, c + c0, (size_t)m * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dD, d + c0, (size_t)m * 8, hipMemcpyHostToDevice, st));
        igd_fisher_cells<false><<<igd_hip_fisher_grid(m), IGD_SETS_WG, 0, st>>>(dA, dB, dC, dD, 0, 1, c0, m, dP, odds_ratio ? dO : nullptr, nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(pvalue_log + c0, dP, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        if (odds_ratio) HIPCHK(hipMemcpyAsync(odds_ratio + c0, dO, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}

// igd_fisher_cells<true> over nsets x ncols cells (ncols = nFiles for the dataset tables, the number of groups for
// igd_hip_group_enrich_sets): rows = the sets' support (host), usupport[ncols], nk[nsets] = the sets' sizes, nu = the
// universe's; b, c, d and the clamp flag are formed on the device.  pvalue_log / odds_ratio (may be NULL) [nsets x ncols] and
// clamped[nsets] (may be NULL) are the host's.
static int fisher_enrich_cells(igd_hip_db *db, int64_t ncols, const int64_t *rows, const int64_t *usupport, const int64_t *nk, int32_t nsets,
                               int64_t nu, double *pvalue_log, double *odds_ratio, int64_t *clamped)
{
    const int64_t nF = ncols, ncell = (int64_t)nsets * nF;
    if (ncell == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    const int64_t step = ncell < IGD_FISHER_CHUNK ? ncell : IGD_FISHER_CHUNK;
    int rc = dev_grow(db, &db->d_fisher, &db->fisherCap, 3 * step + nF + 2 * (int64_t)nsets);
    if (rc != IGD_HIP_OK) return rc;
    int64_t *dA = db->d_fisher, *dU = dA + step, *dN = dU + nF;
    u64 *dCl = (u64 *)(dN + nsets);
    double *dP = (double *)(dCl + nsets), *dO = dP + step;
    HIPCHK(hipMemcpyAsync(dU, usupport, (size_t)nF * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dN, nk, (size_t)nsets * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dCl, 0, (size_t)nsets * 8, st));
    for (int64_t c0 = 0; c0 < ncell; c0 += step) {
        const int64_t m = ncell - c0 < step ? ncell - c0 : step;
        HIPCHK(hipMemcpyAsync(dA, rows + c0, (size_t)m * 8, hipMemcpyHostToDevice, st));
        igd_fisher_cells<true><<<igd_hip_fisher_grid(m), IGD_SETS_WG, 0, st>>>(dA, dU, dN, nullptr, nu, nF, c0, m, dP, odds_ratio ? dO : nullptr, dCl);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(pvalue_log + c0, dP, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        if (odds_ratio) HIPCHK(hipMemcpyAsync(odds_ratio + c0, dO, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
    }
    if (clamped) {
        HIPCHK(hipMemcpyAsync(clamped, dCl, (size_t)nsets * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return IGD_HIP_OK;
}

// igd_hip_enrich_sets and, for a caller that also prints them (the command line tool), the regions with any hit: nhit[nsets]
// and *unhit, DEFINED like the rest (both may be NULL)
// min_overlap: the sets' and the universe's supports are both taken under it (igd_hip_support_sets_ov); NULL: no threshold
extern "C" int igd_hip_enrich_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                      int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int32_t v,
                                      int rule, int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio,
                                      int64_t *clamped, int64_t *nhit, int64_t *unhit, const igd_hip_min_overlap *min_overlap)
{
    if (!igd_hip_min_overlap_valid(min_overlap)) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_sets: min_overlap (%d bp, %d ppm, %d ppm) out of range", (int)min_overlap->min_bp,
                 (int)min_overlap->ppm_query, (int)min_overlap->ppm_record);
        return IGD_HIP_ERR_ARG;
    }
    if (!db || nsets < 0 || nsets == INT32_MAX || nu < 0 || (nu > 0 && (!u_ichr || !u_qs || !u_qe)) || (db->nFiles > 0 && !usupport) ||
        (nsets > 0 && (!set_off || (db->nFiles > 0 && (!support || !pvalue_log)))) ||
        (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    // (the checks of igd_hip_support_sets, made here so that nothing of the caller's is written before them)
    int rc = sets_check("igd_hip_enrich_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nq = nsets > 0 ? set_off[nsets] : 0;
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] - set_off[k] + nu >= IGD_FISHER_MAX_N) {      // N <= n_k + n_U whatever is clamped
            snprintf(g_err, sizeof g_err, "igd_hip_enrich_sets: set %d and the universe hold 2^31 regions or more", (int)k);
            return IGD_HIP_ERR_ARG;
        }
    const int64_t nF = db->nFiles, ncell = (int64_t)nsets * nF;

    // one support call: the caller's sets, then the universe
    std::vector<int64_t> rows((size_t)((int64_t)(nsets + 1) * nF) + 1, 0), hit((size_t)nsets + 1, 0), nk((size_t)nsets + 1, 0);
    {
        const int64_t tot = nq + nu;
        std::vector<int32_t> cc((size_t)tot + 1), cs((size_t)tot + 1), ce((size_t)tot + 1);
        std::vector<int64_t> off((size_t)nsets + 2);
        if (nq) {
            memcpy(cc.data(), ichr, (size_t)nq * 4); memcpy(cs.data(), qs, (size_t)nq * 4); memcpy(ce.data(), qe, (size_t)nq * 4);
        }
        if (nu) {
            memcpy(cc.data() + nq, u_ichr, (size_t)nu * 4); memcpy(cs.data() + nq, u_qs, (size_t)nu * 4);
            memcpy(ce.data() + nq, u_qe, (size_t)nu * 4);
        }
        off[0] = 0;
        for (int32_t k = 0; k < nsets; k++) { off[(size_t)k + 1] = set_off[k + 1]; nk[(size_t)k] = set_off[k + 1] - set_off[k]; }
        off[(size_t)nsets + 1] = tot;
        rc = igd_hip_support_sets_ov(db, cc.data(), cs.data(), ce.data(), off.data(), nsets + 1, v, rule, rows.data(), hit.data(), min_overlap);
        if (rc != IGD_HIP_OK) return rc;
    }
    if (nF) memcpy(usupport, rows.data() + (size_t)ncell, (size_t)nF * 8);
    if (ncell) memcpy(support, rows.data(), (size_t)ncell * 8);
    if (nhit && nsets) memcpy(nhit, hit.data(), (size_t)nsets * 8);
    if (unhit) *unhit = hit[(size_t)nsets];
    if (clamped && nsets) memset(clamped, 0, (size_t)nsets * 8);
    return fisher_enrich_cells(db, nF, rows.data(), usupport, nk.data(), nsets, nu, pvalue_log, odds_ratio, clamped);
}

extern "C" int igd_hip_enrich_sets_nhit(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                        int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int32_t v,
                                        int rule, int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio,
                                        int64_t *clamped, int64_t *nhit, int64_t *unhit)
{
    return igd_hip_enrich_sets_ov(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, v, rule, support, usupport, pvalue_log, odds_ratio,
                                  clamped, nhit, unhit, nullptr);
}

extern "C" int igd_hip_enrich_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                   int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int32_t v,
                                   int rule, int64_t *support, int64_t *usupport, double *pvalue_log, double *odds_ratio, int64_t *clamped)
{
    return igd_hip_enrich_sets_nhit(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, v, rule, support, usupport, pvalue_log,
                                    odds_ratio, clamped, nullptr, nullptr);
}
