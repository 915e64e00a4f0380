// engine/host_restrict.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_restrict_sets / igd_hip_enrich_restricted: query sets restricted to the universe (restrict_dev.hpp)
// ------------------------------------------------------------------------------------------
// The join.  The host orders the universe regions with ichr >= 0 by (ichr, start) -- the sort is skipped when they come that
// way --, builds per contig the prefix maximum of the ends and uploads them with the permutation back to the caller's order
// and the contig range table.  The sets go through igd_restrict_bits in CHUNKS of whole sets whose rows (nUW words each) stay
// within restrict_row_bytes() (sets_row_bytes()) and, in the enrichment form, whose support rows do too; inside a chunk the
// regions are uploaded in batches of at most igd_hip_max_batch() (a set may be cut between two batches: its row is an OR).
// The rows are zeroed on the stream before the first batch; igd_member_popc behind the last one gives |R_k|.
// The enrichment.  The join of all chunks first (rows to the host, or left on the device when one chunk holds all sets); then
// the universe, in the caller's order, through igd_hip_membership_dev in chunks of at most igd_hip_max_batch() regions and
// member_row_bytes() of rows; per (universe chunk, set chunk) one launch of igd_bits_support into zeroed rows, which are added
// to the host's sums.  The first set chunk carries one row more, the ones row: the universe's own support and hit count.
// The membership rows never leave the device.  Then igd_fisher_cells<true> with n_k := |R_k| as in igd_hip_enrich_sets.
// Everything is computed into buffers of this file and copied to the caller's at the end: on an error nothing is written.
static_assert((unsigned long long)IGD_RESTRICT_BLOCK_WORDS * 32ull <= 0xffffffffull, "an item must fit the 32-bit LDS counters of igd_bits_support");

// The TEST-ONLY variable IGD_HIP_RESTRICT_ROW_BYTES (read once per process, as IGD_HIP_MEMBER_ROW_BYTES) lowers the budget of
// a set chunk so that small fixtures cross the seam between two chunks.
static int64_t restrict_row_bytes(void)
{
    static const int64_t m = env_positive("IGD_HIP_RESTRICT_ROW_BYTES", sets_row_bytes());
    return m;
}

// workgroups igd_restrict_bits is launched with for nregions set regions: a lane takes a second region only when nregions
// exceeds the grid's lanes
extern "C" int32_t igd_hip_restrict_grid(int64_t nregions) { return items_grid(nregions, IGD_SETS_WG); }

// the checks of igd_hip_enrich_sets that both entry points share
static int restrict_check(const char *who, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                          const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu)
{
    if (nsets == INT32_MAX || nu < 0 || (nu > 0 && (!u_ichr || !u_qs || !u_qe))) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return IGD_HIP_ERR_ARG;
    }
    const int rc = sets_check(who, ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    if (nu + 1 >= IGD_FISHER_MAX_N) {
        snprintf(g_err, sizeof g_err, "%s: the universe holds 2^31 - 1 regions or more", who);
        return IGD_HIP_ERR_ARG;
    }
    return IGD_HIP_OK;
}

// sets per chunk: rows of nUW words, and (enrichment form) support rows of nF counters, within the budget
static int64_t restrict_row_cap(int64_t nUW, int64_t nF)
{
    const int64_t per = nUW * 4 > nF * 8 ? nUW * 4 : nF * 8;
    const int64_t cap = per > 0 ? restrict_row_bytes() / per : (int64_t)1 << 20;
    return cap < 1 ? 1 : cap > ((int64_t)1 << 20) ? (int64_t)1 << 20 : cap;
}

// The join of all sets.  bits (host, nsets x nUW words) and size (host, int64[nsets]) are written chunk by chunk.
// The last chunk's rows stay in db->d_rsBits.  rowCap = sets per chunk.
static int restrict_join(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                         const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu, int64_t rowCap,
                         uint32_t *bits, int64_t *size)
{
    const int64_t nUW = (nu + 31) / 32;
    if (nsets == 0) return IGD_HIP_OK;
    if (nu == 0) {
        memset(size, 0, (size_t)nsets * 8);
        return IGD_HIP_OK;
    }
    // the universe regions with a contig, by (ichr, start); ties in the caller's order
    std::vector<int32_t> ord;
    ord.reserve((size_t)nu);
    bool sorted = true;
    for (int64_t u = 0; u < nu; u++) {
        if (u_ichr[u] < 0) continue;
        if (!ord.empty()) {
            const int32_t p = ord.back();
            if (u_ichr[p] > u_ichr[u] || (u_ichr[p] == u_ichr[u] && u_qs[p] > u_qs[u])) sorted = false;
        }
        ord.push_back((int32_t)u);
    }
    if (!sorted)
        std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
            if (u_ichr[a] != u_ichr[b]) return u_ichr[a] < u_ichr[b];
            if (u_qs[a] != u_qs[b]) return u_qs[a] < u_qs[b];
            return a < b;
        });
    const int64_t nv = (int64_t)ord.size();
    std::vector<int32_t> uni((size_t)(4 * nv) + 1);
    int32_t *hs = uni.data(), *he = hs + nv, *hm = he + nv, *hp = hm + nv;
    std::vector<int32_t> cval, cbeg;
    for (int64_t p = 0; p < nv; p++) {
        const int32_t u = ord[(size_t)p];
        const bool first = p == 0 || u_ichr[ord[(size_t)p - 1]] != u_ichr[u];
        if (first) { cval.push_back(u_ichr[u]); cbeg.push_back((int32_t)p); }
        hs[p] = u_qs[u]; he[p] = u_qe[u]; hp[p] = u;
        hm[p] = first || u_qe[u] > hm[p - 1] ? u_qe[u] : hm[p - 1];
    }
    cbeg.push_back((int32_t)nv);
    const int nc = (int)cval.size();

    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    int rc = dev_grow(db, &db->d_rsUni, &db->rsUniCap, 4 * nv + 1);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_rsTab, &db->rsTabCap, (int64_t)(2 * nc + 1) + (nsets < rowCap ? nsets : rowCap) + 1);
    if (rc != IGD_HIP_OK) return rc;
    int32_t *dS = db->d_rsUni, *dE = dS + nv, *dM = dE + nv, *dP = dM + nv;
    int32_t *dCv = db->d_rsTab, *dCb = dCv + nc, *dOff = dCb + nc + 1;
    if (nv) HIPCHK(hipMemcpyAsync(dS, hs, (size_t)(4 * nv) * 4, hipMemcpyHostToDevice, st));
    if (nc) HIPCHK(hipMemcpyAsync(dCv, cval.data(), (size_t)nc * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dCb, cbeg.data(), (size_t)(nc + 1) * 4, hipMemcpyHostToDevice, st));

    const int64_t step = max_batch();
    std::vector<int32_t> hoff, hsize;
    for (int32_t k0 = 0; k0 < nsets; k0 += (int32_t)rowCap) {
        const int32_t rows = (int32_t)(nsets - k0 < rowCap ? nsets - k0 : rowCap);
        rc = dev_grow(db, &db->d_rsBits, &db->rsBitsCap, (int64_t)rows * nUW);
        if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_rsSize, &db->rsSizeCap, (int64_t)rows);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemsetAsync(db->d_rsBits, 0, (size_t)((int64_t)rows * nUW) * 4, st));
        hoff.resize((size_t)rows + 1);
        for (int64_t c0 = set_off[k0]; c0 < set_off[k0 + rows] && nv > 0; c0 += step) {
            const int64_t m = set_off[k0 + rows] - c0 < step ? set_off[k0 + rows] - c0 : step;
            for (int32_t k = 0; k <= rows; k++) {        // the sets' first regions, numbered within this batch
                const int64_t o = set_off[k0 + k] - c0;
                hoff[(size_t)k] = (int32_t)(o < 0 ? 0 : o > m ? m : o);
            }
            if ((rc = stage_queries(db, ichr, qs, qe, c0, m)) != IGD_HIP_OK) return rc;
            HIPCHK(hipMemcpyAsync(dOff, hoff.data(), (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, st));
            igd_restrict_bits<<<igd_hip_restrict_grid(m), IGD_SETS_WG, 0, st>>>(db->d_qc, db->d_qs, db->d_qe, (int)m, dOff, rows, dCv, dCb, nc,
                                                                                 dS, dE, dM, dP, nUW, db->d_rsBits);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));            // (hoff and the staging buffers are written again by the next batch)
        }
        igd_member_popc<<<igd_hip_member_grid(rows), IGD_SETS_WG, 0, st>>>(db->d_rsBits, rows, (int)nUW, db->d_rsSize);
        HIPCHK(hipGetLastError());
        hsize.resize((size_t)rows);
        HIPCHK(hipMemcpyAsync(hsize.data(), db->d_rsSize, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(bits + (size_t)k0 * (size_t)nUW, db->d_rsBits, (size_t)((int64_t)rows * nUW) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        for (int32_t k = 0; k < rows; k++) size[k0 + k] = hsize[(size_t)k];
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_restrict_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                     int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                                     uint32_t *bits, int64_t *size)
{
    if (!db) {
        snprintf(g_err, sizeof g_err, "igd_hip_restrict_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    int rc = restrict_check("igd_hip_restrict_sets", ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nUW = (nu + 31) / 32;
    if (nsets > 0 && (!size || (nUW > 0 && !bits))) {
        snprintf(g_err, sizeof g_err, "igd_hip_restrict_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    std::vector<uint32_t> hb((size_t)((int64_t)nsets * nUW) + 1);
    std::vector<int64_t> hz((size_t)nsets + 1);
    rc = restrict_join(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, restrict_row_cap(nUW, 0), hb.data(), hz.data());
    if (rc != IGD_HIP_OK) return rc;
    if (nsets && nUW) memcpy(bits, hb.data(), (size_t)((int64_t)nsets * nUW) * 4);
    if (nsets) memcpy(size, hz.data(), (size_t)nsets * 8);
    return IGD_HIP_OK;
}

extern "C" int igd_hip_enrich_restricted(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                         int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                                         int32_t v, int rule, int64_t *support, int64_t *usupport, int64_t *size, double *pvalue_log,
                                         double *odds_ratio, uint32_t *bits, int64_t *nhit, int64_t *unhit)
{
    if (!db || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) || (db->nFiles > 0 && !usupport) ||
        (nsets > 0 && (!size || (db->nFiles > 0 && (!support || !pvalue_log))))) {
        snprintf(g_err, sizeof g_err, "igd_hip_enrich_restricted: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    int rc = restrict_check("igd_hip_enrich_restricted", ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32, nUW = (nu + 31) / 32, ncell = (int64_t)nsets * nF;
    const int64_t rowCap = restrict_row_cap(nUW, nF);
    const bool one = (int64_t)nsets <= rowCap;           // all sets in one chunk: its rows stay on the device

    std::vector<uint32_t> hb((size_t)((int64_t)nsets * nUW) + 1);
    std::vector<int64_t> hz((size_t)nsets + 1, 0), rows((size_t)ncell + 1, 0), urow((size_t)nF + 1, 0), hit((size_t)nsets + 1, 0);
    int64_t uhit = 0;
    rc = restrict_join(db, ichr, qs, qe, set_off, nsets, u_ichr, u_qs, u_qe, nu, rowCap, hb.data(), hz.data());
    if (rc != IGD_HIP_OK) return rc;

    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    if (nu > 0 && nF > 0) {
        const bool lds = nF <= IGD_RESTRICT_LDS_FILES;
        const size_t ldsB = (size_t)(4 + (lds ? nF : 0)) * 4;
        const int64_t byRows = member_row_bytes() / (nW * 4);
        int64_t ustep = max_batch();
        if (byRows < ustep) ustep = byRows < 1 ? 1 : byRows;
        std::vector<int64_t> hrows, htot;
        for (int64_t u0 = 0; u0 < nu; u0 += ustep) {
            const int64_t um = nu - u0 < ustep ? nu - u0 : ustep, u1 = u0 + um;
            rc = ensure_member_ws(db, um * nW, um);
            if (rc == IGD_HIP_OK) rc = stage_queries(db, u_ichr, u_qs, u_qe, u0, um);
            if (rc != IGD_HIP_OK) return rc;
            rc = igd_hip_membership_dev(db, db->d_qc, db->d_qs, db->d_qe, um, v, rule, db->d_memBits, db->d_memNf, nullptr, st);
            if (rc != IGD_HIP_OK) return rc;
            const int64_t w0 = u0 >> 5, w1 = (u1 + 31) >> 5, nblk = (w1 - w0 + IGD_RESTRICT_BLOCK_WORDS - 1) / IGD_RESTRICT_BLOCK_WORDS;
            for (int32_t k0 = 0; k0 == 0 || k0 < nsets; k0 += (int32_t)rowCap) {
                const int32_t srows = (int32_t)(nsets - k0 < rowCap ? nsets - k0 : rowCap);
                const int32_t r = srows + (k0 == 0 ? 1 : 0);             // the first chunk carries the ones row
                const int ones = k0 == 0 ? srows : -1;
                if (srows > 0 && !one) {
                    rc = dev_grow(db, &db->d_rsBits, &db->rsBitsCap, (int64_t)srows * nUW);
                    if (rc != IGD_HIP_OK) return rc;
                    HIPCHK(hipMemcpyAsync(db->d_rsBits, hb.data() + (size_t)k0 * (size_t)nUW, (size_t)((int64_t)srows * nUW) * 4,
                                          hipMemcpyHostToDevice, st));
                }
                rc = sets_ws(db, (int64_t)r * nF, r, 0);
                if (rc != IGD_HIP_OK) return rc;
                HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)((int64_t)r * nF) * 8, st));
                HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)r * 8, st));
                const int64_t items = (int64_t)r * nblk;
                const int grid = (int)(items < IGD_SETS_GRID ? items : IGD_SETS_GRID);
                u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
                if (lds) igd_bits_support<true><<<grid, IGD_SETS_WG, ldsB, st>>>(db->d_rsBits, nUW, r, ones, u0, u1, db->d_memBits, db->d_memNf, (int)nF, R, T);
                else igd_bits_support<false><<<grid, IGD_SETS_WG, ldsB, st>>>(db->d_rsBits, nUW, r, ones, u0, u1, db->d_memBits, db->d_memNf, (int)nF, R, T);
                HIPCHK(hipGetLastError());
                hrows.resize((size_t)((int64_t)r * nF));
                htot.resize((size_t)r);
                HIPCHK(hipMemcpyAsync(hrows.data(), db->d_setRows, (size_t)((int64_t)r * nF) * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(htot.data(), db->d_setTot, (size_t)r * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                HIPCHK(hipGetLastError());
                for (int32_t k = 0; k < srows; k++) {
                    int64_t *dst = rows.data() + (size_t)(k0 + k) * (size_t)nF;
                    const int64_t *src = hrows.data() + (size_t)k * (size_t)nF;
                    for (int64_t f = 0; f < nF; f++) dst[f] += src[f];
                    hit[(size_t)(k0 + k)] += htot[(size_t)k];
                }
                if (k0 == 0) {
                    const int64_t *src = hrows.data() + (size_t)srows * (size_t)nF;
                    for (int64_t f = 0; f < nF; f++) urow[(size_t)f] += src[f];
                    uhit += htot[(size_t)srows];
                }
            }
        }
    }

    // the statistics: igd_fisher_cells<true> on the restricted supports, n_k := |R_k| (nothing can be clamped)
    std::vector<double> hp((size_t)ncell + 1), ho((size_t)ncell + 1);
    rc = fisher_enrich_cells(db, db->nFiles, rows.data(), urow.data(), hz.data(), nsets, nu, hp.data(), odds_ratio ? ho.data() : nullptr, nullptr);
    if (rc != IGD_HIP_OK) return rc;

    if (nF) memcpy(usupport, urow.data(), (size_t)nF * 8);
    if (ncell) {
        memcpy(support, rows.data(), (size_t)ncell * 8);
        memcpy(pvalue_log, hp.data(), (size_t)ncell * 8);
        if (odds_ratio) memcpy(odds_ratio, ho.data(), (size_t)ncell * 8);
    }
    if (nsets) memcpy(size, hz.data(), (size_t)nsets * 8);
    if (bits && nsets && nUW) memcpy(bits, hb.data(), (size_t)((int64_t)nsets * nUW) * 4);
    if (nhit && nsets) memcpy(nhit, hit.data(), (size_t)nsets * 8);
    if (unhit) *unhit = uhit;
    return IGD_HIP_OK;
}
