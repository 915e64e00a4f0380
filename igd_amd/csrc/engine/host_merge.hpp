// engine/host_merge.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_merge_sets / igd_hip_merge_sets_dev / igd_hip_dataset_bp / igd_hip_jaccard_sets: region sets merged on the device, the
// merged base pairs of every dataset, and the base-pair intersection of every set with every dataset (merge_dev.hpp; the
// definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// The device form is a fixed sequence of launches on the caller's stream, with no wait and no copy to the host: set numbers
// and the first key; stable radix passes by qe, qs, ichr and the set number (32, 32, bits(nCtg - 1) and bits(nsets) bits), the
// next key gathered through the permutation between them; the sorted regions; the three launches of the segmented maximum
// scan; the exclusive sum of the run flags (exclusive_scan); run heads, runs, offsets.  Its arrays are ONE workspace of the
// handle that only grows (d_merge: about 62 bytes per region in the device form, about 90 in the host form, which keeps the
// caller's three arrays and the four result arrays behind it).  The workspace is the handle's: calls on ONE handle must be ordered
// with respect to each other (one stream, or events between streams); dev_grow waits for the engine's stream only.  The host form puts the caller's arrays behind that workspace,
// runs the device form on the engine's stream and copies the runs back.
//
// igd_hip_dataset_bp is igd_hip_coverage_sets over one set: every tile of every contig as one query.  The result is kept in
// the handle per (v, rule) -- a gType-0 database has no value field, so there every v is one entry -- and bpComputed counts the
// times it was computed and not found (igd_hip_dataset_bp_computed).
//
// igd_hip_jaccard_sets merges through the host form and hands the runs to igd_hip_coverage_sets as they are: run_set_chunks
// stages host arrays, and a second entrance for resident ones would have to cut a resident array at chunk seams the host
// decides from set_off, which it does not have before the merge's counts are back.  So the runs make one round trip; they
// are 12 bytes per run, read back once, against the slab rows the coverage stage copies per chunk anyway.
#define IGD_MERGE_MAX_REGIONS ((int64_t)1 << 30)
#define IGD_MERGE_GRID 4096

struct MergeWs {
    uint32_t *setOf, *kA, *vA, *kB, *vB, *sSet, *flag, *hist;
    int32_t *sChr, *sQs, *sQe, *inc, *exc, *runStart;
    int64_t *pos, *dig, *sums, *tot;
    MergeAgg *tiles;
    // host form only: the caller's arrays and results
    int32_t *in[3], *out[4];
    int64_t *setOff, *mOff, *dropped;
    int64_t bytes;
};

// carves `base` (may be null: sizes only) into the arrays of a merge of n regions in nsets sets
static MergeWs merge_layout(char *base, int64_t n, int32_t nsets, bool hostForm)
{
    MergeWs w;
    int64_t at = 0;
    auto take = [&](auto **p, int64_t count) {
        *p = (typename std::remove_reference<decltype(**p)>::type *)(base + at);
        at += (count * (int64_t)sizeof(**p) + 255) & ~(int64_t)255;
    };
    const int64_t nh = rs_blocks(n) * 256, nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    const int64_t nsum = ((nh > n ? nh : n) + SCAN_TILE - 1) / SCAN_TILE + 1;
    take(&w.setOf, n); take(&w.kA, n); take(&w.vA, n); take(&w.kB, n); take(&w.vB, n); take(&w.sSet, n); take(&w.flag, n);
    take(&w.hist, nh); take(&w.sChr, n); take(&w.sQs, n); take(&w.sQe, n); take(&w.inc, n); take(&w.exc, n); take(&w.runStart, n);
    take(&w.pos, n); take(&w.dig, nh); take(&w.sums, nsum); take(&w.tot, 1); take(&w.tiles, nb);
    if (hostForm) {
        for (int k = 0; k < 3; k++) take(&w.in[k], n);
        for (int k = 0; k < 4; k++) take(&w.out[k], n);
        take(&w.setOff, (int64_t)nsets + 1); take(&w.mOff, (int64_t)nsets + 1); take(&w.dropped, (int64_t)nsets);
    }
    w.bytes = at;
    return w;
}

static int merge_gap_bad(const char *who, int64_t gap)
{
    if (igd_hip_merge_gap_valid(gap)) return 0;
    snprintf(g_err, sizeof g_err, "%s: gap %lld outside 0 .. 2^30", who, (long long)gap);
    return 1;
}

// the launches (arguments checked, n > 0, nsets > 0, the workspace carved)
static int merge_launches(igd_hip_db *db, const MergeWs &w, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe,
                          const int64_t *d_set_off, int32_t nsets, int64_t n, int64_t gap, int32_t *m_ichr, int32_t *m_qs, int32_t *m_qe,
                          int64_t *m_off, int32_t *m_count, int64_t *n_dropped, hipStream_t st)
{
    // (TEST-ONLY: IGD_HIP_MERGE_GRID, read once per process, lowers the grid so that small fixtures give a workgroup a second round)
    static const int64_t maxGrid = env_positive("IGD_HIP_MERGE_GRID", IGD_MERGE_GRID);
    // (TEST-ONLY: IGD_HIP_MERGE_CARRY_WG, read once per process, lowers the threads of the carry workgroup -- whole waves, 64 ..
    // IGD_MERGE_CARRY_WG -- so that a few hundred tiles take it through several rounds)
    static const unsigned carryWg = []() {
        const int64_t t = env_positive("IGD_HIP_MERGE_CARRY_WG", IGD_MERGE_CARRY_WG) / WAVE * WAVE;
        return (unsigned)(t < WAVE ? WAVE : t > IGD_MERGE_CARRY_WG ? IGD_MERGE_CARRY_WG : t);
    }();
    auto grid = [](int64_t items) { const int64_t g = (items + IGD_MERGE_WG - 1) / IGD_MERGE_WG; return (unsigned)(g < maxGrid ? g : maxGrid); };
    auto bits_of = [](uint64_t top) { int b = 0; while (b < 32 && (top >> b)) b++; return b; };
    const unsigned g = grid(n);
    uint32_t *kA = w.kA, *vA = w.vA, *kB = w.kB, *vB = w.vB;
    igd_merge_sets_of<<<g, IGD_MERGE_WG, 0, st>>>(d_ichr, d_qs, d_qe, d_set_off, nsets, db->nCtg, n, w.setOf, kA, vA);
    HIPCHK(radix_sort_pairs(&kA, &vA, &kB, &vB, n, 32, w.hist, w.dig, w.sums, w.tot, st));
    const int keyBits[3] = {32, bits_of(db->nCtg > 0 ? (uint64_t)db->nCtg - 1 : 0), bits_of((uint64_t)nsets)};
    for (int which = 0; which < 3; which++) {
        if (keyBits[which] == 0) continue;               // (one contig: nothing to order by)
        igd_merge_key<<<g, IGD_MERGE_WG, 0, st>>>(d_ichr, d_qs, w.setOf, nsets, vA, n, which, kA);
        HIPCHK(radix_sort_pairs(&kA, &vA, &kB, &vB, n, keyBits[which], w.hist, w.dig, w.sums, w.tot, st));
    }
    igd_merge_gather<<<g, IGD_MERGE_WG, 0, st>>>(d_ichr, d_qs, d_qe, w.setOf, vA, n, w.sSet, w.sChr, w.sQs, w.sQe);
    const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    igd_merge_scan_tiles<<<(unsigned)nb, SCAN_WG, 0, st>>>(w.sSet, w.sChr, w.sQe, n, w.tiles);
    igd_merge_scan_carry<<<1, carryWg, 0, st>>>(w.tiles, nb);
    igd_merge_scan_apply<<<(unsigned)nb, SCAN_WG, 0, st>>>(w.sSet, w.sChr, w.sQs, w.sQe, n, (uint32_t)nsets, gap, w.tiles, w.inc, w.exc, w.flag);
    HIPCHK(hipGetLastError());
    HIPCHK((exclusive_scan<uint32_t, int64_t>(w.flag, n, w.pos, w.sums, w.tot, st)));
    igd_merge_heads<<<g, IGD_MERGE_WG, 0, st>>>(w.flag, w.pos, n, w.runStart);
    igd_merge_runs<<<g, IGD_MERGE_WG, 0, st>>>(w.sSet, w.sChr, w.sQs, w.inc, w.runStart, w.tot, n, (uint32_t)nsets, m_ichr, m_qs, m_qe, m_count);
    igd_merge_offsets<<<grid((int64_t)nsets + 1), IGD_MERGE_WG, 0, st>>>(w.sSet, w.pos, w.tot, n, d_set_off, nsets, m_off, n_dropped);
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

static int merge_ws(igd_hip_db *db, int64_t n, int32_t nsets, bool hostForm, MergeWs *w)
{
    const int rc = dev_grow(db, &db->d_merge, &db->mergeCap, merge_layout(nullptr, n, nsets, hostForm).bytes);
    if (rc == IGD_HIP_OK) *w = merge_layout(db->d_merge, n, nsets, hostForm);
    return rc;
}

extern "C" int igd_hip_merge_sets_dev(igd_hip_db *db, const int32_t *d_ichr, const int32_t *d_qs, const int32_t *d_qe, const int64_t *d_set_off,
                                      int32_t nsets, int64_t n, int64_t gap, int32_t *d_m_ichr, int32_t *d_m_qs, int32_t *d_m_qe,
                                      int64_t *d_m_off, int32_t *d_m_count, int64_t *d_n_dropped, void *stream)
{
    if (merge_gap_bad("igd_hip_merge_sets_dev", gap)) return IGD_HIP_ERR_ARG;
    if (!db || nsets < 0 || n < 0 || n > IGD_MERGE_MAX_REGIONS || (nsets == 0 && n > 0) ||
        (nsets > 0 && (!d_set_off || !d_m_off || !d_n_dropped)) || (n > 0 && (!d_ichr || !d_qs || !d_qe || !d_m_ichr || !d_m_qs || !d_m_qe))) {
        snprintf(g_err, sizeof g_err, "igd_hip_merge_sets_dev: bad argument (at most 2^30 regions)");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = stream ? (hipStream_t)stream : db->stream;
    if (n == 0) {                                        // only empty sets
        HIPCHK(hipMemsetAsync(d_m_off, 0, ((size_t)nsets + 1) * 8, st));
        HIPCHK(hipMemsetAsync(d_n_dropped, 0, (size_t)nsets * 8, st));
        return IGD_HIP_OK;
    }
    MergeWs w;
    const int rc = merge_ws(db, n, nsets, false, &w);
    if (rc != IGD_HIP_OK) return rc;
    return merge_launches(db, w, d_ichr, d_qs, d_qe, d_set_off, nsets, n, gap, d_m_ichr, d_m_qs, d_m_qe, d_m_off, d_m_count, d_n_dropped, st);
}

extern "C" int igd_hip_merge_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                                  int64_t gap, int32_t *m_ichr, int32_t *m_qs, int32_t *m_qe, int64_t *m_off, int32_t *m_count, int64_t *n_dropped)
{
    if (merge_gap_bad("igd_hip_merge_sets", gap)) return IGD_HIP_ERR_ARG;
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !m_off || !n_dropped))) {
        snprintf(g_err, sizeof g_err, "igd_hip_merge_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_merge_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t n = set_off[nsets];
    if (n > IGD_MERGE_MAX_REGIONS || (n > 0 && (!m_ichr || !m_qs || !m_qe))) {
        snprintf(g_err, sizeof g_err, "igd_hip_merge_sets: bad argument (at most 2^30 regions)");
        return IGD_HIP_ERR_ARG;
    }
    if (n == 0) {
        for (int32_t k = 0; k <= nsets; k++) m_off[k] = 0;
        for (int32_t k = 0; k < nsets; k++) n_dropped[k] = 0;
        return IGD_HIP_OK;
    }
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    MergeWs w;
    if ((rc = merge_ws(db, n, nsets, true, &w)) != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(w.in[0], ichr, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.in[1], qs, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.in[2], qe, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w.setOff, set_off, ((size_t)nsets + 1) * 8, hipMemcpyHostToDevice, st));
    rc = merge_launches(db, w, w.in[0], w.in[1], w.in[2], w.setOff, nsets, n, gap, w.out[0], w.out[1], w.out[2], w.mOff, m_count ? w.out[3] : nullptr,
                        w.dropped, st);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(m_ichr, w.out[0], (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(m_qs, w.out[1], (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(m_qe, w.out[2], (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (m_count) HIPCHK(hipMemcpyAsync(m_count, w.out[3], (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(m_off, w.mOff, ((size_t)nsets + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(n_dropped, w.dropped, (size_t)nsets * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return IGD_HIP_OK;
}

// ---- merged base pairs per dataset ---------------------------------------------------------
extern "C" int64_t igd_hip_dataset_bp_computed(const igd_hip_db *db) { return db ? db->bpComputed : 0; }

extern "C" int igd_hip_dataset_bp(igd_hip_db *db, int32_t v, int rule, int64_t *file_bp)
{
    if (!db || !file_bp || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_dataset_bp: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    const int64_t nF = db->nFiles;
    const int32_t vkey = db->gType == 1 ? v : IGD_HIP_NO_VALUE_FILTER;       // (no value field: every v counts every record)
    for (const igd_hip_db::BpEntry &e : db->bpCache)
        if (e.v == vkey && e.rule == rule) {
            memcpy(file_bp, e.bp.data(), (size_t)(nF + 1) * 8);
            return IGD_HIP_OK;
        }
    // one query per tile of the file: [t nbp, (t + 1) nbp), the end capped at INT32_MAX
    std::vector<int32_t> c, s, e;
    for (int32_t ic = 0; ic < db->nCtg; ic++)
        for (int64_t t = 0; t < db->hNTile[(size_t)ic]; t++) {
            int32_t ws, we;
            if (!igd_hip_tile_query(db->nbp, t, &ws, &we)) break;
            c.push_back(ic); s.push_back(ws); e.push_back(we);
        }
    igd_hip_db::BpEntry ent;
    ent.v = vkey; ent.rule = rule;
    ent.bp.assign((size_t)nF + 1, 0);
    const int64_t off[2] = {0, (int64_t)c.size()};
    const int rc = igd_hip_coverage_sets(db, c.data(), s.data(), e.data(), off, 1, v, rule, ent.bp.data(), ent.bp.data() + nF);
    if (rc != IGD_HIP_OK) return rc;
    db->bpComputed++;
    memcpy(file_bp, ent.bp.data(), (size_t)(nF + 1) * 8);
    db->bpCache.push_back(std::move(ent));
    return IGD_HIP_OK;
}

// ---- the table -----------------------------------------------------------------------------
extern "C" int igd_hip_jaccard_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                                    int32_t v, int rule, int64_t *inter, int64_t *set_bp, int64_t *file_bp, int64_t *n_merged, int64_t *n_dropped)
{
    if (!db || nsets < 0 || !file_bp || (nsets > 0 && (!set_off || !inter || !set_bp || !n_merged || !n_dropped)) ||
        (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_jaccard_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    int rc = sets_check("igd_hip_jaccard_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    const int64_t nF = db->nFiles, n = nsets > 0 ? set_off[nsets] : 0;
    if (n > IGD_MERGE_MAX_REGIONS) {
        snprintf(g_err, sizeof g_err, "igd_hip_jaccard_sets: bad argument (at most 2^30 regions)");
        return IGD_HIP_ERR_ARG;
    }
    if ((rc = igd_hip_dataset_bp(db, v, rule, file_bp)) != IGD_HIP_OK) return rc;
    if (nsets == 0) return IGD_HIP_OK;
    std::vector<int32_t> mc((size_t)n), ms((size_t)n), me((size_t)n);
    std::vector<int64_t> moff((size_t)nsets + 1), cov((size_t)nsets * (size_t)nF, 0), any((size_t)nsets, 0);
    if ((rc = igd_hip_merge_sets(db, ichr, qs, qe, set_off, nsets, 0, mc.data(), ms.data(), me.data(), moff.data(), nullptr, n_dropped)) != IGD_HIP_OK)
        return rc;
    if ((rc = igd_hip_coverage_sets(db, mc.data(), ms.data(), me.data(), moff.data(), nsets, v, rule, cov.data(), any.data())) != IGD_HIP_OK) return rc;
    for (int32_t k = 0; k < nsets; k++) {
        int64_t bp = 0;
        for (int64_t r = moff[(size_t)k]; r < moff[(size_t)k + 1]; r++) bp += (int64_t)me[(size_t)r] - (int64_t)ms[(size_t)r];
        set_bp[k] = bp;
        n_merged[k] = moff[(size_t)k + 1] - moff[(size_t)k];
        for (int64_t f = 0; f < nF; f++) inter[(int64_t)k * (nF + 1) + f] = cov[(size_t)(k * nF + f)];
        inter[(int64_t)k * (nF + 1) + nF] = any[(size_t)k];
    }
    return IGD_HIP_OK;
}
