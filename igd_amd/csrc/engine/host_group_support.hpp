// engine/host_group_support.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_group_support_sets / igd_hip_group_enrich_sets: support and enrichment per GROUP of datasets
// ------------------------------------------------------------------------------------------
// The chunks are those of igd_hip_support_sets -- run_set_chunks (host_common.hpp) with rows of ngroups columns instead of nFiles
// -- and every set is cut into slices for igd_sets_group_support (group_support_dev.hpp): one launch per chunk.  The grouping
// (include/igd_hip.h: grp_off, grp_idx) is checked on the host before anything of the caller's is written, goes to the device
// once per call (d_gsTab: grp_off, then grp_idx) and stays there for all its chunks.  There is no wide form: more than
// IGD_HIP_GROUP_MAX groups is an argument error.
// The enrichment form mirrors igd_hip_enrich_sets_ov: ONE group-support call over nsets + 1 sets, the universe last and counted
// once, then fisher_enrich_cells over nsets x ngroups cells (b, c, d and the clamp flag formed on the device).
// igd_sets_group_support's LDS counters are 32 bits wide: a query adds at most 1 per group and a slice is flushed at its end
static_assert(IGD_SETS_SLICE_MAX <= IGD_GROUP_SLICE_CAP, "sets_slice_len() must not cut longer slices than igd_sets_group_support counts in 32 bits");
static_assert(IGD_GROUP_LDS_GROUPS == IGD_HIP_GROUP_MAX, "the kernel's LDS budget and the limit the header names are one number");

// the grouping as the header defines it, or IGD_HIP_ERR_ARG with the first bad entry named
static int groups_check(const char *who, int32_t nFiles, const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups)
{
    if (ngroups <= 0 || ngroups > IGD_HIP_GROUP_MAX) {
        snprintf(g_err, sizeof g_err, "%s: %d groups given, 1 .. %d are possible", who, (int)ngroups, (int)IGD_HIP_GROUP_MAX);
        return IGD_HIP_ERR_ARG;
    }
    if (!grp_off) {
        snprintf(g_err, sizeof g_err, "%s: bad argument (grp_off)", who);
        return IGD_HIP_ERR_ARG;
    }
    int64_t at = 0;
    const int bad = igd_hip_groups_first_bad(nFiles, grp_off, grp_idx, ngroups, &at);
    if (bad == IGD_HIP_GROUPS_BAD_OFF)
        snprintf(g_err, sizeof g_err, "%s: grp_off[%lld] = %d: the offsets start at 0 and do not decrease", who, (long long)at, (int)grp_off[at]);
    else if (bad == IGD_HIP_GROUPS_BAD_RANGE)
        snprintf(g_err, sizeof g_err, "%s: grp_idx[%lld] = %d is not in [0, %d)", who, (long long)at, (int)grp_idx[at], (int)ngroups);
    else if (bad == IGD_HIP_GROUPS_BAD_ORDER)
        snprintf(g_err, sizeof g_err, "%s: grp_idx[%lld] = %d does not ascend within its dataset's run", who, (long long)at, (int)grp_idx[at]);
    else if (bad)
        snprintf(g_err, sizeof g_err, "%s: bad argument (grp_idx)", who);
    return bad ? IGD_HIP_ERR_ARG : IGD_HIP_OK;
}

// grp_off[nFiles + 1] and grp_idx[grp_off[nFiles]] into d_gsTab, on the engine's stream
static int groups_upload(igd_hip_db *db, const int32_t *grp_off, const int32_t *grp_idx)
{
    const int64_t nOff = (int64_t)db->nFiles + 1, nIdx = grp_off[db->nFiles];
    const int rc = dev_grow(db, &db->d_gsTab, &db->gsTabCap, nOff + nIdx);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(db->d_gsTab, grp_off, (size_t)nOff * 4, hipMemcpyHostToDevice, db->stream));
    if (nIdx) HIPCHK(hipMemcpyAsync(db->d_gsTab + nOff, grp_idx, (size_t)nIdx * 4, hipMemcpyHostToDevice, db->stream));
    return IGD_HIP_OK;
}

// igd_sets_group_support on `ns` slices of the table at db->d_setSlices
static int group_support_launch(igd_hip_db *db, const SliceImage &im, int ns, int grid, int v, int32_t nG, bool ov, MinOv mo)
{
    const int64_t nW = ((int64_t)nG + 31) / 32;
    const size_t ldsB = (size_t)(4 + nG + (IGD_SETS_WG / IGD_WAVE) * nW) * 4;
    const int32_t *off = db->d_gsTab, *idx = db->d_gsTab + (int64_t)db->nFiles + 1;
    u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
    with_flags(im.useV, ov, [&](auto V, auto O) {
        igd_sets_group_support<V(), O()><<<grid, IGD_SETS_WG, ldsB, db->stream>>>(im.view, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns,
                                                                                 im.krule, v, off, idx, nG, R, T, mo);
    });
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

// the argument checks both entries make before they write anything
static int group_args_check(const char *who, const igd_hip_db *db, int32_t nsets, int rule, const int32_t *grp_off, const int32_t *grp_idx,
                            int32_t ngroups, const igd_hip_min_overlap *min_overlap)
{
    if (!igd_hip_min_overlap_valid(min_overlap)) {
        snprintf(g_err, sizeof g_err, "%s: min_overlap (%d bp, %d ppm, %d ppm) out of range", who, (int)min_overlap->min_bp,
                 (int)min_overlap->ppm_query, (int)min_overlap->ppm_record);
        return IGD_HIP_ERR_ARG;
    }
    if (!db || nsets < 0 || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return IGD_HIP_ERR_ARG;
    }
    return groups_check(who, db->nFiles, grp_off, grp_idx, ngroups);
}

extern "C" int igd_hip_group_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                          int32_t nsets, const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule,
                                          int64_t *gsupport, int64_t *gnhit, const igd_hip_min_overlap *min_overlap)
{
    int rc = group_args_check("igd_hip_group_support_sets", db, nsets, rule, grp_off, grp_idx, ngroups, min_overlap);
    if (rc != IGD_HIP_OK) return rc;
    if (nsets > 0 && (!set_off || !gsupport)) {
        snprintf(g_err, sizeof g_err, "igd_hip_group_support_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    if ((rc = sets_check("igd_hip_group_support_sets", ichr, qs, qe, set_off, nsets)) != IGD_HIP_OK) return rc;
    if (set_off[nsets] == 0 || db->nFiles == 0 || grp_off[db->nFiles] == 0) return IGD_HIP_OK;

    const bool ov = igd_hip_min_overlap_active(min_overlap);
    const MinOv mo = min_ov_of(min_overlap);
    const SliceImage im = slice_image(db, rule, v);
    HIPCHK(hipSetDevice(db->device));
    if ((rc = groups_upload(db, grp_off, grp_idx)) != IGD_HIP_OK) return rc;
    return run_set_chunks(db, ichr, qs, qe, set_off, nsets, ngroups, sets_slice_len(set_off[nsets]), IGD_SETS_GRID, INT64_MAX, gsupport, gnhit,
                          [&](int64_t, int64_t, int) { return IGD_HIP_OK; },
                          [&](int ns, int grid) { return group_support_launch(db, im, ns, grid, v, ngroups, ov, mo); }, no_big_sets);
}

extern "C" int igd_hip_group_enrich_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off,
                                         int32_t nsets, const int32_t *u_ichr, const int32_t *u_qs, const int32_t *u_qe, int64_t nu,
                                         const int32_t *grp_off, const int32_t *grp_idx, int32_t ngroups, int32_t v, int rule,
                                         int64_t *gsupport, int64_t *gusupport, double *pvalue_log, double *odds_ratio, int64_t *clamped,
                                         int64_t *gnhit, int64_t *gunhit, const igd_hip_min_overlap *min_overlap)
{
    int rc = group_args_check("igd_hip_group_enrich_sets", db, nsets, rule, grp_off, grp_idx, ngroups, min_overlap);
    if (rc != IGD_HIP_OK) return rc;
    if (nsets == INT32_MAX || nu < 0 || (nu > 0 && (!u_ichr || !u_qs || !u_qe)) || !gusupport ||
        (nsets > 0 && (!set_off || !gsupport || !pvalue_log))) {
        snprintf(g_err, sizeof g_err, "igd_hip_group_enrich_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if ((rc = sets_check("igd_hip_group_enrich_sets", ichr, qs, qe, set_off, nsets)) != IGD_HIP_OK) return rc;
    const int64_t nq = nsets > 0 ? set_off[nsets] : 0;
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] - set_off[k] + nu >= IGD_FISHER_MAX_N) {      // N <= n_k + n_U whatever is clamped
            snprintf(g_err, sizeof g_err, "igd_hip_group_enrich_sets: set %d and the universe hold 2^31 regions or more", (int)k);
            return IGD_HIP_ERR_ARG;
        }
    const int64_t nG = ngroups, ncell = (int64_t)nsets * nG;

    // one group-support call: the caller's sets, then the universe
    std::vector<int64_t> rows((size_t)((int64_t)(nsets + 1) * nG), 0), hit((size_t)nsets + 1, 0), nk((size_t)nsets + 1, 0);
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
        rc = igd_hip_group_support_sets(db, cc.data(), cs.data(), ce.data(), off.data(), nsets + 1, grp_off, grp_idx, ngroups, v, rule,
                                        rows.data(), hit.data(), min_overlap);
        if (rc != IGD_HIP_OK) return rc;
    }
    memcpy(gusupport, rows.data() + (size_t)ncell, (size_t)nG * 8);
    if (ncell) memcpy(gsupport, rows.data(), (size_t)ncell * 8);
    if (gnhit && nsets) memcpy(gnhit, hit.data(), (size_t)nsets * 8);
    if (gunhit) *gunhit = hit[(size_t)nsets];
    if (clamped && nsets) memset(clamped, 0, (size_t)nsets * 8);
    return fisher_enrich_cells(db, nG, rows.data(), gusupport, nk.data(), nsets, nu, pvalue_log, odds_ratio, clamped);
}
