// engine/host_support.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_support_sets: per set and file, the queries of the set that overlap at least one record of the file
// ------------------------------------------------------------------------------------------
// Chunks as in igd_hip_search_sets (run_set_chunks, host_common.hpp): contiguous runs of sets whose queries fit one engine batch and
// whose device rows fit sets_row_bytes(); a set may be cut at a chunk's end (support is a sum over queries), a query never is.
// Per chunk the queries go to the device once, EVERY set is cut into slices for igd_sets_support (support_dev.hpp) -- there
// is no large-set route: the batch pipeline is tile-major and does not know what a query met in another unit -- one launch
// counts them, and the chunk's rows and nhit come back and are added to the caller's.  The staging buffers, rows, totals
// and slice table are those of igd_hip_search_sets; only the wide form's bitmap stripes are this file's own.
// igd_sets_support's LDS counters are 32 bits wide: a query adds at most 1 per file and a slice is flushed at its end
static_assert((unsigned long long)IGD_SETS_SLICE_MAX <= 0xffffffffull, "a slice must fit the 32-bit LDS counters of igd_sets_support");
#define IGD_SUPPORT_BITS_BYTES ((int64_t)256 << 20)   // wide form: the grid is cut so that its stripes stay below this

// the LDS form, or the wide form with the waves' bitmaps in global memory (support_dev.hpp): decided here, nowhere else
static bool support_lds(const igd_hip_db *db) { return (int64_t)db->nFiles <= IGD_SUPPORT_LDS_FILES; }

// wide form only: one zeroed stripe of nW words per wave of a grid of `maxGrid` workgroups
static int ensure_support_bits(igd_hip_db *db, int64_t maxGrid)
{
    if (support_lds(db)) return IGD_HIP_OK;
    bool grew;
    const int64_t words = maxGrid * (IGD_SETS_WG / IGD_WAVE) * (((int64_t)db->nFiles + 31) / 32);
    const int rc = dev_grow(db, &db->d_supBits, &db->supBitsCap, words, &grew);
    // zeroed once: every wave of igd_sets_support leaves its stripe all zero
    if (rc == IGD_HIP_OK && grew) HIPCHK(hipMemsetAsync(db->d_supBits, 0, (size_t)words * 4, db->stream));
    return rc;
}
static int64_t support_max_grid(const igd_hip_db *db)
{
    // wide form: as many workgroups as IGD_SUPPORT_BITS_BYTES of stripes allow (10^6 files: 128 KiB per wave, 512 workgroups)
    const int64_t nW = ((int64_t)db->nFiles + 31) / 32;
    return support_lds(db) ? IGD_SETS_GRID : wide_grid(IGD_SUPPORT_BITS_BYTES, nW * 4 * (IGD_SETS_WG / IGD_WAVE));
}

// igd_sets_support, or igd_sets_support_ov under an active threshold (mo), on `ns` slices of the table at db->d_setSlices
static int support_launch(igd_hip_db *db, const SliceImage &im, const int32_t *c, const int32_t *s, const int32_t *e, int ns, int grid,
                          int v, bool ov, MinOv mo)
{
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    hipStream_t st = db->stream;
    u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
    with_flags(im.useV, support_lds(db), [&](auto V, auto L) {
        const size_t ldsB = L() ? (size_t)(4 + nF + (IGD_SETS_WG / IGD_WAVE) * nW) * 4 : 0;
        if (ov) igd_sets_support_ov<V(), L()><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, c, s, e, db->d_setSlices, ns, im.krule, v, R, T, db->d_supBits, mo);
        else igd_sets_support<V(), L()><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, c, s, e, db->d_setSlices, ns, im.krule, v, R, T, db->d_supBits);
    });
    HIPCHK(hipGetLastError());
    return IGD_HIP_OK;
}

extern "C" int igd_hip_support_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                       const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *support, int64_t *nhit,
                                       const igd_hip_min_overlap *min_overlap)
{
    if (!igd_hip_min_overlap_valid(min_overlap)) {
        snprintf(g_err, sizeof g_err, "igd_hip_support_sets: min_overlap (%d bp, %d ppm, %d ppm) out of range", (int)min_overlap->min_bp,
                 (int)min_overlap->ppm_query, (int)min_overlap->ppm_record);
        return IGD_HIP_ERR_ARG;
    }
    const bool ov = igd_hip_min_overlap_active(min_overlap);
    const MinOv mo = min_ov_of(min_overlap);
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !support)) || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_support_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_support_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    if (set_off[nsets] == 0 || db->nFiles == 0) return IGD_HIP_OK;

    const SliceImage im = slice_image(db, rule, v);
    const int64_t maxGrid = support_max_grid(db);
    return run_set_chunks(db, ichr, qs, qe, set_off, nsets, db->nFiles, sets_slice_len(set_off[nsets]), maxGrid, INT64_MAX, support, nhit,
                          [&](int64_t, int64_t, int) { return ensure_support_bits(db, maxGrid); },
                          [&](int ns, int grid) { return support_launch(db, im, db->d_qc, db->d_qs, db->d_qe, ns, grid, v, ov, mo); },
                          no_big_sets);
}

extern "C" int igd_hip_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                    const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *support, int64_t *nhit)
{
    return igd_hip_support_sets_ov(db, ichr, qs, qe, set_off, nsets, v, rule, support, nhit, nullptr);
}
