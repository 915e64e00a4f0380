// engine/host_support.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_support_sets: per set and file, the queries of the set that overlap at least one record of the file
// ------------------------------------------------------------------------------------------
// Chunks as in igd_hip_search_sets (host_sets.hpp): contiguous runs of sets whose queries fit one engine batch and whose
// device rows fit IGD_SETS_ROW_BYTES; a set may be cut at a chunk's end (support is a sum over queries), a query never is.
// Per chunk the queries go to the device once, EVERY set is cut into slices for igd_sets_support (support_dev.hpp) -- there
// is no large-set route: the batch pipeline is tile-major and does not know what a query met in another unit -- one launch
// counts them, and the chunk's rows and nhit come back and are added to the caller's.  The staging buffers, rows, totals
// and slice table are those of igd_hip_search_sets; only the wide form's bitmap stripes are this file's own.
// igd_sets_support's LDS counters are 32 bits wide: a query adds at most 1 per file and a slice is flushed at its end
static_assert((unsigned long long)IGD_SETS_SLICE_MAX <= 0xffffffffull, "a slice must fit the 32-bit LDS counters of igd_sets_support");
#define IGD_SUPPORT_BITS_BYTES ((int64_t)256 << 20)   // wide form: the grid is cut so that its stripes stay below this

// wide form (more than IGD_SUPPORT_LDS_FILES files): one zeroed stripe of `nW` words per wave of a grid of `grid` workgroups
static int ensure_support_bits(igd_hip_db *db, int64_t words)
{
    if (words <= db->supBitsCap) return IGD_HIP_OK;
    int rc;
    HIPCHK(hipStreamSynchronize(db->stream));
    if (db->d_supBits) (void)hipFree(db->d_supBits);
    db->d_supBits = nullptr; db->supBitsCap = 0;
    if ((rc = dalloc(&db->d_supBits, (size_t)words, nullptr)) != IGD_HIP_OK) return rc;
    db->supBitsCap = words;
    // zeroed once: every wave of igd_sets_support leaves its stripe all zero
    HIPCHK(hipMemsetAsync(db->d_supBits, 0, (size_t)words * 4, db->stream));
    return IGD_HIP_OK;
}

// igd_sets_support, or igd_sets_support_ov under an active threshold (mo), on `ns` slices of the table at db->d_setSlices
static int support_launch(igd_hip_db *db, const DbView &view, const int32_t *c, const int32_t *s, const int32_t *e, int ns, int grid,
                          int krule, int v, bool useV, bool lds, bool ov, MinOv mo)
{
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    const size_t ldsB = lds ? (size_t)(4 + nF + (IGD_SETS_WG / IGD_WAVE) * nW) * 4 : 0;
    hipStream_t st = db->stream;
    u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
    unsigned *B = (unsigned *)db->d_supBits;
    if (ov && useV && lds) igd_sets_support_ov<true, true><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B, mo);
    else if (ov && useV) igd_sets_support_ov<true, false><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B, mo);
    else if (ov && lds) igd_sets_support_ov<false, true><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B, mo);
    else if (ov) igd_sets_support_ov<false, false><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B, mo);
    else if (useV && lds) igd_sets_support<true, true><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B);
    else if (useV) igd_sets_support<true, false><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B);
    else if (lds) igd_sets_support<false, true><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B);
    else igd_sets_support<false, false><<<grid, IGD_SETS_WG, ldsB, st>>>(view, c, s, e, db->d_setSlices, ns, krule, v, R, T, B);
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
    if (set_off[0] != 0) {
        snprintf(g_err, sizeof g_err, "igd_hip_support_sets: set_off[0] = %lld, not 0", (long long)set_off[0]);
        return IGD_HIP_ERR_ARG;
    }
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] < set_off[k]) {
            snprintf(g_err, sizeof g_err, "igd_hip_support_sets: set_off decreases at set %d", (int)k);
            return IGD_HIP_ERR_ARG;
        }
    const int64_t nq = set_off[nsets];
    if (nq > 0 && (!ichr || !qs || !qe)) {
        snprintf(g_err, sizeof g_err, "igd_hip_support_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0 || db->nFiles == 0) return IGD_HIP_OK;

    // the image and the rule word as igd_hip_search_sets gives them to igd_sets_count (re-tiled copy, its gate bit)
    igd_hip_db *img = db->inner ? db->inner : db;
    const int krule = db->inner ? (IGD_HIP_RULE_FLAT | (rule == IGD_HIP_RULE_NEST ? 0x100 : 0)) : rule;
    const bool useV = v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1;     // gType 0 has no value field
    const bool lds = (int64_t)db->nFiles <= IGD_SUPPORT_LDS_FILES;
    const int64_t nF = db->nFiles, nW = (nF + 31) / 32;
    const int64_t step = max_batch();
    const int64_t rowCap = IGD_SETS_ROW_BYTES / (nF * 8) > 0 ? IGD_SETS_ROW_BYTES / (nF * 8) : 1;
    int64_t sliceLen = (nq + IGD_SETS_SLICES - 1) / IGD_SETS_SLICES;
    sliceLen = sliceLen < IGD_SETS_SLICE_MIN ? IGD_SETS_SLICE_MIN : sliceLen > IGD_SETS_SLICE_MAX ? IGD_SETS_SLICE_MAX : sliceLen;
    // wide form: as many workgroups as IGD_SUPPORT_BITS_BYTES of stripes allow (10^6 files: 128 KiB per wave, 512 workgroups)
    int64_t maxGrid = IGD_SETS_GRID;
    if (!lds) {
        const int64_t g = IGD_SUPPORT_BITS_BYTES / (nW * 4 * (IGD_SETS_WG / IGD_WAVE));
        maxGrid = g < 1 ? 1 : g < IGD_SETS_GRID ? g : IGD_SETS_GRID;
    }

    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    std::vector<int64_t> hrows, htot;
    int32_t k = 0;
    int64_t pos = 0;                                     // next query to be counted (in set k)
    while (k < nsets) {
        // one chunk: sets k0.., queries [c0, pos)
        const int32_t k0 = k;
        const int64_t c0 = pos;
        int64_t rows = 0;
        slices.clear();
        while (k < nsets && k - k0 < rowCap) {
            const int64_t end = set_off[k + 1] < c0 + step ? set_off[k + 1] : c0 + step;
            const int32_t row = k - k0;
            rows = row + 1;
            for (int64_t a = pos; a < end; a += sliceLen)
                slices.push_back(SetSlice{row, (int32_t)(a - c0), (int32_t)((a + sliceLen < end ? a + sliceLen : end) - c0), 0});
            pos = end;
            if (pos < set_off[k + 1]) break;             // the batch is full: the rest of set k opens the next chunk
            k++;
        }
        const int64_t m = pos - c0;
        if (m == 0) continue;                            // (only empty sets: their rows stay as they are)
        const int ns = (int)slices.size();
        const int grid = ns < maxGrid ? ns : (int)maxGrid;
        int rc = ensure_qstage(db, m);
        if (rc == IGD_HIP_OK) rc = ensure_sets_ws(db, rows * nF, rows, (int64_t)ns);
        if (rc == IGD_HIP_OK && !lds) rc = ensure_support_bits(db, maxGrid * (IGD_SETS_WG / IGD_WAVE) * nW);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(db->d_qc, ichr + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_qs, qs + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_qe, qe + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
        HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
        HIPCHK(hipMemcpyAsync(db->d_setSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        if ((rc = support_launch(db, img->v, db->d_qc, db->d_qs, db->d_qe, ns, grid, krule, v, useV, lds, ov, mo)) != IGD_HIP_OK) return rc;
        hrows.resize((size_t)(rows * nF));
        htot.resize((size_t)rows);
        HIPCHK(hipMemcpyAsync(hrows.data(), db->d_setRows, (size_t)(rows * nF) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(htot.data(), db->d_setTot, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        for (int64_t r = 0; r < rows; r++) {
            int64_t *dst = support + (k0 + r) * nF;
            const int64_t *src = hrows.data() + r * nF;
            for (int64_t f = 0; f < nF; f++) dst[f] += src[f];
            if (nhit) nhit[k0 + r] += htot[(size_t)r];
        }
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_support_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                    const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *support, int64_t *nhit)
{
    return igd_hip_support_sets_ov(db, ichr, qs, qe, set_off, nsets, v, rule, support, nhit, nullptr);
}
