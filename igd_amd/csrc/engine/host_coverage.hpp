// engine/host_coverage.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_coverage_sets: per set and file, the base pairs of the set's queries that lie under the file's records
// ------------------------------------------------------------------------------------------
// Chunks as igd_hip_support_sets (host_support.hpp): contiguous runs of sets whose queries fit one engine batch and whose
// device rows fit IGD_SETS_ROW_BYTES; a set may be cut at a chunk's end (coverage is a sum over queries), a query never is.
// Per chunk the queries go to the device once, EVERY set is cut into slices for igd_sets_coverage (coverage_dev.hpp) -- no
// large-set route, for the reason given there for support: the batch pipeline is tile-major, and the union of a file's
// records under a query needs everything the query meets in one place -- one launch counts them, and the chunk's rows and
// covered[] come back and are added to the caller's.  The staging buffers, rows, totals and slice table are those of
// igd_hip_search_sets; only the wide form's frontier stripes are this file's own.
#define IGD_COVERAGE_FRONT_BYTES ((int64_t)256 << 20)   // wide form: the grid is cut so that its stripes stay below this

// wide form (more than IGD_COVERAGE_LDS_FILES files): one stripe of nFiles 64-bit frontier words per wave of the grid, and
// the tag base of a launch over `m` queries.  A wave numbers its queries tag0 + 1 .. tag0 + m at most, and a word counts
// only under the tag that wrote it, so the stripes are zeroed when they are allocated and before the tags would wrap,
// not per launch.
static int coverage_fronts(igd_hip_db *db, int64_t words, int64_t m, unsigned *tag0)
{
    int rc;
    if (words > db->covFrontCap) {
        HIPCHK(hipStreamSynchronize(db->stream));
        if (db->d_covFront) (void)hipFree(db->d_covFront);
        db->d_covFront = nullptr; db->covFrontCap = 0;
        if ((rc = dalloc(&db->d_covFront, (size_t)words, nullptr)) != IGD_HIP_OK) return rc;
        db->covFrontCap = words;
        db->covTag = 0xffffffffull;                      // (new memory: zero it below)
    }
    if (db->covTag + (unsigned long long)m >= 0xffffffffull) {
        HIPCHK(hipMemsetAsync(db->d_covFront, 0, (size_t)db->covFrontCap * 8, db->stream));
        db->covTag = 0;
    }
    *tag0 = (unsigned)db->covTag;
    db->covTag += (unsigned long long)m;
    return IGD_HIP_OK;
}

#ifdef IGD_COVERAGE_PROBE
// probe build only: iterations with a hit, and those of them that took the ordered path, since the last call
extern "C" int igd_hip_coverage_probe(unsigned long long *out)
{
    unsigned long long zero[2] = {0, 0};
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_covProbe), sizeof zero));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_covProbe), zero, sizeof zero));
    return IGD_HIP_OK;
}
#endif

extern "C" int igd_hip_coverage_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                    const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *coverage, int64_t *covered)
{
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !coverage)) || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_coverage_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    if (set_off[0] != 0) {
        snprintf(g_err, sizeof g_err, "igd_hip_coverage_sets: set_off[0] = %lld, not 0", (long long)set_off[0]);
        return IGD_HIP_ERR_ARG;
    }
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] < set_off[k]) {
            snprintf(g_err, sizeof g_err, "igd_hip_coverage_sets: set_off decreases at set %d", (int)k);
            return IGD_HIP_ERR_ARG;
        }
    const int64_t nq = set_off[nsets];
    if (nq > 0 && (!ichr || !qs || !qe)) {
        snprintf(g_err, sizeof g_err, "igd_hip_coverage_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0 || db->nFiles == 0) return IGD_HIP_OK;

    // the image and the rule word as igd_hip_support_sets gives them to igd_sets_support (re-tiled copy, its gate bit)
    igd_hip_db *img = db->inner ? db->inner : db;
    const int krule = db->inner ? (IGD_HIP_RULE_FLAT | (rule == IGD_HIP_RULE_NEST ? 0x100 : 0)) : rule;
    const bool useV = v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1;     // gType 0 has no value field
    const bool lds = (int64_t)db->nFiles <= IGD_COVERAGE_LDS_FILES;
    const int64_t nF = db->nFiles;
    const int64_t step = max_batch();
    const int64_t rowCap = IGD_SETS_ROW_BYTES / (nF * 8) > 0 ? IGD_SETS_ROW_BYTES / (nF * 8) : 1;
    int64_t sliceLen = (nq + IGD_SETS_SLICES - 1) / IGD_SETS_SLICES;
    sliceLen = sliceLen < IGD_SETS_SLICE_MIN ? IGD_SETS_SLICE_MIN : sliceLen > IGD_SETS_SLICE_MAX ? IGD_SETS_SLICE_MAX : sliceLen;
    // wide form: as many workgroups as IGD_COVERAGE_FRONT_BYTES of stripes allow (20 000 files: 156 KiB per wave, 419
    // workgroups; 10^6 files: 7.6 MiB per wave, 8 workgroups)
    int64_t maxGrid = IGD_SETS_GRID;
    if (!lds) {
        const int64_t g = IGD_COVERAGE_FRONT_BYTES / (nF * 8 * (IGD_SETS_WG / IGD_WAVE));
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
        unsigned tag0 = 0;
        if (rc == IGD_HIP_OK && !lds) rc = coverage_fronts(db, maxGrid * (IGD_SETS_WG / IGD_WAVE) * nF, m, &tag0);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(db->d_qc, ichr + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_qs, qs + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_qe, qe + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
        HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
        HIPCHK(hipMemcpyAsync(db->d_setSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
        {
            const size_t ldsB = lds ? (size_t)(2 + nF * (1 + IGD_SETS_WG / IGD_WAVE)) * 8 : 0;
            u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
            u64 *B = (u64 *)db->d_covFront;
            if (ldsB > (size_t)65536) {                  // (more dynamic LDS than a launch gets unasked)
                (void)hipFuncSetAttribute((const void *)igd_sets_coverage<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
                (void)hipFuncSetAttribute((const void *)igd_sets_coverage<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
            }
            if (useV && lds) igd_sets_coverage<true, true><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, B, tag0);
            else if (useV) igd_sets_coverage<true, false><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, B, tag0);
            else if (lds) igd_sets_coverage<false, true><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, B, tag0);
            else igd_sets_coverage<false, false><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, B, tag0);
            HIPCHK(hipGetLastError());
        }
        hrows.resize((size_t)(rows * nF));
        htot.resize((size_t)rows);
        HIPCHK(hipMemcpyAsync(hrows.data(), db->d_setRows, (size_t)(rows * nF) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(htot.data(), db->d_setTot, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        for (int64_t r = 0; r < rows; r++) {
            int64_t *dst = coverage + (k0 + r) * nF;
            const int64_t *src = hrows.data() + r * nF;
            for (int64_t f = 0; f < nF; f++) dst[f] += src[f];
            if (covered) covered[k0 + r] += htot[(size_t)r];
        }
    }
    return IGD_HIP_OK;
}
