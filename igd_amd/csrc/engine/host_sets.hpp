// engine/host_sets.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_search_sets: many query sets in one call, one hits[] row per set
// ------------------------------------------------------------------------------------------
// The sets are taken in CHUNKS: contiguous runs of sets whose queries fit one engine batch (igd_hip_max_batch()) and whose
// device rows fit IGD_SETS_ROW_BYTES.  A set may be cut at a chunk's end: its row is a sum, and the rest of the set opens the
// next chunk.  Per chunk: the queries go to the device once; sets of fewer than IGD_SETS_BIG_MIN queries are cut into slices
// for igd_sets_count (sets_dev.hpp), one launch for all of them; each larger set (its part in this chunk) is counted by the
// batch pipeline of igd_hip_search_dev into its own row, so a single large set costs what igd_hip_search_ex costs; then the
// chunk's rows and totals come back and are added to the caller's.
#define IGD_SETS_ROW_BYTES ((int64_t)256 << 20)   // device rows of one chunk (10^5 sets x 1 900 files would be 1.5 GB)
#define IGD_SETS_BIG_MIN_DEFAULT ((int64_t)1 << 17)
#define IGD_SETS_SLICES 4096                      // slices the small sets of a chunk are cut into, about (16 per CU) ...
#define IGD_SETS_SLICE_MIN 64                     // ... within these bounds of queries per slice
#define IGD_SETS_SLICE_MAX 4096                    // (igd_sets_support keeps 32-bit LDS counters that a query raises by at most 1 and that are
                                                  // flushed per slice: they hold because a slice has at most this many queries -- support_dev.hpp)

// Sets with at least this many queries take the batch pipeline.  The TEST-ONLY variable IGD_SETS_BIG_MIN (read per call)
// moves the boundary so that both routes, and a mix of them in one call, are reached by small fixtures.
static int64_t sets_big_min(void)
{
    const char *e = getenv("IGD_SETS_BIG_MIN");
    const long long x = (e && *e) ? atoll(e) : 0;
    return x >= 1 ? (int64_t)x : IGD_SETS_BIG_MIN_DEFAULT;
}

static int ensure_sets_ws(igd_hip_db *db, int64_t rowWords, int64_t rows, int64_t nSlices)
{
    int rc;
    if (rowWords > db->setRowCap || rows > db->setTotCap) {
        HIPCHK(hipStreamSynchronize(db->stream));
        if (db->d_setRows) (void)hipFree(db->d_setRows);
        if (db->d_setTot) (void)hipFree(db->d_setTot);
        db->d_setRows = db->d_setTot = nullptr;
        db->setRowCap = db->setTotCap = 0;
        if ((rc = dalloc(&db->d_setRows, (size_t)rowWords, nullptr)) != IGD_HIP_OK) return rc;
        if ((rc = dalloc(&db->d_setTot, (size_t)rows, nullptr)) != IGD_HIP_OK) return rc;
        db->setRowCap = rowWords; db->setTotCap = rows;
    }
    if (nSlices > db->setSliceCap) {
        HIPCHK(hipStreamSynchronize(db->stream));
        if (db->d_setSlices) (void)hipFree(db->d_setSlices);
        db->d_setSlices = nullptr; db->setSliceCap = 0;
        if ((rc = dalloc(&db->d_setSlices, (size_t)nSlices, nullptr)) != IGD_HIP_OK) return rc;
        db->setSliceCap = nSlices;
    }
    return IGD_HIP_OK;
}

// the kernel's copy of a caller's threshold (NULL or all zero: inactive -- the plain kernels are launched)
static inline MinOv min_ov_of(const igd_hip_min_overlap *t)
{
    return igd_hip_min_overlap_active(t) ? MinOv{t->min_bp, t->ppm_query, t->ppm_record} : MinOv{0, 0, 0};
}

// With an active threshold EVERY set is cut into slices for igd_sets_count_ov: the batch pipeline takes no threshold.
extern "C" int igd_hip_search_sets_ov(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                      const int64_t *set_off, int32_t nsets, int32_t v, int rule, int flags,
                                      int64_t *hits, int64_t *totals, const igd_hip_min_overlap *min_overlap)
{
    if (!igd_hip_min_overlap_valid(min_overlap)) {
        snprintf(g_err, sizeof g_err, "igd_hip_search_sets: min_overlap (%d bp, %d ppm, %d ppm) out of range", (int)min_overlap->min_bp,
                 (int)min_overlap->ppm_query, (int)min_overlap->ppm_record);
        return IGD_HIP_ERR_ARG;
    }
    const bool ov = igd_hip_min_overlap_active(min_overlap);
    const MinOv mo = min_ov_of(min_overlap);
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !hits)) || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT) ||
        ((flags & IGD_HIP_FLAG_SORTED) && (flags & IGD_HIP_FLAG_BUCKET))) {
        snprintf(g_err, sizeof g_err, "igd_hip_search_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    if (set_off[0] != 0) {
        snprintf(g_err, sizeof g_err, "igd_hip_search_sets: set_off[0] = %lld, not 0", (long long)set_off[0]);
        return IGD_HIP_ERR_ARG;
    }
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] < set_off[k]) {
            snprintf(g_err, sizeof g_err, "igd_hip_search_sets: set_off decreases at set %d", (int)k);
            return IGD_HIP_ERR_ARG;
        }
    const int64_t nq = set_off[nsets];
    if (nq > 0 && (!ichr || !qs || !qe)) {
        snprintf(g_err, sizeof g_err, "igd_hip_search_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nq == 0 || db->nFiles == 0) return IGD_HIP_OK;

    // the image the slice kernel reads: the re-tiled copy when there is one, with the rule word its grouping kernels get
    // (rule FLAT over the copy's tiles, bit 8 = rule NEST on the FILE's tiles; search_dev_impl)
    igd_hip_db *img = db->inner ? db->inner : db;
    const int krule = db->inner ? (IGD_HIP_RULE_FLAT | (rule == IGD_HIP_RULE_NEST ? 0x100 : 0)) : rule;
    const bool useV = v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1;     // gType 0 has no value field
    const bool lds = (int64_t)db->nFiles <= IGD_SETS_LDS_FILES;
    const int64_t nF = db->nFiles;
    const int64_t step = max_batch();
    const int64_t rowCap = IGD_SETS_ROW_BYTES / (nF * 8) > 0 ? IGD_SETS_ROW_BYTES / (nF * 8) : 1;
    const int64_t bigMin = ov ? INT64_MAX : sets_big_min();
    const int bigFlags = flags & ~IGD_HIP_FLAG_ZERO_FIRST;
    int64_t nSmall = 0;
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] - set_off[k] < bigMin) nSmall += set_off[k + 1] - set_off[k];
    int64_t sliceLen = (nSmall + IGD_SETS_SLICES - 1) / IGD_SETS_SLICES;
    sliceLen = sliceLen < IGD_SETS_SLICE_MIN ? IGD_SETS_SLICE_MIN : sliceLen > IGD_SETS_SLICE_MAX ? IGD_SETS_SLICE_MAX : sliceLen;

    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    std::vector<int64_t> hrows, htot;
    struct Big { int32_t row; int64_t a, b; };
    std::vector<Big> bigs;
    int32_t k = 0;
    int64_t pos = 0;                                     // next query to be counted (in set k)
    while (k < nsets) {
        // one chunk: sets k0.., queries [c0, pos)
        const int32_t k0 = k;
        const int64_t c0 = pos;
        int64_t rows = 0;
        slices.clear(); bigs.clear();
        while (k < nsets && k - k0 < rowCap) {
            const int64_t end = set_off[k + 1] < c0 + step ? set_off[k + 1] : c0 + step;
            const int32_t row = k - k0;
            rows = row + 1;
            if (end > pos) {
                if (set_off[k + 1] - set_off[k] >= bigMin) bigs.push_back(Big{row, pos - c0, end - c0});
                else
                    for (int64_t a = pos; a < end; a += sliceLen)
                        slices.push_back(SetSlice{row, (int32_t)(a - c0), (int32_t)((a + sliceLen < end ? a + sliceLen : end) - c0), 0});
            }
            pos = end;
            if (pos < set_off[k + 1]) break;             // the batch is full: the rest of set k opens the next chunk
            k++;
        }
        const int64_t m = pos - c0;
        if (m == 0) continue;                            // (only empty sets: their rows stay as they are)
        int rc = ensure_qstage(db, m);
        if (rc == IGD_HIP_OK) rc = ensure_sets_ws(db, rows * nF, rows, (int64_t)slices.size());
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemcpyAsync(db->d_qc, ichr + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_qs, qs + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(db->d_qe, qe + c0, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
        HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
        if (!slices.empty()) {
            HIPCHK(hipMemcpyAsync(db->d_setSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
            const int ns = (int)slices.size();
            const int grid = ns < IGD_SETS_GRID ? ns : IGD_SETS_GRID;
            const size_t ldsB = lds ? (size_t)nF * 8 : 0;
            u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
            if (ov && useV && lds) igd_sets_count_ov<true, true><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, mo);
            else if (ov && useV) igd_sets_count_ov<true, false><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, mo);
            else if (ov && lds) igd_sets_count_ov<false, true><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, mo);
            else if (ov) igd_sets_count_ov<false, false><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T, mo);
            else if (useV && lds) igd_sets_count<true, true><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T);
            else if (useV) igd_sets_count<true, false><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T);
            else if (lds) igd_sets_count<false, true><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T);
            else igd_sets_count<false, false><<<grid, IGD_SETS_WG, ldsB, st>>>(img->v, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, krule, v, R, T);
            HIPCHK(hipGetLastError());
        }
        for (const Big &b : bigs) {
            // the batch pipeline into row b.row (ADDED to, like the slices' adds); a broken order promise adds nothing and is
            // repaired as igd_hip_search_ex repairs it: the same queries once more, the device choosing the grouping
            int64_t *row = db->d_setRows + (int64_t)b.row * nF, *tot = db->d_setTot + b.row;
            rc = igd_hip_search_dev(db, db->d_qc + b.a, db->d_qs + b.a, db->d_qe + b.a, b.b - b.a, v, rule, bigFlags, row, tot, st);
            if (rc == IGD_HIP_OK) rc = igd_hip_sync(db, st);
            if (rc == IGD_HIP_ERR_UNSORTED) {
                rc = igd_hip_search_dev(db, db->d_qc + b.a, db->d_qs + b.a, db->d_qe + b.a, b.b - b.a, v, rule,
                                        bigFlags & ~(IGD_HIP_FLAG_SORTED | IGD_HIP_FLAG_SHORT), row, tot, st);
                if (rc == IGD_HIP_OK) rc = igd_hip_sync(db, st);
            }
            if (rc != IGD_HIP_OK) return rc;
        }
        hrows.resize((size_t)(rows * nF));
        htot.resize((size_t)rows);
        HIPCHK(hipMemcpyAsync(hrows.data(), db->d_setRows, (size_t)(rows * nF) * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(htot.data(), db->d_setTot, (size_t)rows * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        for (int64_t r = 0; r < rows; r++) {
            int64_t *dst = hits + (k0 + r) * nF;
            const int64_t *src = hrows.data() + r * nF;
            for (int64_t f = 0; f < nF; f++) dst[f] += src[f];
            if (totals) totals[k0 + r] += htot[(size_t)r];
        }
    }
    return IGD_HIP_OK;
}

extern "C" int igd_hip_search_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                   const int64_t *set_off, int32_t nsets, int32_t v, int rule, int flags,
                                   int64_t *hits, int64_t *totals)
{
    return igd_hip_search_sets_ov(db, ichr, qs, qe, set_off, nsets, v, rule, flags, hits, totals, nullptr);
}
