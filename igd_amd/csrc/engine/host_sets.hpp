// engine/host_sets.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_search_sets: many query sets in one call, one hits[] row per set
// ------------------------------------------------------------------------------------------
// The sets are taken in the CHUNKS of run_set_chunks (host_common.hpp): contiguous runs of sets whose queries fit one engine
// batch and whose device rows fit sets_row_bytes().  Per chunk: sets of fewer than IGD_SETS_BIG_MIN queries are cut into slices
// for igd_sets_count (sets_dev.hpp), one launch for all of them; each larger set (its part in this chunk) is counted by the
// batch pipeline of igd_hip_search_dev into its own row, so a single large set costs what igd_hip_search_ex costs; then the
// chunk's rows and totals come back and are added to the caller's.
#define IGD_SETS_ROW_BYTES ((int64_t)256 << 20)   // device rows of one chunk (10^5 sets x 1 900 files would be 1.5 GB)
#define IGD_SETS_BIG_MIN_DEFAULT ((int64_t)1 << 17)
#define IGD_SETS_SLICES 4096                      // slices the small sets of a chunk are cut into, about (16 per CU) ...
#define IGD_SETS_SLICE_MIN 64                     // ... within these bounds of queries per slice
#define IGD_SETS_SLICE_MAX 4096                    // (igd_sets_support keeps 32-bit LDS counters that a query raises by at most 1 and that are
                                                  // flushed per slice: they hold because a slice has at most this many queries -- support_dev.hpp)

// Device rows of one chunk of sets.  The TEST-ONLY variable IGD_HIP_SETS_ROW_BYTES (read once per process) lowers the budget so
// that small fixtures cross the row seam; perm_row_bytes() and restrict_row_bytes() default to it.
static int64_t sets_row_bytes(void)
{
    static const int64_t m = env_positive("IGD_HIP_SETS_ROW_BYTES", IGD_SETS_ROW_BYTES);
    return m;
}

static int64_t sets_slice_len(int64_t n)
{
    const int64_t len = (n + IGD_SETS_SLICES - 1) / IGD_SETS_SLICES;
    return len < IGD_SETS_SLICE_MIN ? IGD_SETS_SLICE_MIN : len > IGD_SETS_SLICE_MAX ? IGD_SETS_SLICE_MAX : len;
}

// Sets with at least this many queries take the batch pipeline.  The TEST-ONLY variable IGD_SETS_BIG_MIN (read per call)
// moves the boundary so that both routes, and a mix of them in one call, are reached by small fixtures.
static int64_t sets_big_min(void) { return env_positive("IGD_SETS_BIG_MIN", IGD_SETS_BIG_MIN_DEFAULT); }

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
    int rc = sets_check("igd_hip_search_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    if (set_off[nsets] == 0 || db->nFiles == 0) return IGD_HIP_OK;

    const SliceImage im = slice_image(db, rule, v);
    const int64_t nF = db->nFiles;
    const bool lds = nF <= IGD_SETS_LDS_FILES;
    const int64_t bigMin = ov ? INT64_MAX : sets_big_min();
    const int bigFlags = flags & ~IGD_HIP_FLAG_ZERO_FIRST;
    int64_t nSmall = 0;
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] - set_off[k] < bigMin) nSmall += set_off[k + 1] - set_off[k];
    hipStream_t st = db->stream;
    auto launch = [&](int ns, int grid) {
        u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
        with_flags(im.useV, lds, [&](auto V, auto L) {
            const size_t ldsB = L() ? (size_t)nF * 8 : 0;
            if (ov) igd_sets_count_ov<V(), L()><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, im.krule, v, R, T, mo);
            else igd_sets_count<V(), L()><<<grid, IGD_SETS_WG, ldsB, st>>>(im.view, db->d_qc, db->d_qs, db->d_qe, db->d_setSlices, ns, im.krule, v, R, T);
        });
        return IGD_HIP_OK;
    };
    // the batch pipeline into row `row` (ADDED to, like the slices' adds); a broken order promise adds nothing and is
    // repaired as igd_hip_search_ex repairs it: the same queries once more, the device choosing the grouping
    auto big = [&](int32_t row, int64_t a, int64_t b) {
        int64_t *dst = db->d_setRows + (int64_t)row * nF, *tot = db->d_setTot + row;
        int r = igd_hip_search_dev(db, db->d_qc + a, db->d_qs + a, db->d_qe + a, b - a, v, rule, bigFlags, dst, tot, st);
        if (r == IGD_HIP_OK) r = igd_hip_sync(db, st);
        if (r == IGD_HIP_ERR_UNSORTED) {
            r = igd_hip_search_dev(db, db->d_qc + a, db->d_qs + a, db->d_qe + a, b - a, v, rule,
                                   bigFlags & ~(IGD_HIP_FLAG_SORTED | IGD_HIP_FLAG_SHORT), dst, tot, st);
            if (r == IGD_HIP_OK) r = igd_hip_sync(db, st);
        }
        return r;
    };
    return run_set_chunks(db, ichr, qs, qe, set_off, nsets, db->nFiles, sets_slice_len(nSmall), IGD_SETS_GRID, bigMin, hits, totals,
                          [](int64_t, int64_t, int) { return IGD_HIP_OK; }, launch, big);
}

extern "C" int igd_hip_search_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                   const int64_t *set_off, int32_t nsets, int32_t v, int rule, int flags,
                                   int64_t *hits, int64_t *totals)
{
    return igd_hip_search_sets_ov(db, ichr, qs, qe, set_off, nsets, v, rule, flags, hits, totals, nullptr);
}
