// engine/host_coverage.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_hip_coverage_sets: per set and file, the base pairs of the set's queries that lie under the file's records
// ------------------------------------------------------------------------------------------
// Chunks as igd_hip_support_sets (run_set_chunks, host_common.hpp): contiguous runs of sets whose queries fit one engine batch and
// whose device rows fit sets_row_bytes(); a set may be cut at a chunk's end (coverage is a sum over queries), a query never is.
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
    bool grew;
    const int rc = dev_grow(db, &db->d_covFront, &db->covFrontCap, words, &grew);
    if (rc != IGD_HIP_OK) return rc;
    if (grew) db->covTag = 0xffffffffull;                // (new memory: zero it below)
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

// igd_sets_coverage over `ns` slices of the table at db->d_setSlices, queries (c, s, e), into db->d_setRows / d_setTot (zeroed)
static int coverage_launch(igd_hip_db *db, const SliceImage &im, const int32_t *c, const int32_t *s, const int32_t *e, int ns, int grid,
                           int32_t v, unsigned tag0)
{
    const int64_t nF = db->nFiles;
    u64 *R = (u64 *)db->d_setRows, *T = (u64 *)db->d_setTot;
    with_flags(im.useV, nF <= IGD_COVERAGE_LDS_FILES, [&](auto V, auto L) {
        const size_t ldsB = L() ? (size_t)(2 + nF * (1 + IGD_SETS_WG / IGD_WAVE)) * 8 : 0;
        if (ldsB > (size_t)65536)                        // (more dynamic LDS than a launch gets unasked)
            (void)hipFuncSetAttribute((const void *)igd_sets_coverage<V(), L()>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsB);
        igd_sets_coverage<V(), L()><<<grid, IGD_SETS_WG, ldsB, db->stream>>>(im.view, c, s, e, db->d_setSlices, ns, im.krule, v, R, T,
                                                                            (u64 *)db->d_covFront, tag0);
    });
    return IGD_HIP_OK;
}

extern "C" int igd_hip_coverage_sets(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe,
                                    const int64_t *set_off, int32_t nsets, int32_t v, int rule, int64_t *coverage, int64_t *covered)
{
    if (!db || nsets < 0 || (nsets > 0 && (!set_off || !coverage)) || (rule != IGD_HIP_RULE_NEST && rule != IGD_HIP_RULE_FLAT)) {
        snprintf(g_err, sizeof g_err, "igd_hip_coverage_sets: bad argument");
        return IGD_HIP_ERR_ARG;
    }
    if (nsets == 0) return IGD_HIP_OK;
    int rc = sets_check("igd_hip_coverage_sets", ichr, qs, qe, set_off, nsets);
    if (rc != IGD_HIP_OK) return rc;
    if (set_off[nsets] == 0 || db->nFiles == 0) return IGD_HIP_OK;

    const SliceImage im = slice_image(db, rule, v);
    const int64_t nF = db->nFiles;
    const bool lds = nF <= IGD_COVERAGE_LDS_FILES;
    // wide form: as many workgroups as IGD_COVERAGE_FRONT_BYTES of stripes allow (20 000 files: 156 KiB per wave, 419
    // workgroups; 10^6 files: 7.6 MiB per wave, 8 workgroups)
    const int64_t maxGrid = lds ? IGD_SETS_GRID : wide_grid(IGD_COVERAGE_FRONT_BYTES, nF * 8 * (IGD_SETS_WG / IGD_WAVE));
    unsigned tag0 = 0;
    auto launch = [&](int ns, int grid) { return coverage_launch(db, im, db->d_qc, db->d_qs, db->d_qe, ns, grid, v, tag0); };
    return run_set_chunks(db, ichr, qs, qe, set_off, nsets, db->nFiles, sets_slice_len(set_off[nsets]), maxGrid, INT64_MAX, coverage, covered,
                          [&](int64_t m, int64_t, int) {
                              return lds ? IGD_HIP_OK : coverage_fronts(db, maxGrid * (IGD_SETS_WG / IGD_WAVE) * nF, m, &tag0);
                          },
                          launch, no_big_sets);
}
