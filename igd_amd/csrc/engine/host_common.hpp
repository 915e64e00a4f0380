// engine/host_common.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// What the host sides of the region-set entry points share: workspace growth, query staging, the image a slice kernel reads,
// the set_off checks, slice, step and grid arithmetic, kernel dispatch by template flags, and two drivers:
//   run_region_chunks  host arrays in chunks of regions, rows back per chunk: igd_hip_nearest(_signed), igd_hip_flank,
//                      igd_hip_map, igd_hip_membership, igd_hip_cooccur
//   run_set_chunks     chunks of sets, rows added on the host: igd_hip_search_sets / igd_hip_support_sets / igd_hip_coverage_sets /
//                      igd_hip_group_support_sets (rows of ngroups columns)
// (The group driver of the resident set statistics, run_set_groups, is in host_nearest.hpp; the chunk driver of the three
// permutation nulls, run_perm_chunks, in host_permute.hpp.)
// ------------------------------------------------------------------------------------------
#include <type_traits>

// A positive integer from the environment, else dflt.  The TEST-ONLY variables that lower a budget so that small fixtures
// cross a seam are read ONCE per process, as IGD_HIP_MAX_BATCH is: their accessors keep the value in a function-local static.
static int64_t env_positive(const char *name, int64_t dflt)
{
    const char *e = getenv(name);
    const long long x = e && *e ? atoll(e) : 0;
    return x > 0 ? (int64_t)x : dflt;
}

// The grid of the four reductions over a slice table (igd_nearest_reduce, igd_nearest_hist, igd_flank_reldist, igd_map_reduce):
// gx workgroups of 64 columns across, gy down, and workgroup (x, y) takes the slices y, y + gy, ..  About IGD_REDUCE_WGS
// workgroups per launch (64 per CU), never more rows than slices or than a grid's y may have.
// The TEST-ONLY variable IGD_HIP_REDUCE_WGS (read once per process, as IGD_HIP_MAX_BATCH) lowers the number so that small
// fixtures give a workgroup a second slice.
#define IGD_REDUCE_WGS 16384
static int reduce_grid_y(int gx, int ns)
{
    static const int64_t wgs = env_positive("IGD_HIP_REDUCE_WGS", IGD_REDUCE_WGS);
    const int64_t gy = wgs / (gx > 0 ? gx : 1), top = ns < 65535 ? ns : 65535;
    return (int)(gy > top ? (top < 1 ? 1 : top) : gy < 1 ? 1 : gy);
}

// the same for ncols columns and nslices slices (tests): ncols is nFiles + 1 for the nearest family, nFiles for igd_hip_map_sets
extern "C" int32_t igd_hip_reduce_grid_y(int64_t ncols, int64_t nslices)
{
    const int64_t gx = (ncols + IGD_WAVE - 1) / IGD_WAVE;
    return reduce_grid_y((int)(gx < INT_MAX ? gx : INT_MAX), (int)(nslices < INT_MAX ? nslices : INT_MAX));
}

// the chunk driver's two budgets, defined beside their constants in host_sets.hpp
static int64_t sets_row_bytes(void);                 // device rows of one chunk of sets (IGD_SETS_ROW_BYTES; TEST-ONLY IGD_HIP_SETS_ROW_BYTES)
static int64_t sets_slice_len(int64_t n);            // queries per slice when n queries are cut for one launch (IGD_SETS_SLICES, _MIN, _MAX)

// A workspace of the handle that only grows: behind a wait for the stream (a launch may still read the old one) the old
// allocation is freed and `need` elements are allocated.  *grew: the memory is new (whoever needs it zeroed does that).
template <typename T>
static int dev_grow(igd_hip_db *db, T **p, int64_t *cap, int64_t need, bool *grew = nullptr)
{
    if (grew) *grew = false;
    if (need <= *cap) return IGD_HIP_OK;
    int rc;
    HIPCHK(hipStreamSynchronize(db->stream));
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if ((rc = dalloc(p, (size_t)need, nullptr)) != IGD_HIP_OK) return rc;
    *cap = need;
    if (grew) *grew = true;
    return IGD_HIP_OK;
}

// the rows, totals and slice table of one chunk of sets (igd_hip_db::d_setRows, d_setTot, d_setSlices)
static int sets_ws(igd_hip_db *db, int64_t rowWords, int64_t rows, int64_t nSlices)
{
    int rc = dev_grow(db, &db->d_setRows, &db->setRowCap, rowWords);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_setTot, &db->setTotCap, rows);
    if (rc == IGD_HIP_OK) rc = dev_grow(db, &db->d_setSlices, &db->setSliceCap, nSlices);
    return rc;
}

// queries [c0, c0 + m) of the caller's arrays into the staging buffers of igd_hip_search (d_qc, d_qs, d_qe), on the engine's stream
static int stage_queries(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t c0, int64_t m)
{
    const int rc = ensure_qstage(db, m);
    if (rc != IGD_HIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(db->d_qc, ichr + c0, (size_t)m * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync(db->d_qs, qs + c0, (size_t)m * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync(db->d_qe, qe + c0, (size_t)m * 4, hipMemcpyHostToDevice, db->stream));
    return IGD_HIP_OK;
}

// Regions per chunk of a host form whose device rows cost bytesPerRegion each: the batch limit, or as many as `budget` bytes of
// rows hold, at least one.  (igd_hip_nearest: 4 nFiles of nearest_row_bytes(); igd_hip_flank: 8 nFiles; igd_hip_map: 4 or 12
// nFiles of map_row_bytes(); igd_hip_membership and igd_hip_cooccur: 4 nW of member_row_bytes().)
static int64_t chunk_step(int64_t budget, int64_t bytesPerRegion)
{
    const int64_t byRows = budget / bytesPerRegion, step = max_batch();
    return byRows < step ? (byRows < 1 ? 1 : byRows) : step;
}

// The region-chunk driver of the host row forms (the arguments are checked, nq > 0).  For c0 = 0, step, ..: regions
// [c0, c0 + m) go to the staging buffers, body(c0, m, st) grows its own workspace, runs the _dev form over the staged arrays
// and enqueues the copies back to the caller's arrays at row c0 -- rows are per region, so chunks need no merging -- and the
// stream is waited for: the staging buffers and the workspace are written again by the next chunk.
template <typename Body>
static int run_region_chunks(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, int64_t nq, int64_t step, Body &&body)
{
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    for (int64_t c0 = 0; c0 < nq; c0 += step) {
        const int64_t m = nq - c0 < step ? nq - c0 : step;
        int rc = stage_queries(db, ichr, qs, qe, c0, m);
        if (rc == IGD_HIP_OK) rc = body(c0, m, st);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
    }
    return IGD_HIP_OK;
}

// [a0, b0) of a staged array cut into slices of row `row`, at most `len` regions each, positions relative to `base`
static void push_slices(std::vector<SetSlice> &slices, int32_t row, int64_t a0, int64_t b0, int64_t len, int64_t base)
{
    for (int64_t a = a0; a < b0; a += len)
        slices.push_back(SetSlice{row, (int32_t)(a - base), (int32_t)((a + len < b0 ? a + len : b0) - base), 0});
}

// The image a slice kernel (walk_query_tiles, sets_dev.hpp) reads: the re-tiled copy when there is one, with the rule word its
// grouping kernels get (rule FLAT over the copy's tiles, bit 8 = rule NEST on the FILE's tiles; search_dev_impl); and whether
// `value >= v` is tested at all (gType 0 has no value field).
struct SliceImage { const DbView &view; int krule; bool useV; };
static SliceImage slice_image(const igd_hip_db *db, int rule, int32_t v)
{
    return SliceImage{(db->inner ? db->inner : db)->v,
                      db->inner ? (IGD_HIP_RULE_FLAT | (rule == IGD_HIP_RULE_NEST ? 0x100 : 0)) : rule,
                      v != IGD_HIP_NO_VALUE_FILTER && db->gType == 1};
}

// nsets sets as offsets into the query arrays: set_off[0] == 0, non-decreasing, arrays present where there are queries
static int sets_check(const char *who, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets)
{
    if (nsets < 0 || (nsets > 0 && !set_off)) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return IGD_HIP_ERR_ARG;
    }
    if (nsets > 0 && set_off[0] != 0) {
        snprintf(g_err, sizeof g_err, "%s: set_off[0] = %lld, not 0", who, (long long)set_off[0]);
        return IGD_HIP_ERR_ARG;
    }
    for (int32_t k = 0; k < nsets; k++)
        if (set_off[k + 1] < set_off[k]) {
            snprintf(g_err, sizeof g_err, "%s: set_off decreases at set %d", who, (int)k);
            return IGD_HIP_ERR_ARG;
        }
    if (nsets > 0 && set_off[nsets] > 0 && (!ichr || !qs || !qe)) {
        snprintf(g_err, sizeof g_err, "%s: bad argument", who);
        return IGD_HIP_ERR_ARG;
    }
    return IGD_HIP_OK;
}

// wide forms (per-wave stripes in global memory): as many workgroups as `budget` bytes of stripes allow, 1 .. IGD_SETS_GRID
static int64_t wide_grid(int64_t budget, int64_t bytesPerWorkgroup)
{
    const int64_t g = budget / bytesPerWorkgroup;
    return g < 1 ? 1 : g < IGD_SETS_GRID ? g : IGD_SETS_GRID;
}

// workgroups for n items, `per` of them per workgroup, 1 .. IGD_SETS_GRID: the grid takes a second round only past that
// (igd_hip_member_grid, igd_hip_fisher_grid: one item per wave; igd_hip_restrict_grid, igd_hip_permute_grid: one per lane)
static int32_t items_grid(int64_t n, int64_t per)
{
    const int64_t g = (n + per - 1) / per;
    return (int32_t)(g < 1 ? 1 : g < IGD_SETS_GRID ? g : IGD_SETS_GRID);
}

// f(A, B) with the two flags as std::true_type / std::false_type, so that a launch kernel<A(), B()><<<...>>> is written once
template <typename F>
static void with_flags(bool a, bool b, F &&f)
{
    if (a && b) f(std::true_type{}, std::true_type{});
    else if (a) f(std::true_type{}, std::false_type{});
    else if (b) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

// The chunk driver.  The sets are taken in CHUNKS: contiguous runs of sets whose queries fit one engine batch
// (igd_hip_max_batch()) and whose device rows fit sets_row_bytes().  A set may be cut at a chunk's end: its row is a sum over
// queries, and the rest of the set opens the next chunk; a query never is.  Per chunk: the queries go to the device once; the
// part of every set of fewer than bigMin queries is cut into slices of sliceLen (row, first, last query within the chunk);
// prepare(m, rows, nSlices) sees to the caller's own workspace; launch(ns, grid) counts the slices into the zeroed d_setRows /
// d_setTot; big(row, a, b) counts queries [a, b) of the chunk, part of a larger set, into row `row`; then the chunk's rows and
// totals come back and are ADDED to hits[nsets][ncols] and, when given, totals[nsets].  ncols is the row width: nFiles for the
// dataset tables, the number of groups for igd_hip_group_support_sets.
template <typename Prepare, typename Launch, typename Big>
static int run_set_chunks(igd_hip_db *db, const int32_t *ichr, const int32_t *qs, const int32_t *qe, const int64_t *set_off, int32_t nsets,
                          int64_t ncols, int64_t sliceLen, int64_t maxGrid, int64_t bigMin, int64_t *hits, int64_t *totals, Prepare &&prepare,
                          Launch &&launch, Big &&big)
{
    const int64_t nF = ncols, step = max_batch();
    const int64_t rowCap = sets_row_bytes() / (nF * 8) > 0 ? sets_row_bytes() / (nF * 8) : 1;
    HIPCHK(hipSetDevice(db->device));
    hipStream_t st = db->stream;
    std::vector<SetSlice> slices;
    std::vector<int64_t> hrows, htot;
    struct BigPart { int32_t row; int64_t a, b; };
    std::vector<BigPart> bigs;
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
                if (set_off[k + 1] - set_off[k] >= bigMin) bigs.push_back(BigPart{row, pos - c0, end - c0});
                else push_slices(slices, row, pos, end, sliceLen, c0);
            }
            pos = end;
            if (pos < set_off[k + 1]) break;             // the batch is full: the rest of set k opens the next chunk
            k++;
        }
        const int64_t m = pos - c0;
        if (m == 0) continue;                            // (only empty sets: their rows stay as they are)
        const int ns = (int)slices.size();
        int rc = sets_ws(db, rows * nF, rows, (int64_t)ns);
        if (rc == IGD_HIP_OK) rc = prepare(m, rows, ns);
        if (rc == IGD_HIP_OK) rc = stage_queries(db, ichr, qs, qe, c0, m);
        if (rc != IGD_HIP_OK) return rc;
        HIPCHK(hipMemsetAsync(db->d_setRows, 0, (size_t)(rows * nF) * 8, st));
        HIPCHK(hipMemsetAsync(db->d_setTot, 0, (size_t)rows * 8, st));
        if (ns) {
            HIPCHK(hipMemcpyAsync(db->d_setSlices, slices.data(), slices.size() * sizeof(SetSlice), hipMemcpyHostToDevice, st));
            if ((rc = launch(ns, ns < maxGrid ? ns : (int)maxGrid)) != IGD_HIP_OK) return rc;
            HIPCHK(hipGetLastError());
        }
        for (const BigPart &b : bigs)
            if ((rc = big(b.row, b.a, b.b)) != IGD_HIP_OK) return rc;
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
static int no_big_sets(int32_t, int64_t, int64_t) { return IGD_HIP_OK; }     // (bigMin = INT64_MAX: never called)
