// engine/sets_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_sets_count: many small query sets in one launch (igd_hip_search_sets), one hits[] row per set
// ------------------------------------------------------------------------------------------
// The batch pipeline of igd_hip_search_dev adds a whole batch into ONE int64[nFiles] row.  A caller with a thousand sets of
// a thousand queries each would pay that pipeline's launches, copies and sync once per set; here the sets share one launch.
// Work item = slice: (row k, queries [a, b)) of at most one set, cut on the host (host_sets.hpp).  Persistent workgroups of
// four waves stride over the slice table; the waves of a workgroup own different queries of its slice.  Per query its tiles
// come from query_span (the rule word as the grouping kernels get it, re-tiled gate bit included), and each tile is walked
// FORWARD from its first record, 64 records per lane-step, two steps per iteration (all loads of both issued together):
//       lob <= start < qe  &&  end > qs  [&& value >= v]
// with lob = INT_MIN in the query's first tile and the tile's start coordinate in the later ones (the reference's prefix
// skip of records counted in an earlier tile, src/igd_search.c:510-511).  The records of a tile are ordered by start, so
// the walk ends after the first step whose largest start is >= qe -- no bisection, hence no chain of dependent loads.
// Counters: LDS, one 64-bit counter per file (ds_add_u64; cannot overflow), flushed at the end of each slice with device-
// scope atomic adds of the non-zero ones into row k (slices of one set may run on several CUs at once).  A database with
// more files than IGD_SETS_LDS_FILES adds straight into the row with global atomics instead (LDS = false).
struct SetSlice { int32_t row, a, b, pad; };         // 16 bytes: one scalar load per slice

#define IGD_SETS_WG 256                              // threads per workgroup (4 waves)
#define IGD_SETS_LDS_FILES 8192                      // 64-bit counters in 64 KiB of LDS
#define IGD_SETS_GRID 2048                           // persistent workgroups (8 per CU of the MI355X's 256)

// The minimum overlap of the `_ov` kernels (include/igd_hip.h: igd_hip_min_overlap), by value in the kernel arguments.
// OV = false: the fields are never read and the body below is the plain kernel's, instruction for instruction.
// OV = true, per query and wave-uniform: need = igd_hip_min_overlap_need_q -- max(min_bp, 1, ceil(lenq * ppm_query / 10^6)), the
// one 64-bit division of the test -- and a query that no record can satisfy (qe <= qs) is left before its tiles are looked up.
// Per lane: ov = min(qe, end) - max(qs, start) as a 32-bit difference (records have 0 <= start < end), one compare against
// need, and, behind a wave-uniform branch on ppm_record, ov * 10^6 >= (end - start) * ppm_record as two 64-bit products.
struct MinOv { int32_t min_bp, ppm_query, ppm_record; };

__device__ __forceinline__ bool min_ov_pair(int need, int ppmR, int qs, int qe, int s, int e)
{
    const int ov = (int)((unsigned)(qe < e ? qe : e) - (unsigned)(qs > s ? qs : s));
    bool ok = ov >= need;
    if (ppmR) ok = ok & ((int64_t)ov * IGD_HIP_PPM >= (int64_t)(int)((unsigned)e - (unsigned)s) * (int64_t)ppmR);
    return ok;
}

// The forward walk over one query's tiles that igd_sets_count, igd_sets_support, igd_sets_coverage and igd_member_rows share:
// tiles gt0 .. gt0 + ntl - 1 (query_span), each from its first record, 2 x 64 records per iteration with all loads issued
// together, the predicate above with its USE_V (value >= v) and OV (min_ov_pair under `need`, `mo`) terms, then
// step(s0, e0, x0, h0, s1, e1, x1, h1) -- start, end, idx and "counted" of this lane's two records; a lane past the tile's end
// has h = false -- and the early exit.  Everything but `lane` and what step() does per lane is wave-uniform.
// VAL (igd_map_rows): step(s0, e0, x0, h0, v0, s1, e1, x1, h1, v1) also receives the lane's two value words; they are loaded when
// USE_V or LOADV is set and are 0 otherwise.  VAL = LOADV = false is the walk as it was, instruction for instruction.
template <bool USE_V, bool OV, bool VAL = false, bool LOADV = false, typename F>
__device__ __forceinline__ void walk_query_tiles(const DbView &db, int lane, int nF, int qs, int qe, int gt0, int ntl, int v, int need,
                                                 const MinOv &mo, F &&step)
{
    for (int k = 0; k < ntl; k++) {
        const int t = gt0 + k;
        const int tcnt = __builtin_amdgcn_readfirstlane(db.tileCnt[t]);
        if (tcnt == 0) continue;
        const int lob = (k == 0) ? INT_MIN : __builtin_amdgcn_readfirstlane(db.tileBd[t]);
        const int64_t toff = db.tileOff[t];
        for (int i0 = 0; i0 < tcnt; i0 += 2 * IGD_WAVE) {
            const int i = i0 + lane, j = i + IGD_WAVE;
            const bool ok0 = i < tcnt, ok1 = j < tcnt;
            const int s0 = ok0 ? db.start[toff + i] : INT_MAX;
            const int e0 = ok0 ? db.end[toff + i] : INT_MIN;
            const int x0 = ok0 ? db.idx[toff + i] : -1;
            const int s1 = ok1 ? db.start[toff + j] : INT_MAX;
            const int e1 = ok1 ? db.end[toff + j] : INT_MIN;
            const int x1 = ok1 ? db.idx[toff + j] : -1;
            bool h0 = (s0 >= lob) & (s0 < qe) & (e0 > qs) & ((unsigned)x0 < (unsigned)nF);
            bool h1 = (s1 >= lob) & (s1 < qe) & (e1 > qs) & ((unsigned)x1 < (unsigned)nF);
            int v0 = 0, v1 = 0;
            if (USE_V || LOADV) {
                v0 = ok0 ? db.value[toff + i] : INT_MIN;
                v1 = ok1 ? db.value[toff + j] : INT_MIN;
            }
            if (USE_V) {
                h0 = h0 & (v0 >= v);
                h1 = h1 & (v1 >= v);
            }
            if (OV) {
                h0 = h0 & min_ov_pair(need, mo.ppm_record, qs, qe, s0, e0);
                h1 = h1 & min_ov_pair(need, mo.ppm_record, qs, qe, s1, e1);
            }
            if constexpr (VAL) step(s0, e0, x0, h0, v0, s1, e1, x1, h1, v1);
            else step(s0, e0, x0, h0, s1, e1, x1, h1);
            // records are ordered by start: a step whose largest start is >= qe ends the tile
            if (__builtin_amdgcn_readlane(s1, 63) >= qe) break;
        }
    }
}

template <bool USE_V, bool LDS, bool OV>
__device__ __forceinline__ void sets_count_body(const DbView &db, const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                const int32_t *__restrict__ q_qe, const SetSlice *__restrict__ slices, int nSlices,
                                                int rule, int v, u64 *__restrict__ rows, u64 *__restrict__ totals, const MinOv mo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    igd_lds_u64 *cnt = (igd_lds_u64 *)smem;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    if (LDS) {
        for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) cnt[f] = 0;
        __syncthreads();
    }
    for (int s = blockIdx.x; s < nSlices; s += gridDim.x) {
        const SetSlice sl = slices[s];
        u64 *row = rows + (size_t)sl.row * (size_t)nF;
        u64 found = 0;
        for (int q = sl.a + wave; q < sl.b; q += IGD_SETS_WG / IGD_WAVE) {
            const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
            const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
            const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
            int need = 0;
            if (OV) {
                need = __builtin_amdgcn_readfirstlane(igd_hip_min_overlap_need_q(mo.min_bp, mo.ppm_query, qs, qe));
                if (need < 0) continue;
            }
            int gt0, ntl;
            if (!query_span(db, cc, qs, qe, rule, gt0, ntl)) continue;
            gt0 = __builtin_amdgcn_readfirstlane(gt0);
            ntl = __builtin_amdgcn_readfirstlane(ntl);
            walk_query_tiles<USE_V, OV>(db, lane, nF, qs, qe, gt0, ntl, v, need, mo, [&](int, int, int x0, bool h0, int, int, int x1, bool h1) {
                if (LDS) {
                    if (h0) (void)__hip_atomic_fetch_add(cnt + x0, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_add(cnt + x1, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    if (h0) (void)__hip_atomic_fetch_add(row + x0, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h1) (void)__hip_atomic_fetch_add(row + x1, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                found += (u64)__popcll(__ballot(h0)) + (u64)__popcll(__ballot(h1));
            });
        }
        if (lane == 0 && found) (void)__hip_atomic_fetch_add(totals + sl.row, found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (LDS) {
            __syncthreads();
            for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) {
                const u64 c = cnt[f];
                if (c) {
                    (void)__hip_atomic_fetch_add(row + f, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    cnt[f] = 0;
                }
            }
            __syncthreads();
        }
    }
}

template <bool USE_V, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_sets_count(DbView db, const int32_t *__restrict__ q_ichr,
                                                             const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                             const SetSlice *__restrict__ slices, int nSlices, int rule, int v,
                                                             u64 *__restrict__ rows, u64 *__restrict__ totals)
{
    sets_count_body<USE_V, LDS, false>(db, q_ichr, q_qs, q_qe, slices, nSlices, rule, v, rows, totals, MinOv{0, 0, 0});
}

// the same walk under a minimum overlap per pair (igd_hip_search_sets_ov with an active threshold).  amdgpu_num_sgpr: the threshold's
// four scalars push the allocation past the 100 SGPRs that eight waves per SIMD leave each wave (the plain kernels use 94 .. 100);
// capped there, two to six of them live in VGPR lanes (v_writelane / v_readlane, no scratch) and the occupancy stays the twins'.
template <bool USE_V, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) __attribute__((amdgpu_num_sgpr(102))) void igd_sets_count_ov(DbView db, const int32_t *__restrict__ q_ichr,
                                                                const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                                const SetSlice *__restrict__ slices, int nSlices, int rule, int v,
                                                                u64 *__restrict__ rows, u64 *__restrict__ totals, MinOv mo)
{
    sets_count_body<USE_V, LDS, true>(db, q_ichr, q_qs, q_qe, slices, nSlices, rule, v, rows, totals, mo);
}
