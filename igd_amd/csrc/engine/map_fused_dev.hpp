// engine/map_fused_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_map_slices: the set statistics of the overlapping records' values per dataset without the count and agg rows
// (igd_hip_map_sets_fused / igd_hip_permute_map; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// igd_hip_map_sets writes count[q][f] and agg[q][f] to memory (igd_map_rows) and reads them back (igd_map_reduce): 2 x 12 nFiles
// bytes per region for three numbers per (set, file).  Here the rows never leave the CU: this kernel is to igd_map_rows (LDS
// form) + igd_map_reduce what igd_nearest_slices (nearest_fused_dev.hpp) is to igd_nearest_rows + igd_nearest_reduce.  The shape
// is igd_nearest_slices': 256 threads, persistent workgroups striding over a SetSlice table, slice = (row k of the matrices,
// regions [a, b)) of one set or one permutation, at most IGD_SETS_SLICE_MAX regions; wave w takes regions a + w, a + w + 4, ..
// Per region it is igd_map_rows<USE_V, OP, true>, word for word: igd_hip_nearest_widen(qs, qe, 0), query_span under the caller's
// rule word (FLAT on slice_image), walk_query_tiles<USE_V, false, true, OP != COUNT> over the interval -- every record met once,
// value >= v where the image filters -- and per counted record 1 added to count[idx] and its value folded into agg[idx] of the
// wave's table.
//
// LDS per workgroup (nF files), the 64-bit arrays first so that each is 8-byte aligned for any nF:
//   pairs[nF]    64-bit, shared by the four waves: the counted records of the slice so far.  ds_add_u64, nothing returned.
//   agg_sum[nF]  64-bit, shared: the sum over the slice's regions of the region's aggregate, sign-extended, modulo 2^64.
//                ds_add_u64, nothing returned.  Op COUNT has none: its agg_sum IS pairs, written twice by the flush.
//   n_hit[nF]    32-bit, shared: the regions of the slice with a counted record; a slice holds at most IGD_SETS_SLICE_MAX = 4 096
//                regions.  ds_add_u32, nothing returned.
//   tables       per wave one table PRIVATE to the wave, map_dev.hpp's: u32 count[nF] and, by op, i32 agg[nF] (MIN: INT32_MAX,
//                MAX: INT32_MIN when empty) or u64 agg[nF] (SUM, 0 when empty).  ds_add_u32; ds_min_i32 / ds_max_i32; ds_add_u64;
//                nothing returned.
//   fold         After a region with a counted record (wave-uniform: the ballots) the wave reads its table lane-strided and,
//                for every file with count > 0, stores the empty values back over what it read (a cell with count 0 holds them
//                already: agg is folded only where count is raised) and adds 1 to n_hit[f], count to pairs[f], agg to
//                agg_sum[f].  A region without a counted record touches nothing: its table is empty and it adds 0 everywhere.
//   order        nearest_fused_dev.hpp's argument: a wave's table is touched by that wave only, and a wave's LDS operations are
//                executed by the LDS unit in the order they were issued -- the atomics of the region, then the reads of the
//                fold, then the resets, then the next region's atomics; the wave-scope fences keep the compiler from moving
//                them across each other.  n_hit[], pairs[] and agg_sum[] ARE shared by the four waves, hence LDS atomics
//                there; integer adds commute, so the order in which the waves arrive does not matter.  They are read with plain
//                loads only between the two workgroup barriers of the flush, when no wave is adding.
//   flush        After the last region of a slice: barrier; the threads stride over the nF columns and issue one device-scope
//                64-bit atomic add (nothing returned) per NON-ZERO statistic into the three matrices int64[rows][nF] --
//                igd_map_reduce's layout: stat (n_hit), + matWords (pairs), + 2 matWords (agg_sum) -- and clear the column;
//                barrier.  Slices of one row may run on several CUs at once; everything is an integer modulo 2^64, so arrival
//                order does not matter.
//   bound        Per file and workgroup 20 B of shared accumulators (12 under COUNT) and four private tables of 4 (COUNT), 8
//                (MIN, MAX) or 12 B (SUM): 28, 52 and 68 B.  The limit is what ONE workgroup may have, the CU's whole 160 KiB =
//                163 840 B: igd_hip_map_fused_max_files = 163 840 / 28 = 5 851 (COUNT), / 52 = 3 150 (MIN, MAX), / 68 = 2 409
//                (SUM), so that 1 900 files -- the database the project is measured on -- take this kernel under every op.  The
//                occupancy follows from nF: at 1 900 files COUNT needs 53 200 B (three workgroups per CU), MIN / MAX 98 800 B
//                and SUM 129 200 B: ONE workgroup per CU, four waves on a CU that could hold thirty-two, where
//                igd_nearest_slices keeps two workgroups.  The walk is bound by its loads' latency, which a second workgroup
//                would overlap; WHAT THAT OCCUPANCY COSTS HAS NOT BEEN MEASURED.  Above 64 KiB the launch asks for its
//                dynamic LDS (hipFuncSetAttribute, map_fused_launch).  There is no wide form: above the limit the host takes
//                igd_map_rows + igd_map_reduce (host_permute_map.hpp).
// All stores to memory are vector stores or vector atomics.
#define IGD_MAP_FUSED_LDS_LIMIT 163840               // the LDS of one CU, all of which one workgroup may have

// bytes of LDS one file costs a workgroup: the shared accumulators and the four waves' tables
__host__ __device__ constexpr int map_fused_file_bytes(int op)
{
    return (op == IGD_HIP_MAP_COUNT ? 12 : 20) + (IGD_SETS_WG / IGD_WAVE) * map_lds_file_bytes(op);
}
#define IGD_MAP_FUSED_LDS_BYTES(nF, op) ((size_t)(nF) * (size_t)map_fused_file_bytes(op))
__host__ __device__ constexpr int map_fused_max_files(int op) { return IGD_MAP_FUSED_LDS_LIMIT / map_fused_file_bytes(op); }
static_assert(map_fused_max_files(IGD_HIP_MAP_SUM) >= 1900 && map_fused_max_files(IGD_HIP_MAP_MIN) >= 1900 &&
              map_fused_max_files(IGD_HIP_MAP_COUNT) >= 1900, "1 900 files take igd_map_slices under every op");

template <bool USE_V, int OP>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_map_slices(DbView db, const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                             const int32_t *__restrict__ q_qe, const SetSlice *__restrict__ slices,
                                                             int nSlices, int krule, int v, u64 *__restrict__ stat, int64_t matWords)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WAVES = IGD_SETS_WG / IGD_WAVE;
    constexpr bool SUM = OP == IGD_HIP_MAP_SUM, MINMAX = OP == IGD_HIP_MAP_MIN || OP == IGD_HIP_MAP_MAX, AGG = OP != IGD_HIP_MAP_COUNT;
    constexpr int EMPTY = map_agg_empty(OP);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    // the workgroup's LDS: u64 pairs[nF] [AGG: u64 agg_sum[nF]] [SUM: u64 agg[WAVES][nF]] u32 n_hit[nF] [MIN, MAX: i32 agg[WAVES][nF]]
    // u32 count[WAVES][nF]
    igd_lds_u64 *pairs = (igd_lds_u64 *)smem;
    igd_lds_u64 *asum = pairs + (AGG ? nF : 0);                          // (COUNT: never touched)
    igd_lds_u64 *tabs64 = asum + nF;                                     // (SUM only)
    igd_lds_u32 *nhit = (igd_lds_u32 *)(tabs64 + (SUM ? WAVES * nF : 0));
    igd_lds_i32 *tabs32 = (igd_lds_i32 *)(nhit + nF);                    // (MIN, MAX only)
    igd_lds_u32 *tabsc = (igd_lds_u32 *)(tabs32 + (MINMAX ? WAVES * nF : 0));
    igd_lds_u64 *ta64 = tabs64 + (SUM ? wave * nF : 0);                  // this wave's tables
    igd_lds_i32 *ta32 = tabs32 + (MINMAX ? wave * nF : 0);
    igd_lds_u32 *tc = tabsc + wave * nF;
    for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) {
        pairs[f] = 0;
        nhit[f] = 0;
        if (AGG) asum[f] = 0;
    }
    for (int f = threadIdx.x; f < WAVES * nF; f += IGD_SETS_WG) {
        tabsc[f] = 0;
        if (SUM) tabs64[f] = 0;
        if (MINMAX) tabs32[f] = EMPTY;
    }
    __syncthreads();
    for (int s = blockIdx.x; s < nSlices; s += gridDim.x) {
        const SetSlice sl = slices[s];
        for (int q = sl.a + wave; q < sl.b; q += WAVES) {
            const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
            const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
            const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
            int ws, we;
            igd_hip_nearest_widen(qs, qe, 0, &ws, &we);
            int gt0 = 0, ntl = 0;
            if (!query_span(db, cc, ws, we, krule, gt0, ntl)) continue;
            gt0 = __builtin_amdgcn_readfirstlane(gt0);
            ntl = __builtin_amdgcn_readfirstlane(ntl);
            u64 any = 0;
            walk_query_tiles<USE_V, false, true, AGG>(db, lane, nF, ws, we, gt0, ntl, v, 0, MinOv{0, 0, 0},
                                                      [&](int, int, int x0, bool h0, int v0, int, int, int x1, bool h1, int v1) {
                if (h0) (void)__hip_atomic_fetch_add(tc + x0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h1) (void)__hip_atomic_fetch_add(tc + x1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (SUM) {
                    if (h0) (void)__hip_atomic_fetch_add(ta64 + x0, (u64)(int64_t)v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_add(ta64 + x1, (u64)(int64_t)v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (OP == IGD_HIP_MAP_MIN) {
                    if (h0) (void)__hip_atomic_fetch_min(ta32 + x0, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_min(ta32 + x1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (OP == IGD_HIP_MAP_MAX) {
                    if (h0) (void)__hip_atomic_fetch_max(ta32 + x0, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_max(ta32 + x1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                any |= __ballot(h0) | __ballot(h1);
            });
            if (!any) continue;
            // the region's atomics, then the reads of the table, then the resets, then the next region's atomics: one wave, one
            // LDS unit, program order (see the head of this file)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int w = lane; w < nF; w += IGD_WAVE) {
                const unsigned c = __hip_atomic_load(tc + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (c == 0) continue;                                    // (the cell is empty already)
                __hip_atomic_store(tc + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                (void)__hip_atomic_fetch_add(nhit + w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                (void)__hip_atomic_fetch_add(pairs + w, (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (SUM) {
                    const u64 a = __hip_atomic_load(ta64 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(ta64 + w, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (a) (void)__hip_atomic_fetch_add(asum + w, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (MINMAX) {
                    const int a = __hip_atomic_load(ta32 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(ta32 + w, EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (a) (void)__hip_atomic_fetch_add(asum + w, (u64)(int64_t)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        __syncthreads();
        u64 *dst = stat + (size_t)sl.row * (size_t)nF;
        for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) {
            const unsigned h = nhit[f];
            if (h) {                                                     // (pairs[f] != 0 or agg_sum[f] != 0 implies n_hit != 0)
                const u64 np = pairs[f], sa = AGG ? asum[f] : np;
                (void)__hip_atomic_fetch_add(dst + f, (u64)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(dst + matWords + f, np, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (sa) (void)__hip_atomic_fetch_add(dst + 2 * matWords + f, sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                nhit[f] = 0;
                pairs[f] = 0;
                if (AGG) asum[f] = 0;
            }
        }
        __syncthreads();
    }
}
