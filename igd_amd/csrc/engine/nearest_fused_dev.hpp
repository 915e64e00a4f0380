// engine/nearest_fused_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_nearest_slices: the set statistics of the nearest record per dataset without the distance rows
// (igd_hip_nearest_sets_fused / igd_hip_permute_nearest; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// igd_hip_nearest_sets writes dist[q][f] to memory (igd_nearest_rows) and reads it back (igd_nearest_reduce): 2 x 4 nFiles
// bytes per region for three numbers per (set, file).  Here the row never leaves the CU.  The shape is sets_support_body's
// (support_dev.hpp): 256 threads, persistent workgroups striding over a SetSlice table, slice = (row k of the matrices,
// regions [a, b)) of one set or one permutation, at most IGD_SETS_SLICE_MAX regions; wave w takes regions a + w, a + w + 4, ..
// Per region it is igd_nearest_rows<USE_V, true>, word for word: igd_hip_nearest_widen, query_span under the caller's rule
// word (FLAT on slice_image), walk_query_tiles<USE_V, false> over the widened interval, d from the TRUE qs, qe
// (igd_hip_nearest_dist), an unsigned minimum into the wave's table.
//
// LDS per workgroup (nF files, nC = nF + 1 columns):
//   sum[nC]     64-bit, shared by the four waves: sum_dist of the slice so far.  A slice of 4 096 regions at distance 2^30 sums
//               to 2^42: 32 bits are not enough.  ds_add_u64, nothing returned.
//   table[4][nF] one table of nF words per wave, PRIVATE to the wave, 0xffffffff = none (nearest_dev.hpp's).  ds_min_u32,
//               nothing returned.
//   cnt[nC]     32-bit, shared: n_within in the low 16 bits, n_overlap in the high 16, raised with ONE ds_add_u32 of
//               1 | (x == 0) << 16.  A region adds at most 1 to either half per column and a slice holds at most
//               IGD_SETS_SLICE_MAX = 4 096 regions (< 65 536: static_assert in host_permute_nearest.hpp), so neither half
//               carries between two flushes.
//   fold        After a region with a counted record (wave-uniform: the ballots) the wave reads its table lane-strided,
//               stores 0xffffffff back over what it read, and for every word x != none adds to cnt[f] and (x != 0) to sum[f];
//               the wave-wide unsigned minimum of the row feeds column nF the same way, by lane 0.  A region without a
//               counted record touches nothing: its table is all "none" already and it adds 0 to every statistic.
//   order       nearest_dev.hpp's argument, for the new accesses: a wave's table is touched by that wave only, and a wave's LDS
//               operations are executed by the LDS unit in the order they were issued -- the minima of the region, then the
//               reads of the fold, then the resets, then the next region's minima; the wave-scope fences keep the compiler
//               from moving them across each other.  cnt[] and sum[] ARE shared by the four waves, hence LDS atomics there;
//               integer adds commute, so the order in which the waves arrive does not matter.  They are read with plain loads
//               only between the two workgroup barriers of the flush, when no wave is adding.
//   flush       After the last region of a slice: barrier; the threads stride over the nC columns and issue one device-scope
//               64-bit atomic add (nothing returned) per NON-ZERO statistic into the three matrices int64[rows][nC] --
//               igd_nearest_reduce's layout: stat, + matWords, + 2 matWords -- and clear the column; barrier.  Slices of one
//               row may run on several CUs at once; everything is an integer, so arrival order does not matter.
//   bound       28 B per file and workgroup (8 + 4 per column, 16 per file of tables) + 12 B: 52 KiB at 1 900 files, where a CU's
//               160 KiB hold three workgroups.  IGD_NEAREST_FUSED_LDS_FILES = 2 920: 28 x 2 920 + 12 = 81 772 B <= 81 920 B =
//               half of 163 840 B, so TWO workgroups per CU stay resident at the limit, as nearest_dev.hpp argues for its
//               own: the walk is bound by its loads' latency and two workgroups overlap each other's -- arithmetic, not a
//               measurement.  There is no wide form: above the limit the host takes igd_nearest_rows + igd_nearest_reduce.
// All stores to memory are vector stores or vector atomics.
#define IGD_NEAREST_FUSED_LDS_FILES 2920             // 28 B per file + 12 B <= 80 KiB: two workgroups per CU stay resident
#define IGD_NEAREST_FUSED_LDS_BYTES(nF) ((size_t)(nF) * 28 + 12)

template <bool USE_V>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_nearest_slices(DbView db, const int32_t *__restrict__ q_ichr,
                                                                 const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                                 const SetSlice *__restrict__ slices, int nSlices, int window, int krule,
                                                                 int v, u64 *__restrict__ stat, int64_t matWords)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles, nC = nF + 1;
    igd_lds_u64 *sum = (igd_lds_u64 *)smem;                              // [nC]
    igd_lds_u32 *tabs = (igd_lds_u32 *)(sum + nC);                       // [4][nF]
    igd_lds_u32 *cnt = tabs + (IGD_SETS_WG / IGD_WAVE) * nF;             // [nC]
    igd_lds_u32 *tb = tabs + wave * nF;                                  // this wave's table
    for (int f = threadIdx.x; f < nC; f += IGD_SETS_WG) { sum[f] = 0; cnt[f] = 0; }
    for (int f = threadIdx.x; f < (IGD_SETS_WG / IGD_WAVE) * nF; f += IGD_SETS_WG) tabs[f] = IGD_NEAREST_NONE;
    __syncthreads();
    for (int s = blockIdx.x; s < nSlices; s += gridDim.x) {
        const SetSlice sl = slices[s];
        for (int q = sl.a + wave; q < sl.b; q += IGD_SETS_WG / IGD_WAVE) {
            const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
            const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
            const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
            int ws, we;
            igd_hip_nearest_widen(qs, qe, window, &ws, &we);
            int gt0 = 0, ntl = 0;
            if (!query_span(db, cc, ws, we, krule, gt0, ntl)) continue;
            gt0 = __builtin_amdgcn_readfirstlane(gt0);
            ntl = __builtin_amdgcn_readfirstlane(ntl);
            u64 any = 0;
            walk_query_tiles<USE_V, false>(db, lane, nF, ws, we, gt0, ntl, v, 0, MinOv{0, 0, 0}, [&](int s0, int e0, int x0, bool h0, int s1, int e1, int x1, bool h1) {
                // (a lane without a counted record computes a d nobody reads)
                const unsigned d0 = (unsigned)igd_hip_nearest_dist(qs, qe, s0, e0), d1 = (unsigned)igd_hip_nearest_dist(qs, qe, s1, e1);
                if (h0) (void)__hip_atomic_fetch_min(tb + x0, d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h1) (void)__hip_atomic_fetch_min(tb + x1, d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                any |= __ballot(h0) | __ballot(h1);
            });
            if (!any) continue;
            // the region's minima, then the reads of the row, then the resets, then the next region's minima: one wave, one
            // LDS unit, program order (see the head of this file)
            unsigned m = IGD_NEAREST_NONE;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int w = lane; w < nF; w += IGD_WAVE) {
                const unsigned x = __hip_atomic_load(tb + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(tb + w, IGD_NEAREST_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (x != IGD_NEAREST_NONE) {
                    (void)__hip_atomic_fetch_add(cnt + w, x == 0 ? 0x10001u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (x) (void)__hip_atomic_fetch_add(sum + w, (u64)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                m = x < m ? x : m;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned y = (unsigned)__shfl_xor((int)m, o);
                m = y < m ? y : m;
            }
            if (lane == 0) {                                             // (any != 0: m is a distance)
                (void)__hip_atomic_fetch_add(cnt + nF, m == 0 ? 0x10001u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (m) (void)__hip_atomic_fetch_add(sum + nF, (u64)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        u64 *dst = stat + (size_t)sl.row * (size_t)nC;
        for (int f = threadIdx.x; f < nC; f += IGD_SETS_WG) {
            const unsigned c = cnt[f];
            if (c) {                                                     // (sum[f] != 0 implies n_within != 0)
                const u64 sd = sum[f];
                (void)__hip_atomic_fetch_add(dst + f, (u64)(c & 0xffffu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (c >> 16) (void)__hip_atomic_fetch_add(dst + matWords + f, (u64)(c >> 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (sd) (void)__hip_atomic_fetch_add(dst + 2 * matWords + f, sd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                cnt[f] = 0;
                sum[f] = 0;
            }
        }
        __syncthreads();
    }
}
