// engine/group_support_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_sets_group_support: support counts per GROUP of datasets, many query sets in one launch (igd_hip_group_support_sets)
// ------------------------------------------------------------------------------------------
// A grouping is a many-to-many relation dataset -> groups in CSR form: grp_off[nFiles + 1] (non-decreasing from 0) and
// grp_idx[grp_off[nFiles]] (each in [0, nG), strictly ascending within one dataset's run; the host checks all of it before a
// launch, so the kernel indexes LDS with grp_idx unchecked).  With F_q = the datasets igd_sets_support counts for query q:
//       gsupport[k][g] = the queries q of set k for which F_q holds a dataset of group g      (a UNION over the datasets of g:
//                        neither the sum nor the maximum of their supports)
//       gnhit[k]       = the queries q of set k for which F_q holds a dataset with at least one group
// The walk is sets_support_body's in its LDS form (support_dev.hpp): the same slices, persistent workgroups of four waves,
// query_span, walk_query_tiles<USE_V, OV>, the same early exit.  What differs:
//   mark     a lane with a hit on dataset x reads grp_off[x], grp_off[x + 1] and applies support_mark<true> to every
//            grp_idx[j] of that run: atomic OR with return on the wave's bitmap, the counter raised only by the lane that found
//            the bit clear.  Lanes of one step that reach one group through different datasets are serialised by the LDS unit
//            exactly as two lanes on one file are in igd_sets_support.  The loop length differs per lane: a wave pays the
//            longest run of its hit lanes in every step.  That divergence is the cost of the feature.
//   any      the ballot of the lanes that marked at least one group, not of the lanes with a hit: a query that meets only
//            unlabelled datasets leaves the bitmap all clear, is not counted in gnhit and clears nothing.
//   table    grp_off / grp_idx are read through the ordinary cached path from global memory (uploaded once per call, resident
//            for all its chunks; 1 900 datasets with three labels each are 30 KB).  nFiles is not bounded by LDS at all.
// LDS per workgroup: [0] the slice's queries with a marked group (16 bytes with padding), nG 32-bit counters, four bitmaps of
// ceil(nG / 32) words = 4.5 bytes per GROUP + 16 bytes.  IGD_GROUP_LDS_GROUPS = 8192 groups are 36 KiB + 16 B: four workgroups
// (16 waves) fit the 160 KiB of a CU, the figure of IGD_SUPPORT_LDS_FILES.  There is no wide (global-bitmap) form: more
// groups are refused by the host.
// The counters are 32 bits wide and that is enough BY CONSTRUCTION, unchanged from igd_sets_support: a slice holds at most
// IGD_SETS_SLICE_MAX = 4096 queries, a query adds at most 1 per column (the bitmap), and the counters are flushed and cleared
// at the end of every slice.  IGD_GROUP_SLICE_CAP is the longest slice this kernel may be handed; host_group_support.hpp holds
// IGD_SETS_SLICE_MAX, which is defined behind this part, to it.
#define IGD_GROUP_LDS_GROUPS 8192                    // 36 KiB of LDS per workgroup: 4 workgroups per CU
#define IGD_GROUP_SLICE_CAP 4096                     // regions per slice: the most a 32-bit counter is raised between two flushes
static_assert((unsigned long long)IGD_GROUP_SLICE_CAP <= 0xffffffffull, "a slice's regions must fit the 32-bit LDS counters of igd_sets_group_support");
static_assert((4 + IGD_GROUP_LDS_GROUPS + (256 / 64) * (IGD_GROUP_LDS_GROUPS / 32)) * 4 <= 40 * 1024, "four workgroups of igd_sets_group_support per CU");

// one lane's hit on dataset x: every group of x is marked; true if x has any group
__device__ __forceinline__ bool group_mark(igd_lds_u32 *bits, igd_lds_u32 *cnt, const int32_t *__restrict__ grp_off,
                                           const int32_t *__restrict__ grp_idx, int x)
{
    const int j0 = grp_off[x], j1 = grp_off[x + 1];
    for (int j = j0; j < j1; j++) support_mark<true>(bits, cnt, nullptr, nullptr, grp_idx[j]);
    return j1 > j0;
}

// amdgpu_num_sgpr: as igd_sets_support_ov / igd_sets_count_ov (sets_dev.hpp) -- the table's two pointers and, under OV, the
// threshold's scalars come on top of the twins' allocation; capped, the surplus lives in VGPR lanes, not in scratch.
template <bool USE_V, bool OV>
__global__ __launch_bounds__(IGD_SETS_WG) __attribute__((amdgpu_num_sgpr(102))) void igd_sets_group_support(
    DbView db, const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
    const SetSlice *__restrict__ slices, int nSlices, int rule, int v, const int32_t *__restrict__ grp_off,
    const int32_t *__restrict__ grp_idx, int nG, u64 *__restrict__ rows, u64 *__restrict__ nhit, MinOv mo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    const int nW = (nG + 31) >> 5;                                       // words of one bitmap
    // LDS: [0] the slice's queries with a marked group, [4 ..) counters[nG], then the four waves' bitmaps[nW]
    igd_lds_u32 *lhit = (igd_lds_u32 *)smem;
    igd_lds_u32 *cnt = lhit + 4;
    igd_lds_u32 *bits = cnt + nG + wave * nW;
    for (int g = threadIdx.x; g < 4 + nG + (IGD_SETS_WG / IGD_WAVE) * nW; g += IGD_SETS_WG) lhit[g] = 0;
    __syncthreads();
    for (int s = blockIdx.x; s < nSlices; s += gridDim.x) {
        const SetSlice sl = slices[s];
        u64 *row = rows + (size_t)sl.row * (size_t)nG;
        unsigned hitq = 0;                                               // this wave's queries of the slice with a marked group
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
            u64 any = 0;
            walk_query_tiles<USE_V, OV>(db, lane, nF, qs, qe, gt0, ntl, v, need, mo, [&](int, int, int x0, bool h0, int, int, int x1, bool h1) {
                bool m0 = false, m1 = false;
                if (h0) m0 = group_mark(bits, cnt, grp_off, grp_idx, x0);
                if (h1) m1 = group_mark(bits, cnt, grp_off, grp_idx, x1);
                any |= __ballot(m0) | __ballot(m1);
            });
            if (any) {
                // the next query starts from an empty bitmap (the ORs have returned; the stores below and the next query's
                // ORs are the same wave's accesses to the same unit, executed in order: support_dev.hpp)
                hitq++;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                for (int w = lane; w < nW; w += IGD_WAVE) __hip_atomic_store(bits + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        }
        if (lane == 0 && hitq) (void)__hip_atomic_fetch_add(lhit, hitq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        for (int g = threadIdx.x; g < nG; g += IGD_SETS_WG) {
            const unsigned c = cnt[g];
            if (c) {
                (void)__hip_atomic_fetch_add(row + g, (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                cnt[g] = 0;
            }
        }
        if (threadIdx.x == 0) {
            const unsigned n = lhit[0];
            if (n) {
                (void)__hip_atomic_fetch_add(nhit + sl.row, (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                lhit[0] = 0;
            }
        }
        __syncthreads();
    }
}
