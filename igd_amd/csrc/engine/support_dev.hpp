// engine/support_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_sets_support: support counts of many query sets in one launch (igd_hip_support_sets), one row per set
// ------------------------------------------------------------------------------------------
// support[k][f] = the queries of set k that overlap AT LEAST ONE record of file f (igd_sets_count adds every overlapping
// record: a query under three records of one file counts 3 there and 1 here); nhit[k] = the queries of set k that overlap
// any record at all.  The work is cut and walked as in igd_sets_count (sets_dev.hpp): slices of at most one set, persistent
// workgroups of four waves striding over the slice table, each wave owning whole queries with all their tiles (query_span,
// the same rule word), every tile walked forward from its first record with the same predicate
//       lob <= start < qe  &&  end > qs  [&& value >= v]  &&  idx < nFiles
// and the same early exit.  One wave sees everything a query meets, so "once per (query, file)" is a wave-private question:
//   bitmap   one bit per file, PRIVATE to the wave.  A lane with a hit ORs its bit into word idx >> 5 with an atomic that
//            returns the word as it was (ds_or_rtn_b32); only the lane that finds the bit clear counts the file.  Lanes of
//            one step that hit the same file are serialised by the LDS unit, so exactly one of them sees it clear.  After a
//            query with a hit (wave-uniform: the ballots) the wave stores zeros over its bitmap, 64 words per step; a query
//            without a hit leaves it as it is -- all clear.  One wave only touches the bitmap and its LDS operations are
//            executed in order, so no workgroup barrier stands between queries.
//   counters one 32-bit LDS counter per file, shared by the workgroup's waves (ds_add_u32), flushed at the end of each
//            slice with device-scope atomic adds of the non-zero ones into row k and cleared, as in igd_sets_count.
//            32 bits are enough BY CONSTRUCTION: a slice holds at most IGD_SETS_SLICE_MAX = 4096 queries (host_sets.hpp)
//            and a query adds at most 1 per file, so a counter never exceeds 4096 between two flushes.  (Whoever raises
//            IGD_SETS_SLICE_MAX to 2^32 or lets a counter live across slices has to widen them.)
//   nhit     each wave counts its queries with a hit; the waves' counts meet in one LDS word and thread 0 adds the slice's
//            sum to nhit[row]: one global atomic per slice.
// LDS per workgroup: 4 bytes per file of counters + 4 waves x 1 bit per file of bitmaps = 4.5 bytes per file, + 16 bytes.
// IGD_SUPPORT_LDS_FILES = 8192 files are 36 KiB + 16 B: four workgroups (16 waves) fit the 160 KiB of a CU; the 1 900 files
// of the benchmark database are 8.4 KiB, where the 8 workgroups per CU of the grid are all resident.
// A database with more files (LDS = false) keeps the bitmaps in global memory instead: `gbits`, one stripe of
// ceil(nFiles / 32) words per wave of the grid, device-scope atomic OR with return, the +1 straight into the row with a
// global atomic (the LDS = false form of igd_sets_count), nhit by one atomic per wave and slice.  The stripes are all zero
// when the kernel starts (igd_hip_support_sets zeroes them when it allocates them) and every wave leaves its own all zero.
typedef __attribute__((address_space(3))) unsigned igd_lds_u32;

#define IGD_SUPPORT_LDS_FILES 8192                   // 36 KiB of LDS per workgroup: 4 workgroups per CU

// one lane's hit on file x: set the bit, count the file if this lane set it first
template <bool LDS>
__device__ __forceinline__ void support_mark(igd_lds_u32 *bits, igd_lds_u32 *cnt, unsigned *gbits, u64 *row, int x)
{
    const unsigned bit = 1u << (x & 31);
    if (LDS) {
        const unsigned old = __hip_atomic_fetch_or(bits + (x >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!(old & bit)) (void)__hip_atomic_fetch_add(cnt + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        const unsigned old = __hip_atomic_fetch_or(gbits + (x >> 5), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!(old & bit)) (void)__hip_atomic_fetch_add(row + x, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// OV: the minimum overlap per pair of igd_sets_support_ov, as in sets_count_body (sets_dev.hpp); OV = false is the plain kernel
template <bool USE_V, bool LDS, bool OV>
__device__ __forceinline__ void sets_support_body(const DbView &db, const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                  const int32_t *__restrict__ q_qe, const SetSlice *__restrict__ slices, int nSlices,
                                                  int rule, int v, u64 *__restrict__ rows, u64 *__restrict__ nhit,
                                                  unsigned *__restrict__ gbits, const MinOv mo)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    const int nW = (nF + 31) >> 5;                                       // words of one bitmap
    // LDS: [0] the slice's queries with a hit, [4 ..) counters[nF], then the four waves' bitmaps[nW]
    igd_lds_u32 *lhit = (igd_lds_u32 *)smem;
    igd_lds_u32 *cnt = lhit + 4;
    igd_lds_u32 *bits = cnt + nF + wave * nW;
    unsigned *gb = LDS ? nullptr : gbits + ((size_t)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + (size_t)wave) * (size_t)nW;
    if (LDS) {
        for (int f = threadIdx.x; f < 4 + nF + (IGD_SETS_WG / IGD_WAVE) * nW; f += IGD_SETS_WG) lhit[f] = 0;
        __syncthreads();
    }
    for (int s = blockIdx.x; s < nSlices; s += gridDim.x) {
        const SetSlice sl = slices[s];
        u64 *row = rows + (size_t)sl.row * (size_t)nF;
        unsigned hitq = 0;                                               // this wave's queries of the slice with a hit
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
                if (h0) support_mark<LDS>(bits, cnt, gb, row, x0);
                if (h1) support_mark<LDS>(bits, cnt, gb, row, x1);
                any |= __ballot(h0) | __ballot(h1);
            });
            if (any) {
                // the next query starts from an empty bitmap.  (The ORs above have returned: their values were used.  The
                // stores below and the next query's ORs are the same wave's accesses to the same unit, executed in order.)
                hitq++;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                for (int w = lane; w < nW; w += IGD_WAVE) {
                    if (LDS) __hip_atomic_store(bits + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else __hip_atomic_store(gb + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        }
        if (LDS) {
            if (lane == 0 && hitq) (void)__hip_atomic_fetch_add(lhit, hitq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) {
                const unsigned c = cnt[f];
                if (c) {
                    (void)__hip_atomic_fetch_add(row + f, (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    cnt[f] = 0;
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
        } else if (lane == 0 && hitq) {
            (void)__hip_atomic_fetch_add(nhit + sl.row, (u64)hitq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool USE_V, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_sets_support(DbView db, const int32_t *__restrict__ q_ichr,
                                                               const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                               const SetSlice *__restrict__ slices, int nSlices, int rule, int v,
                                                               u64 *__restrict__ rows, u64 *__restrict__ nhit, unsigned *__restrict__ gbits)
{
    sets_support_body<USE_V, LDS, false>(db, q_ichr, q_qs, q_qe, slices, nSlices, rule, v, rows, nhit, gbits, MinOv{0, 0, 0});
}

// the same walk under a minimum overlap per pair (igd_hip_support_sets_ov, igd_hip_permute_support_ov with an active threshold)
template <bool USE_V, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) __attribute__((amdgpu_num_sgpr(102))) void igd_sets_support_ov(DbView db, const int32_t *__restrict__ q_ichr,
                                                                  const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                                  const SetSlice *__restrict__ slices, int nSlices, int rule, int v,
                                                                  u64 *__restrict__ rows, u64 *__restrict__ nhit,
                                                                  unsigned *__restrict__ gbits, MinOv mo)
{
    sets_support_body<USE_V, LDS, true>(db, q_ichr, q_qs, q_qe, slices, nSlices, rule, v, rows, nhit, gbits, mo);
}
