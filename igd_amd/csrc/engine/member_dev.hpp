// engine/member_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_member_rows: per-query dataset membership (igd_hip_membership / igd_hip_membership_dev), one bit row per query
// ------------------------------------------------------------------------------------------
// member[q][f] = 1 iff at least one record of file f is counted for query q -- the region x dataset matrix whose column sums
// are the support counts (support_dev.hpp builds the same bitmap per wave and throws it away after counting).  Row q is
// nW = ceil(nFiles / 32) words at bits[q * nW ..]; file f is bit f & 31 of word f >> 5; nfiles_hit[q] = popcount of row q;
// nhit += the rows with any bit set.  The walk is igd_sets_support's: persistent workgroups of four waves, each wave owning
// whole queries with all their tiles (query_span, the same rule word), every tile walked forward from its first record,
// two records per lane and step, with the same predicate
//       lob <= start < qe  &&  end > qs  [&& value >= v]  &&  idx < nFiles
// and the same early exit.  There are no sets and no slices here: wave w of the grid takes the queries w, w + waves, ...
// Bits at positions >= nFiles are never set: the predicate holds idx below nFiles.
//
// LDS form (at most IGD_MEMBER_LDS_FILES files): one bitmap of nW words per wave, PRIVATE to the wave.
//   mark     a lane with a hit ORs its bit into word idx >> 5 with an LDS atomic that returns nothing (ds_or_b32): nothing is
//            counted per file, so nobody needs the old word.
//   row      after the query the wave streams its nW words to the row with plain coalesced vector stores, 64 words (256
//            bytes) per step, adds their popcounts across the wave (nfiles_hit[q], one lane stores it) and stores zeros over
//            the words it has read, so the bitmap is all clear when the next query starts.
//   order    one wave only touches its bitmap, and a wave's LDS operations are executed by the LDS unit in the order they were
//            issued.  So the reads of the row come after every OR of the query, and the next query's ORs after the zero
//            stores, without a workgroup barrier between queries; the wave-scope fences keep the compiler from moving the
//            accesses across each other (they cost no instruction).  This is the argument of support_dev.hpp.
//   no hit   A call DEFINES every word of every row.  The LDS form STORES the zeros of a query without a hit (wave-uniform: the
//            ballots, or query_span said no) instead of relying on a memset of the rows before the launch: the memset would
//            write every row once more than needed -- the rows ARE the kernel's traffic, 240 bytes per query at 1 900 files
//            -- and a caller's stream would carry one more operation per call.  Such a query does not read its bitmap at all.
//   bound    IGD_MEMBER_LDS_FILES = 16384 files are 512 words = 2 KiB per wave, 8 KiB + 16 B per workgroup.  The grid's 8
//            workgroups per CU (IGD_SETS_GRID = 2048 on 256 CUs; 32 waves = the 8 per SIMD that 64 VGPRs allow) take 64 KiB of
//            the CU's 160 KiB: all of them stay resident, far above the two per CU asked for (which 80 KiB per workgroup, 640 K
//            files, would still give -- but past a 2 KiB row the kernel only streams rows, and a hit costs the same
//            atomic in either form, so nothing is gained by a larger bitmap while occupancy is lost).
// Wide form (LDS = false, more files): no bitmap.  The rows are zeroed on the stream before the launch (hipMemsetAsync) and
//   a lane with a hit ORs its bit straight into word idx >> 5 of row q with a device-scope atomic that returns nothing
//   (global_atomic_or).  Row q belongs to one wave during the launch.  nfiles_hit comes from igd_member_popc, a small
//   kernel launched behind this one (kernel boundary: no question of which cache a re-read of the row would be served
//   from when two rows share a cache line); it is not launched when the caller wants no nfiles_hit.
// nhit     each wave counts its queries with a hit and stores the count in an LDS word of its own; behind a barrier thread 0
//          adds the four to *nhit: one global atomic per workgroup, at the end.
// All stores to memory are vector stores.
#define IGD_MEMBER_LDS_FILES 16384                   // 8 KiB of bitmaps per workgroup: the grid's 8 workgroups per CU stay resident

template <bool USE_V, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_member_rows(DbView db, const int32_t *__restrict__ q_ichr,
                                                              const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                              int nq, int rule, int v, unsigned *__restrict__ bits,
                                                              int32_t *__restrict__ nfiles_hit, u64 *__restrict__ nhit)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    const int nW = (nF + 31) >> 5;                                       // words of one row
    // LDS: [0 .. 4) the four waves' queries with a hit, [4 ..) the four waves' bitmaps[nW] (LDS form)
    igd_lds_u32 *lhit = (igd_lds_u32 *)smem;
    igd_lds_u32 *bm = lhit + 4 + wave * nW;
    for (int f = threadIdx.x; f < 4 + (LDS ? (IGD_SETS_WG / IGD_WAVE) * nW : 0); f += IGD_SETS_WG) lhit[f] = 0;
    __syncthreads();
    unsigned hitq = 0;                                                   // this wave's queries with a hit
    const int waves = (int)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int q = (int)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; q < nq; q += waves) {
        const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
        const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
        const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
        unsigned *row = bits + (size_t)q * (size_t)nW;
        int gt0 = 0, ntl = 0;
        if (!query_span(db, cc, qs, qe, rule, gt0, ntl)) ntl = 0;        // (an all-zero row, stored below)
        gt0 = __builtin_amdgcn_readfirstlane(gt0);
        ntl = __builtin_amdgcn_readfirstlane(ntl);
        u64 any = 0;
        walk_query_tiles<USE_V, false>(db, lane, nF, qs, qe, gt0, ntl, v, 0, MinOv{0, 0, 0}, [&](int, int, int x0, bool h0, int, int, int x1, bool h1) {
            if (LDS) {
                if (h0) (void)__hip_atomic_fetch_or(bm + (x0 >> 5), 1u << (x0 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h1) (void)__hip_atomic_fetch_or(bm + (x1 >> 5), 1u << (x1 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                if (h0) (void)__hip_atomic_fetch_or(row + (x0 >> 5), 1u << (x0 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (h1) (void)__hip_atomic_fetch_or(row + (x1 >> 5), 1u << (x1 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            any |= __ballot(h0) | __ballot(h1);
        });
        if (any) hitq++;
        if (LDS) {
            if (any) {
                // the query's ORs, then the reads of the row, then the zeros, then the next query's ORs: one wave, one
                // LDS unit, program order (see the head of this file)
                int pc = 0;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                for (int w = lane; w < nW; w += IGD_WAVE) {
                    const unsigned x = __hip_atomic_load(bm + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(bm + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    row[w] = x;
                    pc += __popc(x);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (nfiles_hit) {
                    for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o);
                    if (lane == 0) nfiles_hit[q] = pc;
                }
            } else {
                for (int w = lane; w < nW; w += IGD_WAVE) row[w] = 0u;
                if (nfiles_hit && lane == 0) nfiles_hit[q] = 0;
            }
        }
    }
    if (lane == 0) lhit[wave] = hitq;
    __syncthreads();
    if (threadIdx.x == 0 && nhit) {
        const unsigned n = lhit[0] + lhit[1] + lhit[2] + lhit[3];
        if (n) (void)__hip_atomic_fetch_add(nhit, (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// wide form: nfiles_hit[q] = popcount of row q, one wave per row and step (launched behind igd_member_rows<., false>)
__global__ __launch_bounds__(IGD_SETS_WG) void igd_member_popc(const unsigned *__restrict__ bits, int nq, int nW,
                                                              int32_t *__restrict__ nfiles_hit)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int q = (int)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; q < nq; q += waves) {
        const unsigned *row = bits + (size_t)q * (size_t)nW;
        int pc = 0;
        for (int w = lane; w < nW; w += IGD_WAVE) pc += __popc(row[w]);
        for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o);
        if (lane == 0) nfiles_hit[q] = pc;
    }
}
