// engine/restrict_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_restrict_bits, igd_bits_support: query sets restricted to a universe (igd_hip_restrict_sets / igd_hip_enrich_restricted)
// ------------------------------------------------------------------------------------------
// R_k = { u : some region q of set k has ichr_q == u_ichr_u >= 0, u_qs_u < qe_q and u_qe_u > qs_q } -- LOLA's redefineUserSets:
// a set is replaced by the universe regions it overlaps.  Row k of `bits` is nUW = ceil(nu / 32) words; universe region u (the
// CALLER's numbering) is bit u & 31 of word u >> 5.  Once a set is a subset of the universe its support is a sum over universe
// regions, support[k][f] = sum over u in R_k of member[u][f], with member the rows of igd_member_rows for the universe.
//
// igd_restrict_bits (the join).  The host orders the universe regions with ichr >= 0 by (ichr, start) and uploads
//   ustart[], uend[]   the ordered regions
//   pmax[]             per contig the inclusive prefix maximum of uend
//   perm[]             the caller's number of the region at each position
//   cval[nc], cbeg[nc + 1]   the distinct contig numbers, ascending, and where each one's slice starts
//   off[rows + 1]      the first region of each set of the chunk (regions are numbered within the launch)
// One set region per lane; IGD_SETS_WG threads, at most IGD_SETS_GRID persistent workgroups striding over the regions.  A lane
// finds its row by bisection in off[] (the last k with off[k] <= i: empty sets are passed over), its contig's slice by bisection
// in cval[], and in the slice the first position with ustart >= qe.  Every position before it has ustart < qe; walking back
// from there, position p overlaps iff uend[p] > qs, and the walk ends at the first p with pmax[p] <= qs: no region at or
// before p ends behind qs.  So a long region far to the left is reached (pmax stays above qs until it is passed) and a run of
// short ones to the left of the query ends the walk at once.  The compares are the plain int32 ones of the definition: empty
// and inverted regions on either side are not special-cased, regions that touch do not overlap, ichr < 0 overlaps nothing.
// A hit ORs bit perm[p] into row k with a device-scope atomic that returns nothing (global_atomic_or); the rows are zeroed on
// the stream before the launch.  |R_k| comes from igd_member_popc behind the launch (kernel boundary, as for membership).
//
// igd_bits_support (the gather).  Work item = (row k, block of IGD_RESTRICT_BLOCK_WORDS = 256 words of the row = 8 192 universe
// regions), persistent workgroups of four waves striding over the items.  The membership rows at hand are those of the
// universe regions [u0, u1) (one chunk of igd_hip_membership_dev); bits outside that range are masked off.  Each wave loads 64
// consecutive words of the row, one per lane, and visits the non-zero ones (ballot, v_readlane): a wave skips zero words.  For
// each set bit u with nfiles_hit[u] > 0 the lanes load the words of member row u -- lane j takes words j, j + 64, .. -- and
// every set bit of a word adds 1 to the 32-bit LDS counter of its file (ds_add_u32, nothing returned).  At the end of the
// item the non-zero counters go to support[k][f] with device-scope 64-bit atomic adds and are cleared: the flush of
// igd_sets_support.  nhit[k] += the set bits u with nfiles_hit[u] > 0, one global atomic per item.
//   32 bits   are enough BY CONSTRUCTION: an item holds at most 32 x IGD_RESTRICT_BLOCK_WORDS = 8 192 regions (fewer than 2^32),
//             a region adds at most 1 per file, and the counters are flushed at the end of every item.
//   LDS       4 bytes per file + 16 bytes.  IGD_RESTRICT_LDS_FILES = 8 192 files are 32 KiB + 16 B per workgroup: four workgroups
//             (16 waves) fit the 160 KiB of a CU, the bound of igd_sets_support; the 1 900 files of the benchmark database are
//             7.4 KiB, where the 8 workgroups per CU of the grid are all resident.
//   wide      more files (LDS = false): no counters, every set bit adds 1 straight into support[k][f] with a global atomic
//             (the wide forms of igd_sets_count / igd_sets_support).
//   ones row  row number `onesRow` is not read: it stands for a row of all ones -- the whole universe -- and yields usupport
//             and unhit by the same code.
// Bits at positions >= nFiles of a member row are 0 (igd_member_rows), so no counter outside [0, nFiles) is touched.
// All stores to memory are vector stores or vector atomics.
#define IGD_RESTRICT_LDS_FILES 8192                  // 32 KiB of LDS counters per workgroup: 4 workgroups per CU
#define IGD_RESTRICT_BLOCK_WORDS 256                 // words of a bits row per work item: 64 per wave

__global__ __launch_bounds__(IGD_SETS_WG) void igd_restrict_bits(const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                                const int32_t *__restrict__ q_qe, int nreg,
                                                                const int32_t *__restrict__ off, int rows,
                                                                const int32_t *__restrict__ cval, const int32_t *__restrict__ cbeg, int nc,
                                                                const int32_t *__restrict__ ustart, const int32_t *__restrict__ uend,
                                                                const int32_t *__restrict__ pmax, const int32_t *__restrict__ perm,
                                                                int64_t nUW, unsigned *__restrict__ bits)
{
    const int stride = (int)gridDim.x * IGD_SETS_WG;
    for (int i = (int)blockIdx.x * IGD_SETS_WG + (int)threadIdx.x; i < nreg; i += stride) {
        const int c = q_ichr[i], qs = q_qs[i], qe = q_qe[i];
        if (c < 0) continue;
        // the contig's slice of the ordered universe
        int lo = 0, hi = nc;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (cval[m] < c) lo = m + 1; else hi = m; }
        if (lo >= nc || cval[lo] != c) continue;
        const int s0 = cbeg[lo], s1 = cbeg[lo + 1];
        // the first position with ustart >= qe
        int a = s0, b = s1;
        while (a < b) { const int m = a + ((b - a) >> 1); if (ustart[m] < qe) a = m + 1; else b = m; }
        if (a == s0 || pmax[a - 1] <= qs) continue;      // nothing starts before qe, or nothing that does ends behind qs
        // the row: the last k with off[k] <= i
        int k0 = 0, k1 = rows;
        while (k1 - k0 > 1) { const int m = (k0 + k1) >> 1; if (off[m] <= i) k0 = m; else k1 = m; }
        unsigned *row = bits + (size_t)k0 * (size_t)nUW;
        for (int p = a - 1; p >= s0 && pmax[p] > qs; p--)
            if (uend[p] > qs) {
                const int u = perm[p];
                (void)__hip_atomic_fetch_or(row + (u >> 5), 1u << (u & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
    }
}

template <bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_bits_support(const unsigned *__restrict__ bits, int64_t nUW, int rows, int onesRow,
                                                               int64_t u0, int64_t u1, const unsigned *__restrict__ member,
                                                               const int32_t *__restrict__ nfiles_hit, int nF,
                                                               u64 *__restrict__ support, u64 *__restrict__ nhit)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nW = (nF + 31) >> 5;                                       // words of one member row
    // LDS: [0] the item's regions with a hit, [4 ..) counters[nF] (LDS form)
    igd_lds_u32 *lhit = (igd_lds_u32 *)smem;
    igd_lds_u32 *cnt = lhit + 4;
    for (int f = threadIdx.x; f < 4 + (LDS ? nF : 0); f += IGD_SETS_WG) lhit[f] = 0;
    __syncthreads();
    const int64_t w0 = u0 >> 5, w1 = (u1 + 31) >> 5;                     // the words of a row that hold [u0, u1)
    const int64_t nblk = (w1 - w0 + IGD_RESTRICT_BLOCK_WORDS - 1) / IGD_RESTRICT_BLOCK_WORDS;
    const int64_t items = (int64_t)rows * nblk;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int k = (int)(it / nblk);
        const int64_t wb = w0 + (it - (int64_t)k * nblk) * IGD_RESTRICT_BLOCK_WORDS + wave * IGD_WAVE;   // this wave's first word
        const int64_t w = wb + lane;
        unsigned x = 0;
        if (w < w1) {
            x = k == onesRow ? 0xffffffffu : bits[(size_t)k * (size_t)nUW + (size_t)w];
            const int64_t base = w << 5;
            if (base < u0) x &= 0xffffffffu << (int)(u0 - base);         // (1 .. 31: w >= w0)
            if (base + 32 > u1) x &= (1u << (int)(u1 - base)) - 1u;      // (1 .. 31: w < w1)
        }
        u64 *srow = support + (size_t)k * (size_t)nF;
        unsigned hitq = 0;                                               // this wave's regions of the item with a hit
        u64 nz = __ballot(x != 0);
        while (nz) {
            const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(nz));
            nz &= nz - 1;
            unsigned word = (unsigned)__builtin_amdgcn_readlane((int)x, l);
            const int64_t ub = ((wb + l) << 5) - u0;                     // member row of the word's bit 0
            while (word) {
                const int b = __builtin_ctz(word);
                word &= word - 1;
                const int64_t r = ub + b;
                if (__builtin_amdgcn_readfirstlane(nfiles_hit[r]) <= 0) continue;
                hitq++;
                const unsigned *mrow = member + (size_t)r * (size_t)nW;
                for (int j = lane; j < nW; j += IGD_WAVE) {
                    unsigned m = mrow[j];
                    while (m) {
                        const int f = (j << 5) + __builtin_ctz(m);
                        m &= m - 1;
                        if (LDS) (void)__hip_atomic_fetch_add(cnt + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        else (void)__hip_atomic_fetch_add(srow + f, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        }
        if (LDS) {
            if (lane == 0 && hitq) (void)__hip_atomic_fetch_add(lhit, hitq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) {
                const unsigned c = cnt[f];
                if (c) {
                    (void)__hip_atomic_fetch_add(srow + f, (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    cnt[f] = 0;
                }
            }
            if (threadIdx.x == 0) {
                const unsigned n = lhit[0];
                if (n) {
                    (void)__hip_atomic_fetch_add(nhit + k, (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    lhit[0] = 0;
                }
            }
            __syncthreads();
        } else if (lane == 0 && hitq) {
            (void)__hip_atomic_fetch_add(nhit + k, (u64)hitq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
