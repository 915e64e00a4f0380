// engine/coverage_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_sets_coverage: covered base pairs of many query sets in one launch (igd_hip_coverage_sets), one row per set
// ------------------------------------------------------------------------------------------
// coverage[k][f] = sum over the queries q of set k of | [qs, qe) n union of the records of file f that q counts |  (bp; an
// interval union per query, not a sum over records), covered[k] = the same for the union over all files.  The work is cut
// and walked as in igd_sets_support (support_dev.hpp): slices of at most one set, persistent workgroups of four waves
// striding over the slice table, each wave owning whole queries with all their tiles (query_span, the same rule word), every
// tile walked forward from its first record, 2 x 64 records per iteration with all loads issued together, the same predicate
//       lob <= start < qe  &&  end > qs  [&& value >= v]  &&  idx < nFiles
// and the same early exit.  The walk meets a query's counted records in NON-DECREASING START ORDER: a tile is sorted by
// start, a later tile skips start < lob, and every record of an earlier tile starts before lob.  So one frontier per (query,
// file) gives the exact union: a hit with the clipped interval [lo, hi) = [max(start, qs), min(end, qe)) adds
// max(0, hi - max(lo, front)) and raises front to max(front, hi).  (All the records met so far start at or before lo, so
// what they cover from lo on is exactly [lo, front).)  lo and hi lie in [qs, qe]; their differences are taken unsigned.
//   frontier one 64-bit word per file, PRIVATE to the wave: low half = front, high half = tag, the number of the wave's
//            query that wrote it.  A word with another tag is "no hit yet under this query" -- no clearing pass.  Tags start
//            at tag0 + 1 and rise by one per query; the LDS form starts from zeroed words and tag0 = 0.
//   order    the frontier is exact only if the hits of one file are applied in start order, so the lanes of one iteration
//            that hit the SAME file must be applied in lane order, records 0..63 before 64..127.  Detection: every hit lane
//            reads its file's word, stores its lane number (+ 64 for the second half) over the word's low half and reads it
//            back; a lane that reads another number has company.  (The wave's accesses to one address are performed in
//            program order; every word stored over is written again below.)
//            no lane has company (the common case): plain read-modify-write per lane, no atomics on the frontier.
//            otherwise: a leader loop over the files with company.  The lanes of one file take an in-wave prefix maximum
//            of hi (DPP) in lane order, first half before second, starting from the file's frontier; each adds what it
//            covers beyond the maximum before it, and they store the new frontier.  The other lanes take the plain path.
//   any file one frontier per query in a scalar register; per half-step an in-wave exclusive prefix maximum of hi over the
//            hit lanes; each hit lane adds max(0, hi - max(lo, prefix, frontier)) to a 64-bit sum of its own, reduced over
//            the wave at the end of the slice: one global atomic per slice into covered[row] (LDS form; per wave otherwise).
//   counters one 64-bit LDS counter per file, shared by the workgroup's waves (ds_add_u64), flushed at the end of each
//            slice with device-scope atomic adds of the non-zero ones into row k and cleared, as in igd_sets_count.
//            (32 bits would not do: a slice holds up to 4096 queries of up to 2^32 - 1 bp.)
// LDS per workgroup: 8 bytes per file of counters + 4 waves x 8 bytes per file of frontiers = 40 bytes per file, + 16 bytes.
// IGD_COVERAGE_LDS_FILES = 2040 files are 81 616 B: two workgroups (8 waves) fit the 160 KiB of a CU.  The 1 900 files of
// the benchmark database are 76 016 B: 2 workgroups per CU are resident (igd_sets_support: 8), which is what bounds this
// kernel's occupancy -- registers do not.  A workgroup of fewer waves would not help: the frontiers are per wave.
// A database with more files (LDS = false) keeps the frontier words in global memory instead: `gfront`, one stripe of
// nFiles words per wave of the grid, and adds straight into the row with global atomics.  The stripes are never cleared
// between launches: the host hands out rising tag0 values (host_coverage.hpp) and zeroes the stripes before the tags wrap.
typedef __attribute__((address_space(3))) unsigned igd_lds_u32c;

#define IGD_COVERAGE_LDS_FILES 2040                  // 40 bytes of LDS per file: 2 workgroups per CU

#ifdef IGD_COVERAGE_PROBE
__device__ unsigned long long g_covProbe[2];         // iterations with a hit, iterations that took the ordered path
#endif

// inclusive prefix maximum over the 64 lanes (the pattern of wave_inclusive_sum; lanes without a source keep INT_MIN)
__device__ __forceinline__ int wave_inclusive_max(int v)
{
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1 and 3
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2 and 3
    return v;
}
// the value of the lane before (lane 0: INT_MIN): turns an inclusive prefix into an exclusive one
__device__ __forceinline__ int wave_prev_lane(int v, int lane)
{
    const int p = __builtin_amdgcn_ds_bpermute(((lane - 1) & 63) << 2, v);
    return lane ? p : INT_MIN;
}

// the wave's frontier words: LDS (fl) or its global stripe (fg).  volatile: every access below is performed, in order.
template <bool LDS>
__device__ __forceinline__ u64 cov_word(igd_lds_u64 *fl, u64 *fg, int x)
{
    if (LDS) return *(volatile igd_lds_u64 *)(fl + x);
    return *(volatile u64 *)(fg + x);
}
template <bool LDS>
__device__ __forceinline__ void cov_set_word(igd_lds_u64 *fl, u64 *fg, int x, unsigned tag, int front)
{
    const u64 w = ((u64)tag << 32) | (u64)(unsigned)front;
    if (LDS) *(volatile igd_lds_u64 *)(fl + x) = w;
    else *(volatile u64 *)(fg + x) = w;
}
// the low half of a word alone: a hit lane's number goes in, and whichever lane's store came last comes out
template <bool LDS>
__device__ __forceinline__ void cov_mark(igd_lds_u64 *fl, u64 *fg, int x, unsigned who)
{
    if (LDS) *(volatile igd_lds_u32c *)(fl + x) = who;
    else *(volatile unsigned *)(fg + x) = who;
}
template <bool LDS>
__device__ __forceinline__ unsigned cov_marked(igd_lds_u64 *fl, u64 *fg, int x)
{
    if (LDS) return *(volatile igd_lds_u32c *)(fl + x);
    return *(volatile unsigned *)(fg + x);
}
template <bool LDS>
__device__ __forceinline__ void cov_add(igd_lds_u64 *cnt, u64 *row, int x, unsigned bp)
{
    if (LDS) (void)__hip_atomic_fetch_add(cnt + x, (u64)bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(row + x, (u64)bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// what [lo, hi) covers beyond `from` (lo <= hi, all three in [qs, qe] or from = INT_MIN: the difference fits 32 bits unsigned)
__device__ __forceinline__ unsigned cov_beyond(int lo, int hi, int from)
{
    const int m = lo > from ? lo : from;
    return hi > m ? (unsigned)hi - (unsigned)m : 0u;
}

template <bool USE_V, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_sets_coverage(DbView db, const int32_t *__restrict__ q_ichr,
                                                                const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                                const SetSlice *__restrict__ slices, int nSlices, int rule, int v,
                                                                u64 *__restrict__ rows, u64 *__restrict__ covered, u64 *gfront, unsigned tag0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    // LDS: [0] the slice's bp under any file, [2 ..) counters[nF], then the four waves' frontier words[nF]  (all 64-bit)
    igd_lds_u64 *lcov = (igd_lds_u64 *)smem;
    igd_lds_u64 *cnt = lcov + 2;
    igd_lds_u64 *fl = cnt + (size_t)nF * (size_t)(1 + wave);
    u64 *fg = LDS ? nullptr : gfront + ((size_t)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + (size_t)wave) * (size_t)nF;
    if (LDS) {
        for (int f = threadIdx.x; f < 2 + nF * (1 + IGD_SETS_WG / IGD_WAVE); f += IGD_SETS_WG) lcov[f] = 0;
        __syncthreads();
    }
    unsigned tag = tag0;                                                 // the number of this wave's current query
    for (int s = blockIdx.x; s < nSlices; s += gridDim.x) {
        const SetSlice sl = slices[s];
        u64 *row = rows + (size_t)sl.row * (size_t)nF;
        u64 mine = 0;                                                    // this lane's bp under any file, over the slice
        for (int q = sl.a + wave; q < sl.b; q += IGD_SETS_WG / IGD_WAVE) {
            const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
            const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
            const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
            int gt0, ntl;
            if (!query_span(db, cc, qs, qe, rule, gt0, ntl)) continue;
            gt0 = __builtin_amdgcn_readfirstlane(gt0);
            ntl = __builtin_amdgcn_readfirstlane(ntl);
            tag++;
            int allFront = INT_MIN;                                      // covered up to here under this query, any file
            walk_query_tiles<USE_V, false>(db, lane, nF, qs, qe, gt0, ntl, v, 0, MinOv{0, 0, 0}, [&](int s0, int e0, int x0, bool h0, int s1, int e1, int x1, bool h1) {
                const u64 b0 = __ballot(h0), b1 = __ballot(h1);
                if (b0 | b1) {                                       // (wave-uniform: every lane goes the same way below)
                    const int lo0 = s0 > qs ? s0 : qs, hi0 = e0 < qe ? e0 : qe;
                    const int lo1 = s1 > qs ? s1 : qs, hi1 = e1 < qe ? e1 : qe;
                    // any file: exclusive prefix maximum of hi in lane order, first half before second
                    {
                        const int in0 = wave_inclusive_max(h0 ? hi0 : INT_MIN);
                        const int ex0 = wave_prev_lane(in0, lane);
                        mine += h0 ? cov_beyond(lo0, hi0, ex0 > allFront ? ex0 : allFront) : 0u;
                        const int top0 = __builtin_amdgcn_readlane(in0, 63);
                        allFront = top0 > allFront ? top0 : allFront;
                        if (b1) {
                            const int in1 = wave_inclusive_max(h1 ? hi1 : INT_MIN);
                            const int ex1 = wave_prev_lane(in1, lane);
                            mine += h1 ? cov_beyond(lo1, hi1, ex1 > allFront ? ex1 : allFront) : 0u;
                            const int top1 = __builtin_amdgcn_readlane(in1, 63);
                            allFront = top1 > allFront ? top1 : allFront;
                        }
                    }
                    // per file: the words as they are, then who else is here
                    u64 w0 = 0, w1 = 0;
                    unsigned r0 = (unsigned)lane, r1 = (unsigned)lane + 64u;
                    if (h0) w0 = cov_word<LDS>(fl, fg, x0);
                    if (h1) w1 = cov_word<LDS>(fl, fg, x1);
                    if (h0) cov_mark<LDS>(fl, fg, x0, (unsigned)lane);
                    if (h1) cov_mark<LDS>(fl, fg, x1, (unsigned)lane + 64u);
                    if (h0) r0 = cov_marked<LDS>(fl, fg, x0);
                    if (h1) r1 = cov_marked<LDS>(fl, fg, x1);
                    // a word of another query is no frontier
                    const int f0 = (unsigned)(w0 >> 32) == tag ? (int)(unsigned)w0 : INT_MIN;
                    const int f1 = (unsigned)(w1 >> 32) == tag ? (int)(unsigned)w1 : INT_MIN;
                    u64 p0 = __ballot(r0 != (unsigned)lane), p1 = __ballot(r1 != (unsigned)lane + 64u);   // (a lane without a hit kept its own number)
                    bool d0 = false, d1 = false;                     // applied by the ordered path
#ifdef IGD_COVERAGE_PROBE
                    if (lane == 0) {
                        atomicAdd(&g_covProbe[0], 1ull);
                        if (p0 | p1) atomicAdd(&g_covProbe[1], 1ull);
                    }
#endif
                    while (p0 | p1) {                                // ordered path: one file with company per turn
                        const int xf = p0 ? __builtin_amdgcn_readlane(x0, (int)__builtin_ctzll(p0))
                                          : __builtin_amdgcn_readlane(x1, (int)__builtin_ctzll(p1));
                        const bool m0 = h0 & (x0 == xf), m1 = h1 & (x1 == xf);
                        const u64 mb0 = __ballot(m0), mb1 = __ballot(m1);
                        // the file's frontier as any of its lanes read it (all of them before the first store)
                        const int fx = mb0 ? __builtin_amdgcn_readlane(f0, (int)__builtin_ctzll(mb0))
                                           : __builtin_amdgcn_readlane(f1, (int)__builtin_ctzll(mb1));
                        const int in0 = wave_inclusive_max(m0 ? hi0 : INT_MIN);
                        const int ex0 = wave_prev_lane(in0, lane);
                        int top = __builtin_amdgcn_readlane(in0, 63);
                        top = top > fx ? top : fx;
                        const int in1 = wave_inclusive_max(m1 ? hi1 : INT_MIN);
                        const int ex1 = wave_prev_lane(in1, lane);
                        int end = __builtin_amdgcn_readlane(in1, 63);
                        end = end > top ? end : top;
                        if (m0) {
                            const unsigned bp = cov_beyond(lo0, hi0, ex0 > fx ? ex0 : fx);
                            if (bp) cov_add<LDS>(cnt, row, x0, bp);
                            cov_set_word<LDS>(fl, fg, x0, tag, end);   // (every lane of the file stores the same word)
                        }
                        if (m1) {
                            const unsigned bp = cov_beyond(lo1, hi1, ex1 > top ? ex1 : top);
                            if (bp) cov_add<LDS>(cnt, row, x1, bp);
                            cov_set_word<LDS>(fl, fg, x1, tag, end);
                        }
                        d0 |= m0; d1 |= m1;
                        p0 &= ~mb0; p1 &= ~mb1;
                    }
                    if (h0 & !d0) {                                  // alone on its file: plain read-modify-write
                        const unsigned bp = cov_beyond(lo0, hi0, f0);
                        if (bp) cov_add<LDS>(cnt, row, x0, bp);
                        cov_set_word<LDS>(fl, fg, x0, tag, hi0 > f0 ? hi0 : f0);
                    }
                    if (h1 & !d1) {
                        const unsigned bp = cov_beyond(lo1, hi1, f1);
                        if (bp) cov_add<LDS>(cnt, row, x1, bp);
                        cov_set_word<LDS>(fl, fg, x1, tag, hi1 > f1 ? hi1 : f1);
                    }
                }
            });
        }
        // the slice's bp under any file: the lanes' sums meet in lane 0
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, IGD_WAVE);
        if (LDS) {
            if (lane == 0 && mine) (void)__hip_atomic_fetch_add(lcov, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __syncthreads();
            for (int f = threadIdx.x; f < nF; f += IGD_SETS_WG) {
                const u64 c = cnt[f];
                if (c) {
                    (void)__hip_atomic_fetch_add(row + f, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    cnt[f] = 0;
                }
            }
            if (threadIdx.x == 0) {
                const u64 n = lcov[0];
                if (n) {
                    (void)__hip_atomic_fetch_add(covered + sl.row, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    lcov[0] = 0;
                }
            }
            __syncthreads();
        } else if (lane == 0 && mine) {
            (void)__hip_atomic_fetch_add(covered + sl.row, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
