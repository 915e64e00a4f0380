// engine/permute_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_permute_regions, igd_perm_stats: the permutation null of region-set support (igd_hip_permute_support)
// ------------------------------------------------------------------------------------------
// igd_permute_regions.  Output t of a launch is region i = t % nq under permutation p0 + t / nq; the generator is the one of
// include/igd_hip.h (igd_hip_perm_base, igd_hip_perm_place: three rounds of mix64, two 64-bit remainders), evaluated per
// output -- no table of offsets is built, the 150 contig lengths stay in the cache.  One output per lane at a time, IGD_SETS_WG
// threads, at most IGD_SETS_GRID persistent workgroups striding over the outputs (t < 2^31: the host cuts).  out_ichr, when
// given, receives the contig numbers once more per permutation: igd_sets_support reads a query's three words by one index.
//
// igd_perm_stats.  nrows rows of ncols 64-bit counts; column ncols - 1 is read from `tot` (one word per row) when tot is
// given -- the nhit totals of igd_sets_support next to its rows of ncols - 1 files.  Workgroup (x, y) owns the 64 columns
// [64 x, 64 x + 64), one per lane, and the rows 4 y + wave, + 4 gridDim.y, ..: a wave's load of a row is 512 contiguous bytes.
// Each lane keeps sum, sum of squares, the rows >= and <= observed, minimum and maximum of its column in registers; waves
// 1..3 hand theirs to wave 0 through LDS (6 x 3 x 64 words = 9 KiB), and wave 0 issues one device-scope 64-bit atomic per
// statistic and column (add, signed min, signed max; nothing returned).  Everything is an integer: the order in which rows
// and workgroups arrive does not matter.  igd_perm_stats_init puts the six arrays into their neutral state first (0, 0, 0,
// 0, INT64_MAX, INT64_MIN).  All stores to memory are vector stores or vector atomics.
#define IGD_PERM_STATS_ROWS_Y 64                      // at most this many row groups (gridDim.y) per launch

__global__ __launch_bounds__(IGD_SETS_WG) void igd_permute_regions(const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                                  const int32_t *__restrict__ q_qe, unsigned nq,
                                                                  const int32_t *__restrict__ ctg_len, int nctg, int mode, u64 seed,
                                                                  u64 p0, unsigned total, int32_t *__restrict__ out_ichr,
                                                                  int32_t *__restrict__ out_qs, int32_t *__restrict__ out_qe)
{
    const unsigned stride = gridDim.x * IGD_SETS_WG;
    for (unsigned t = blockIdx.x * IGD_SETS_WG + threadIdx.x; t < total; t += stride) {
        const unsigned p = t / nq, i = t - p * nq;
        const int32_t c = q_ichr[i];
        int32_t s = q_qs[i], e = q_qe[i];
        igd_hip_perm_place(mode, igd_hip_perm_base(seed, p0 + p), c, (int64_t)i, ctg_len, nctg, &s, &e);
        if (out_ichr) out_ichr[t] = c;
        out_qs[t] = s;
        out_qe[t] = e;
    }
}

// st = the six arrays of ncols words each, in the order sum, sumsq, n_ge, n_le, min, max
__global__ __launch_bounds__(IGD_SETS_WG) void igd_perm_stats_init(long long *__restrict__ st, int64_t ncols)
{
    const int64_t stride = (int64_t)gridDim.x * IGD_SETS_WG;
    for (int64_t i = (int64_t)blockIdx.x * IGD_SETS_WG + threadIdx.x; i < 6 * ncols; i += stride)
        st[i] = i < 4 * ncols ? 0ll : i < 5 * ncols ? LLONG_MAX : LLONG_MIN;
}

__global__ __launch_bounds__(IGD_SETS_WG) void igd_perm_stats(const long long *__restrict__ rows, const long long *__restrict__ tot,
                                                             int64_t nrows, int64_t ncols, const long long *__restrict__ observed,
                                                             long long *__restrict__ st)
{
    __shared__ long long part[6][IGD_SETS_WG / IGD_WAVE - 1][IGD_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6);
    const int64_t col = (int64_t)blockIdx.x * IGD_WAVE + lane;
    const bool live = col < ncols;
    const bool fromTot = tot != nullptr && col == ncols - 1;
    const int64_t ld = tot ? ncols - 1 : ncols;
    const long long obs = live ? observed[col] : 0;
    u64 sum = 0, sq = 0;
    long long ge = 0, le = 0, mn = LLONG_MAX, mx = LLONG_MIN;
    if (live)
        for (int64_t r = (int64_t)blockIdx.y * (IGD_SETS_WG / IGD_WAVE) + wave; r < nrows; r += (int64_t)gridDim.y * (IGD_SETS_WG / IGD_WAVE)) {
            const long long x = fromTot ? tot[r] : rows[r * ld + col];
            sum += (u64)x;
            sq += (u64)x * (u64)x;
            ge += x >= obs;
            le += x <= obs;
            mn = x < mn ? x : mn;
            mx = x > mx ? x : mx;
        }
    if (wave > 0) {
        part[0][wave - 1][lane] = (long long)sum; part[1][wave - 1][lane] = (long long)sq;
        part[2][wave - 1][lane] = ge; part[3][wave - 1][lane] = le;
        part[4][wave - 1][lane] = mn; part[5][wave - 1][lane] = mx;
    }
    __syncthreads();
    if (wave == 0 && live) {
        for (int w = 0; w < IGD_SETS_WG / IGD_WAVE - 1; w++) {
            sum += (u64)part[0][w][lane]; sq += (u64)part[1][w][lane];
            ge += part[2][w][lane]; le += part[3][w][lane];
            const long long a = part[4][w][lane], b = part[5][w][lane];
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        // (a workgroup whose row range is empty -- gridDim.y is cut to the rows -- would add the neutral values: harmless)
        (void)__hip_atomic_fetch_add((u64 *)st + col, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add((u64 *)st + ncols + col, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(st + 2 * ncols + col, ge, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(st + 3 * ncols + col, le, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_min(st + 4 * ncols + col, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(st + 5 * ncols + col, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
