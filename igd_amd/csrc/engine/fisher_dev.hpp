// engine/fisher_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_fisher_cells: the one-sided ("greater") Fisher exact test of many 2x2 tables in one launch (host_enrich.hpp)
// ------------------------------------------------------------------------------------------
// A table a b / c d has N = a+b+c+d, K = a+b, n = a+c and X ~ Hypergeometric(N, K, n) on lo = max(0, n - (N - K)) .. hi =
// min(n, K).  The kernel gives pvalue_log = -log10 P(X >= a) and the sample odds ratio (a d) / (b c), all in double.
//   shape    ONE WAVE PER CELL; persistent workgroups of four waves stride over the cells as the waves of igd_sets_support
//            stride over queries.  The cells cost very different amounts (no term at all .. thousands), so a cell is not
//            tied to a lane: the 64 lanes take 64 consecutive support points k of ONE cell per step.
//   term     log P(X = k) = lf(K) + lf(N-K) + lf(n) + lf(N-n) - lf(N) - lf(k) - lf(K-k) - lf(n-k) - lf(N-K-n+k), lf(x) =
//            lgamma(x + 1): nine log-factorials.  The five that do not depend on k are ONE lgamma call of the wave (lane j
//            takes the j-th argument; they are handed round with v_readlane), the other four are four calls per step.
//            The nine are added in pairs of like magnitude -- lf(K) - lf(K-k), lf(N-K) - lf(N-K-n+k), lf(n) - lf(n-k),
//            lf(N-n) - lf(N) -- so that the large ones cancel before anything small is added to them.
//            lgamma is called throughout; there is no log-factorial table (DESIGN.md 4.8 says why).
//   tail     summed from the side on which it decays.  mode = floor((n+1)(K+1) / (N+2)).  a > mode: k = a, a+1, .. hi and
//            log p = t_first + log(sum exp(t_k - t_first)).  Otherwise L = sum over k = a-1, a-2, .. lo the same way and
//            log p = log1p(-L); there p is about a half or more, so nothing cancels.  Away from the mode the terms never
//            rise: the first term is the largest, every lane adds exp(t - t_first) <= 1 to a private sum, and the wave
//            stops after the first step whose largest term (lane 0's) is below t_first - IGD_FISHER_STOP = 45 (e^-45 =
//            3e-20, under a double's resolution of the sum) or that reaches the end of the support.  The lanes' sums meet
//            once per cell in a DPP prefix sum (wave_inclusive_sum_f64: the pattern of wave_inclusive_sum on both halves).
//   +0.0     a == lo (p = 1: the whole support) and N == 0 give exactly +0.0 without a term; a value that rounding leaves
//            below zero is +0.0 too.
//   tables   GENERIC form: four int64 arrays.  ENRICHMENT form: support[nsets x nF], usupport[nF], n_k[nsets] and n_U; the
//            wave forms a, b = u - a, c = n_k - a, d = n_U - a - b - c itself, sets a negative b or d to 0 and counts such
//            cells in clamped[k] (one global atomic of lane 0 per clamped cell).
//   stores   lane 0 stores the cell's two doubles; every cell of the launch is stored: outputs are DEFINED.
// No LDS.  The host checks 0 <= entries and N < 2^31 before a launch (host_enrich.hpp): (n+1)(K+1) fits 63 bits.
#define IGD_FISHER_STOP 45.0
#define IGD_FISHER_LN10 2.302585092994045684

template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_from_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);                     // (lanes without a source read +0.0)
}
// inclusive prefix sum over the 64 lanes (wave_inclusive_sum's steps); lane 63 holds the wave's sum.  Every lane takes part.
__device__ __forceinline__ double wave_inclusive_sum_f64(double v)
{
    v += dpp_from_f64<0x111, 0xf>(v);
    v += dpp_from_f64<0x112, 0xf>(v);
    v += dpp_from_f64<0x114, 0xf>(v);
    v += dpp_from_f64<0x118, 0xf>(v);
    v += dpp_from_f64<0x142, 0xa>(v);                    // row_bcast:15 into rows 1 and 3
    v += dpp_from_f64<0x143, 0xc>(v);                    // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ double wave_lane_f64(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ int64_t wave_uniform_i64(int64_t v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((u64)v & 0xffffffffull));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((u64)v >> 32));
    return (int64_t)(((u64)hi << 32) | (u64)lo);
}

// -log10 P(X >= a) of one table, computed by the whole wave (every lane returns it).  Entries >= 0, N < 2^31.
__device__ __forceinline__ double fisher_wave_cell(int64_t a, int64_t b, int64_t c, int64_t d, int lane)
{
    const int64_t N = a + b + c + d, K = a + b, n = a + c;
    const int64_t lo = a - d > 0 ? a - d : 0, hi = n < K ? n : K;
    if (N == 0 || a <= lo) return 0.0;                   // (wave-uniform)
    const int64_t mode = ((n + 1) * (K + 1)) / (N + 2);
    const bool up = a > mode;
    // the five log-factorials that every term shares: lane 0..4 take lf(K), lf(N-K), lf(n), lf(N-n), lf(N)
    const int64_t x5 = lane == 0 ? K : lane == 1 ? N - K : lane == 2 ? n : lane == 3 ? N - n : lane == 4 ? N : 0;
    const double l5 = lgamma((double)x5 + 1.0);
    const double lfK = wave_lane_f64(l5, 0), lfNK = wave_lane_f64(l5, 1), lfn = wave_lane_f64(l5, 2);
    const double tail5 = wave_lane_f64(l5, 3) - wave_lane_f64(l5, 4);           // lf(N-n) - lf(N)
    const int64_t k0 = up ? a : a - 1;                   // the first term: the largest of the side that is summed
    const int64_t rest = N - K - n;                      // (N-K-n+k >= 0 on the support)
    double tFirst = 0.0, acc = 0.0;
    for (int64_t base = 0;; base += IGD_WAVE) {
        const int64_t kk = up ? k0 + base + lane : k0 - base - lane;
        const bool in = up ? kk <= hi : kk >= lo;
        const int64_t k = in ? kk : k0;                  // (a lane past the end computes a term it does not add)
        // t = ((lf(K) - lf(K-k)) + (lf(N-K) - lf(N-K-n+k))) + (((lf(n) - lf(n-k)) - lf(k)) + tail5): one lgamma body, four rounds
        double p01 = 0.0, p23 = 0.0;
#pragma unroll 1
        for (int j = 0; j < 4; j++) {
            const int64_t x = j == 0 ? K - k : j == 1 ? rest + k : j == 2 ? n - k : k;
            const double dlt = (j == 0 ? lfK : j == 1 ? lfNK : j == 2 ? lfn : 0.0) - lgamma((double)x + 1.0);
            if (j < 2) p01 += dlt; else p23 += dlt;
        }
        const double t = p01 + (p23 + tail5);
        const double t0 = wave_lane_f64(t, 0);           // the step's largest term
        if (base == 0) tFirst = t0;
        if (in) acc += exp(t - tFirst);
        if (t0 < tFirst - IGD_FISHER_STOP) break;
        if (up ? k0 + base + IGD_WAVE > hi : k0 - base - IGD_WAVE < lo) break;
    }
    const double S = wave_lane_f64(wave_inclusive_sum_f64(acc), 63);            // >= 1: the first term itself
    double lp = tFirst + log(S);                         // log of the summed side
    if (!up) {
        double L = exp(lp);
        if (!(L < 1.0)) L = 0x1.fffffffffffffp-1;        // (rounding only: p >= P(X >= mode) keeps L well below 1)
        lp = log1p(-L);
    }
    const double r = -lp / IGD_FISHER_LN10;
    return r > 0.0 ? r : 0.0;
}

template <bool ENRICH>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_fisher_cells(const int64_t *__restrict__ A, const int64_t *__restrict__ B,
                                                               const int64_t *__restrict__ C, const int64_t *__restrict__ D,
                                                               int64_t nU, int64_t nF, int64_t cell0, int64_t ncell,
                                                               double *__restrict__ plog, double *__restrict__ odds,
                                                               u64 *__restrict__ clamped)
{
    // GENERIC: A, B, C, D are the tables' entries [ncell].  ENRICH: A = support[ncell] (the cells cell0 .. of the matrix),
    // B = usupport[nF], C = n_k[nsets]; D is not read.
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t stride = (int64_t)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int64_t i = (int64_t)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; i < ncell; i += stride) {
        int64_t a, b, c, d;
        if (ENRICH) {
            const int64_t g = cell0 + i, k = g / nF, f = g - k * nF;
            a = wave_uniform_i64(A[i]);
            const int64_t u = wave_uniform_i64(B[f]), nk = wave_uniform_i64(C[k]);
            b = u - a;
            c = nk - a;
            d = nU - a - b - c;                          // (from b as defined, before its clamp: n_U - u - c)
            const bool cb = b < 0, cd = d < 0;
            if (cb) b = 0;
            if (cd) d = 0;
            if (c < 0) c = 0;                            // (cannot happen: support <= |set|; keeps the entries >= 0)
            if ((cb || cd) && lane == 0) (void)__hip_atomic_fetch_add(clamped + k, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            a = wave_uniform_i64(A[i]);
            b = wave_uniform_i64(B[i]);
            c = wave_uniform_i64(C[i]);
            d = wave_uniform_i64(D[i]);
        }
        const double r = fisher_wave_cell(a, b, c, d, lane);
        if (lane == 0) {
            plog[i] = r;
            if (odds) {
                const double ad = (double)a * (double)d, bc = (double)b * (double)c;
                odds[i] = bc == 0.0 ? (ad > 0.0 ? __builtin_inf() : __builtin_nan("")) : ad / bc;
            }
        }
    }
}
