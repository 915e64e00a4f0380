// engine/rank_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_rank_rows: per row of an enrichment table the ranks of its cells by support, by pvalue_log and by odds ratio, their
// maximum and mean, and Benjamini-Hochberg q-values in log10 (host_rank.hpp)
// ------------------------------------------------------------------------------------------
// A row is the m = ncols cells of one query set; the family of the correction is the row.
//   rank     1 + #{g : x[g] > x[f]}: ties take the minimum rank.  +inf is the largest odds ratio, NaN ranks below every
//            number and all NaN of a row tie.
//   q        r[f] = #{g : p[g] >= p[f]}, adj[f] = p[f] + (log10 r[f] - log10 m), q[f] = max(+0.0, max{adj[g] : p[g] <= p[f]}),
//            p = pvalue_log: -log10 of min(1, min over j >= i of m p_(j) / j), never leaving log space.  The difference of
//            the two logarithms is formed first, so r == m gives adj == p bit for bit.
//   shape    ONE WORKGROUP PER ROW; persistent workgroups stride over the rows.  Per column the workgroup
//            1. builds a 64-bit key per cell whose unsigned order is the column's order (rank_key_*), carries the cell's
//               column number beside it, and pads to n = the next power of two with key 0 / index 0xffffffff;
//            2. sorts DESCENDING with a bitonic network, one compare-exchange per thread and step, a barrier between
//               stages.  Equal keys are ordered by index, so the order is total: the result does not depend on the
//               network, and the padding ends behind every cell of the row, also behind cells whose key is 0 (a NaN, a
//               pvalue_log of +0.0);
//            3. scans the sorted row from the left: the start of a cell's tie run is its rank - 1.  Every thread owns n /
//               256 consecutive positions, finds the last run start among them, takes the last one before them from an
//               exclusive max-scan over the threads (wg_excl_max) and walks its positions again, scattering rank[idx];
//            4. for pvalue_log scans from the right the same way (thread t owns the positions of 255 - t, so the scan over
//               threads is the same prefix scan): the end of a cell's tie run is r.  A second scan over the threads
//               carries the maximum of adj over everything to the right; the walk is repeated with it and scatters q[idx].
//            When all three ranks are in place a last pass forms max_rnk and mean_rnk = (sum of the three) / 3.0.
//   memory   LDS form: keys (8 bytes) and indices (4) of the padded row in dynamic LDS, 12 n + 64 bytes: up to
//            IGD_RANK_LDS_COLS = 8192 columns (96 KiB of the CU's 160).  GLOBAL form, wider rows: the same code on the
//            workgroup's slice of a global workspace ([gridDim.x][n] keys, then indices); __syncthreads() orders a
//            workgroup's own global stores as it does its LDS stores.
//            The compare-exchange reads two 8-byte keys at distance j; below j = 32 the lanes of a half wave fall on 16
//            banks two by two (a 2-way conflict on 5 of a stage's log2 n steps), from j = 32 on there is none.
//   stores   every cell of every requested column is stored, once: outputs are DEFINED.  No atomics.
// The host checks ncols <= IGD_RANK_MAX_COLS and that no pvalue_log is negative or NaN before a launch.
#define IGD_RANK_LDS_COLS 8192
#define IGD_RANK_MAX_COLS ((int64_t)1 << 20)
#define IGD_RANK_SCR_BYTES 64                        // scan scratch in front of the LDS arrays (keeps them 16-byte aligned)
#define IGD_RANK_PAD_IDX 0xffffffffu
#define IGD_RANK_DO_SUP 1                            // columns to rank
#define IGD_RANK_DO_PV 2
#define IGD_RANK_DO_OR 4
#define IGD_RANK_DO_Q 8                              // ... and q-values with the pvalue_log column
#define IGD_RANK_DO_MM 16                            // ... and max_rnk / mean_rnk (needs the three)

__device__ __forceinline__ u64 rank_key_sup(int64_t s) { return (u64)s ^ 0x8000000000000000ull; }
__device__ __forceinline__ u64 rank_key_pv(double p) { return p == 0.0 ? 0ull : (u64)__double_as_longlong(p); }   // (p >= +0.0: the bits are monotone)
__device__ __forceinline__ u64 rank_key_or(double x)
{
    if (x != x) return 0ull;                             // NaN: below -inf (whose key is 0x000fffffffffffff)
    const u64 b = x == 0.0 ? 0ull : (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
// does (ka, ia) come before (kb, ib) in the sorted row?  (descending keys, ascending index among equal keys)
__device__ __forceinline__ bool rank_before(u64 ka, unsigned ia, u64 kb, unsigned ib) { return ka > kb || (ka == kb && ia < ib); }

// exclusive max-scan over the threads of the workgroup, in thread order: the maximum of v over the threads before this one
// (ident for thread 0).  scr: IGD_SETS_WG / IGD_WAVE values of LDS.  Every thread takes part; two barriers.
template <typename T>
__device__ __forceinline__ T wg_excl_max(T v, T ident, T *scr)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < IGD_WAVE; d <<= 1) {
        const T o = __shfl_up(v, d, IGD_WAVE);
        if (lane >= d && o > v) v = o;
    }
    if (lane == IGD_WAVE - 1) scr[wave] = v;
    T ex = __shfl_up(v, 1, IGD_WAVE);
    if (lane == 0) ex = ident;
    __syncthreads();
    for (int w = 0; w < wave; w++) {
        const T o = scr[w];
        if (o > ex) ex = o;
    }
    __syncthreads();
    return ex;
}

// One column of one row: sort, ranks, and (Q) q-values.  key[] / idx[] hold the padded row (n entries) on entry.
template <bool Q>
__device__ __forceinline__ void rank_column(u64 *key, unsigned *idx, int m, int n, double log10m, int32_t *__restrict__ rnk,
                                            double *__restrict__ q, void *scr)
{
    const int t = threadIdx.x;
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int p = t; p < (n >> 1); p += IGD_SETS_WG) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const u64 ki = key[i], kl = key[l];
                const unsigned ii = idx[i], il = idx[l];
                const bool desc = (i & k) == 0;
                if (desc ? rank_before(kl, il, ki, ii) : rank_before(ki, ii, kl, il)) {
                    key[i] = kl; key[l] = ki;
                    idx[i] = il; idx[l] = ii;
                }
            }
        }
    __syncthreads();
    const int S = n >= IGD_SETS_WG ? n / IGD_SETS_WG : 1;      // positions per thread (n is a power of two)
    {
        // from the left: the cells 0 .. m-1 of the sorted row (the padding lies behind them)
        const int a = t * S < m ? t * S : m, b = a + S < m ? a + S : m;
        int last = -1;
        for (int j = a; j < b; j++)
            if (j == 0 || key[j - 1] != key[j]) last = j;
        int cur = wg_excl_max<int>(last, -1, (int *)scr);
        for (int j = a; j < b; j++) {
            if (j == 0 || key[j - 1] != key[j]) cur = j;
            const unsigned c = idx[j];
            if (c < (unsigned)m) rnk[c] = cur + 1;       // (always: the padding sorts behind the m cells)
        }
    }
    if (Q) {
        // from the right: thread t owns the positions of thread 255 - t.  A run ends at j when j is the row's last cell or
        // the next key differs; scans carry the NEGATED position of the nearest end to the right, then the maximum of adj
        const int o = IGD_SETS_WG - 1 - t;
        const int a = o * S < m ? o * S : m, b = a + S < m ? a + S : m;
        int first = -INT_MAX;
        for (int j = b - 1; j >= a; j--)
            if (j == m - 1 || key[j + 1] != key[j]) first = -j;
        const int endR = -wg_excl_max<int>(first, -INT_MAX, (int *)scr);      // (only read when the thread's last cell is no run end: an end lies to the right then)
        double best = -__builtin_inf();
        for (int pass = 0; pass < 2; pass++) {
            int cur = endR;
            double adj = 0.0, run = best;
            bool have = false;
            for (int j = b - 1; j >= a; j--) {
                const bool end = j == m - 1 || key[j + 1] != key[j];
                if (end) cur = j;
                if (end || !have) {
                    adj = __longlong_as_double((long long)key[j]) + (log10((double)(cur + 1)) - log10m);
                    have = true;
                }
                if (adj > run) run = adj;
                const unsigned c = idx[j];
                if (pass && c < (unsigned)m) q[c] = run > 0.0 ? run : 0.0;
            }
            if (pass == 0) best = wg_excl_max<double>(run, -__builtin_inf(), (double *)scr);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_rank_rows(const int64_t *__restrict__ sup, const double *__restrict__ pv,
                                                            const double *__restrict__ odds, int64_t nrows, int m, int n, int what,
                                                            u64 *__restrict__ wsKey, unsigned *__restrict__ wsIdx,
                                                            double *__restrict__ q, int32_t *__restrict__ rSup, int32_t *__restrict__ rPv,
                                                            int32_t *__restrict__ rOr, int32_t *__restrict__ rMax, double *__restrict__ rMean)
{
    extern __shared__ __attribute__((aligned(16))) char rank_smem[];
    u64 *key = LDS ? (u64 *)(rank_smem + IGD_RANK_SCR_BYTES) : wsKey + (size_t)blockIdx.x * (size_t)n;
    unsigned *idx = LDS ? (unsigned *)(rank_smem + IGD_RANK_SCR_BYTES + (size_t)n * 8) : wsIdx + (size_t)blockIdx.x * (size_t)n;
    const int t = threadIdx.x;
    const double log10m = log10((double)m);
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const size_t base = (size_t)row * (size_t)m;
        if (what & IGD_RANK_DO_SUP) {
            __syncthreads();                             // (the row before is done with key[] / idx[])
            for (int c = t; c < n; c += IGD_SETS_WG) {
                key[c] = c < m ? rank_key_sup(sup[base + c]) : 0ull;
                idx[c] = c < m ? (unsigned)c : IGD_RANK_PAD_IDX;
            }
            rank_column<false>(key, idx, m, n, log10m, rSup + base, nullptr, rank_smem);
        }
        if (what & IGD_RANK_DO_OR) {
            __syncthreads();
            for (int c = t; c < n; c += IGD_SETS_WG) {
                key[c] = c < m ? rank_key_or(odds[base + c]) : 0ull;
                idx[c] = c < m ? (unsigned)c : IGD_RANK_PAD_IDX;
            }
            rank_column<false>(key, idx, m, n, log10m, rOr + base, nullptr, rank_smem);
        }
        if (what & IGD_RANK_DO_PV) {
            __syncthreads();
            for (int c = t; c < n; c += IGD_SETS_WG) {
                key[c] = c < m ? rank_key_pv(pv[base + c]) : 0ull;
                idx[c] = c < m ? (unsigned)c : IGD_RANK_PAD_IDX;
            }
            if (what & IGD_RANK_DO_Q) rank_column<true>(key, idx, m, n, log10m, rPv + base, q + base, rank_smem);
            else rank_column<false>(key, idx, m, n, log10m, rPv + base, nullptr, rank_smem);
        }
        if (what & IGD_RANK_DO_MM) {
            __syncthreads();                             // the workgroup's three rank rows are in place
            for (int c = t; c < m; c += IGD_SETS_WG) {
                const int a = rSup[base + c], b = rPv[base + c], d = rOr[base + c];
                rMax[base + c] = a > b ? (a > d ? a : d) : (b > d ? b : d);
                rMean[base + c] = (double)(a + b + d) / 3.0;
            }
        }
    }
}
