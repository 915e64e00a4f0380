// engine/merge_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// Merging region sets on the device, as `bedtools merge -d gap` (the definitions are in include/igd_hip.h):
// the keys of the segmented sort, the segmented maximum scan of the ends, the run heads and their compaction.
// ------------------------------------------------------------------------------------------
// The sort is radix_sort_pairs (igd_sortscan.hpp) over the region numbers: stable LSD passes by qe, qs, ichr and the set
// number, the key of each gathered through the permutation so far (igd_merge_key).  A region that does not take part gets
// the set number nsets, so it ends up behind every set and the kernels below only have to skip that one value.
//
// The scan has the three-launch shape of exclusive_scan: tile aggregates, one workgroup over the aggregates, apply.  A
// single pass would hand the carry from workgroup to workgroup through memory and make each wait for the one before it;
// nothing in this stage is worth a spin between workgroups, and three short launches have no way to hang.  The element is
// the pair (head, max): head says that a segment -- one (set, contig) -- begins inside the span, max is the largest end since
// the last such beginning.  The operator is the usual segmented one,
//     (h1, m1) o (h2, m2) = (h1 | h2, h2 ? m2 : max(m1, m2)),
// associative, with the identity (0, INT32_MIN); ends that take part are above INT32_MIN (qe > qs), so the identity's max
// also says "no earlier region of this segment" where it comes out as the exclusive value of a segment's first region.
//
// Every store is an ordinary vector store; there are no atomics and no LDS beyond the waves' partials.
#define IGD_MERGE_WG 256
#define IGD_MERGE_NONE INT32_MIN                       // exclusive maximum of a segment's first region

struct MergeAgg { int32_t head, mx; };
static __device__ __forceinline__ MergeAgg merge_op(MergeAgg a, MergeAgg b)
{
    return MergeAgg{a.head | b.head, b.head ? b.mx : (a.mx > b.mx ? a.mx : b.mx)};
}
static __device__ __forceinline__ MergeAgg merge_shfl_up(MergeAgg a, int o)
{
    return MergeAgg{__shfl_up(a.head, o), __shfl_up(a.mx, o)};
}

// set number of every region (nsets where it does not take part: no contig of the database, qe <= qs), the identity permutation and the
// first key, qe.  Signed coordinates order as unsigned ones once the sign bit is flipped.
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_sets_of(const int32_t *__restrict__ ichr, const int32_t *__restrict__ qs,
                                                                        const int32_t *__restrict__ qe, const int64_t *__restrict__ set_off,
                                                                        int32_t nsets, int32_t nctg, int64_t n, uint32_t *__restrict__ setOf,
                                                                        uint32_t *__restrict__ key, uint32_t *__restrict__ perm)
{
    for (int64_t i = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IGD_MERGE_WG) {
        int32_t lo = 0, hi = nsets;                      // the last k with set_off[k] <= i (set_off[0] = 0 <= i < n = set_off[nsets])
        while (hi - lo > 1) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (set_off[mid] <= i) lo = mid; else hi = mid;
        }
        const int32_t e = qe[i];
        const bool in = igd_hip_merge_takes_part(nctg, ichr[i], qs[i], e);
        setOf[i] = in ? (uint32_t)lo : (uint32_t)nsets;
        key[i] = (uint32_t)e ^ 0x80000000u;
        perm[i] = (uint32_t)i;
    }
}

// the next key through the permutation so far: which = 0 qs, 1 ichr (0 where the region does not take part), 2 the set number
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_key(const int32_t *__restrict__ ichr, const int32_t *__restrict__ qs,
                                                                    const uint32_t *__restrict__ setOf, int32_t nsets,
                                                                    const uint32_t *__restrict__ perm, int64_t n, int which,
                                                                    uint32_t *__restrict__ key)
{
    for (int64_t i = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IGD_MERGE_WG) {
        const uint32_t p = perm[i];
        const uint32_t s = setOf[p];
        key[i] = which == 0 ? (uint32_t)qs[p] ^ 0x80000000u : which == 1 ? (s == (uint32_t)nsets ? 0u : (uint32_t)ichr[p]) : s;
    }
}

// the regions in sorted order
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_gather(const int32_t *__restrict__ ichr, const int32_t *__restrict__ qs,
                                                                       const int32_t *__restrict__ qe, const uint32_t *__restrict__ setOf,
                                                                       const uint32_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ sSet,
                                                                       int32_t *__restrict__ sChr, int32_t *__restrict__ sQs, int32_t *__restrict__ sQe)
{
    for (int64_t i = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IGD_MERGE_WG) {
        const uint32_t p = perm[i];
        sSet[i] = setOf[p];
        sChr[i] = ichr[p];
        sQs[i] = qs[p];
        sQe[i] = qe[p];
    }
}

// element i of the scan: head where (set, contig) differs from element i - 1
static __device__ __forceinline__ MergeAgg merge_elem(const uint32_t *__restrict__ sSet, const int32_t *__restrict__ sChr,
                                                      const int32_t *__restrict__ sQe, int64_t i)
{
    const bool head = i == 0 || sSet[i] != sSet[i - 1] || sChr[i] != sChr[i - 1];
    return MergeAgg{head ? 1 : 0, sQe[i]};
}

// first launch: the aggregate of every tile of SCAN_TILE elements (thread t takes SCAN_PER consecutive ones, as the apply does)
static __global__ void __launch_bounds__(SCAN_WG) igd_merge_scan_tiles(const uint32_t *__restrict__ sSet, const int32_t *__restrict__ sChr,
                                                                      const int32_t *__restrict__ sQe, int64_t n, MergeAgg *__restrict__ tiles)
{
    __shared__ MergeAgg wagg[SCAN_WG / WAVE];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    MergeAgg a{0, IGD_MERGE_NONE};
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++)
        if (base + k < n) a = merge_op(a, merge_elem(sSet, sChr, sQe, base + k));
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    for (int o = 1; o < WAVE; o <<= 1) {
        const MergeAgg y = merge_shfl_up(a, o);
        if (lane >= o) a = merge_op(y, a);
    }
    if (lane == WAVE - 1) wagg[w] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        MergeAgg t = wagg[0];
        for (int k = 1; k < SCAN_WG / WAVE; k++) t = merge_op(t, wagg[k]);
        tiles[blockIdx.x] = t;
    }
}

// second launch, one workgroup: tiles[b] becomes the aggregate of every tile before b (exclusive; the identity for tile 0).
// The workgroup takes the tiles in rounds of blockDim.x (a multiple of WAVE, IGD_MERGE_CARRY_WG in production) and hands
// the pair from round to round through `carry`.
#define IGD_MERGE_CARRY_WG 1024
static __global__ void __launch_bounds__(IGD_MERGE_CARRY_WG) igd_merge_scan_carry(MergeAgg *__restrict__ tiles, int64_t nb)
{
    __shared__ MergeAgg wagg[IGD_MERGE_CARRY_WG / WAVE];
    __shared__ MergeAgg carry;
    if (threadIdx.x == 0) carry = MergeAgg{0, IGD_MERGE_NONE};
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    for (int64_t base = 0; base < nb; base += blockDim.x) {
        const int64_t i = base + threadIdx.x;
        MergeAgg x = i < nb ? tiles[i] : MergeAgg{0, IGD_MERGE_NONE};
        for (int o = 1; o < WAVE; o <<= 1) {
            const MergeAgg y = merge_shfl_up(x, o);
            if (lane >= o) x = merge_op(y, x);
        }
        if (lane == WAVE - 1) wagg[w] = x;               // inclusive over the wave
        MergeAgg ex = merge_shfl_up(x, 1);               // exclusive within the wave
        if (lane == 0) ex = MergeAgg{0, IGD_MERGE_NONE};
        __syncthreads();
        MergeAgg pre = carry;
        for (int k = 0; k < w; k++) pre = merge_op(pre, wagg[k]);
        if (i < nb) tiles[i] = merge_op(pre, ex);
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) carry = merge_op(pre, x);
        __syncthreads();
    }
}

// third launch: per element the inclusive maximum inc[], the exclusive one exc[] (IGD_MERGE_NONE at a segment's first region)
// and the run flag: the region takes part and opens a run -- first of its (set, contig), or qs > E + gap in 64 bits
static __global__ void __launch_bounds__(SCAN_WG) igd_merge_scan_apply(const uint32_t *__restrict__ sSet, const int32_t *__restrict__ sChr,
                                                                      const int32_t *__restrict__ sQs, const int32_t *__restrict__ sQe,
                                                                      int64_t n, uint32_t nsets, int64_t gap, const MergeAgg *__restrict__ tiles,
                                                                      int32_t *__restrict__ inc, int32_t *__restrict__ exc, uint32_t *__restrict__ flag)
{
    __shared__ MergeAgg wagg[SCAN_WG / WAVE];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    MergeAgg v[SCAN_PER], a{0, IGD_MERGE_NONE};
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++) {
        v[k] = base + k < n ? merge_elem(sSet, sChr, sQe, base + k) : MergeAgg{0, IGD_MERGE_NONE};
        a = merge_op(a, v[k]);
    }
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    MergeAgg x = a;
    for (int o = 1; o < WAVE; o <<= 1) {
        const MergeAgg y = merge_shfl_up(x, o);
        if (lane >= o) x = merge_op(y, x);
    }
    if (lane == WAVE - 1) wagg[w] = x;
    MergeAgg ex = merge_shfl_up(x, 1);                   // everything of the wave before this thread
    if (lane == 0) ex = MergeAgg{0, IGD_MERGE_NONE};
    __syncthreads();
    MergeAgg pre = tiles[blockIdx.x];
    for (int k = 0; k < w; k++) pre = merge_op(pre, wagg[k]);
    pre = merge_op(pre, ex);
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++) {
        const int64_t i = base + k;
        if (i < n) {
            const int32_t E = v[k].head ? IGD_MERGE_NONE : pre.mx;
            pre = merge_op(pre, v[k]);
            inc[i] = pre.mx;
            exc[i] = E;
            flag[i] = sSet[i] != nsets && (v[k].head || igd_hip_merge_opens(sQs[i], E, gap)) ? 1u : 0u;
        }
    }
}

// the sorted position of every run's first region: runStart[pos[i]] = i where flag[i]
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_heads(const uint32_t *__restrict__ flag, const int64_t *__restrict__ pos, int64_t n,
                                                                      int32_t *__restrict__ runStart)
{
    for (int64_t i = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * IGD_MERGE_WG)
        if (flag[i]) runStart[pos[i]] = (int32_t)i;
}

// first sorted position whose set number is >= k (n if there is none)
static __device__ __forceinline__ int64_t merge_lower(const uint32_t *__restrict__ sSet, int64_t n, uint32_t k)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (sSet[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the runs: (ichr, first qs, maximum qe, regions joined) of run r < *total, zeros in the rest of the capacity n
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_runs(const uint32_t *__restrict__ sSet, const int32_t *__restrict__ sChr,
                                                                     const int32_t *__restrict__ sQs, const int32_t *__restrict__ inc,
                                                                     const int32_t *__restrict__ runStart, const int64_t *__restrict__ total,
                                                                     int64_t n, uint32_t nsets, int32_t *__restrict__ m_ichr,
                                                                     int32_t *__restrict__ m_qs, int32_t *__restrict__ m_qe, int32_t *__restrict__ m_count)
{
    const int64_t R = *total;
    for (int64_t r = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; r < n; r += (int64_t)gridDim.x * IGD_MERGE_WG) {
        int32_t c = 0, s = 0, e = 0, cnt = 0;
        if (r < R) {
            const int64_t i = runStart[r];
            const int64_t nxt = r + 1 < R ? (int64_t)runStart[r + 1] : merge_lower(sSet, n, nsets);     // (the regions that take part end there)
            c = sChr[i]; s = sQs[i]; e = inc[nxt - 1]; cnt = (int32_t)(nxt - i);
        }
        m_ichr[r] = c; m_qs[r] = s; m_qe[r] = e;
        if (m_count) m_count[r] = cnt;
    }
}

// per set: m_off[k] = runs of the sets before k (k = 0 .. nsets), n_dropped[k] = its regions that do not take part
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_offsets(const uint32_t *__restrict__ sSet, const int64_t *__restrict__ pos,
                                                                        const int64_t *__restrict__ total, int64_t n,
                                                                        const int64_t *__restrict__ set_off, int32_t nsets,
                                                                        int64_t *__restrict__ m_off, int64_t *__restrict__ n_dropped)
{
    for (int64_t k = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; k <= nsets; k += (int64_t)gridDim.x * IGD_MERGE_WG) {
        const int64_t lb = merge_lower(sSet, n, (uint32_t)k);
        m_off[k] = lb < n && k < nsets ? pos[lb] : *total;
        if (k < nsets && n_dropped) n_dropped[k] = (set_off[k + 1] - set_off[k]) - (merge_lower(sSet, n, (uint32_t)k + 1) - lb);
    }
}
