// engine/map_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_map_rows, igd_map_rowfix, igd_map_reduce: the values of the overlapping records per region and dataset
// (igd_hip_map / igd_hip_map_dev / igd_hip_map_sets; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// count[q][f] = the records of file f that overlap region q, agg[q][f] = the sum, minimum or maximum of their values, 0 where
// count is 0.  The walk is igd_nearest_rows' at W = 0: the wave asks query_span for the tiles of igd_hip_nearest_widen(qs, qe, 0)
// under rule FLAT and runs walk_query_tiles<USE_V, false, true, OP != COUNT> over them, whose predicate
//       lob <= start < qe  &&  end > max(qs, 0)  [&& value >= v]  &&  idx < nFiles
// is "overlaps" with every record met once (records have 0 <= start < end); the step also receives the lane's two value words
// (loaded when the op reads them or the filter does).  The shape is igd_nearest_rows': 256 threads, items_grid(nq, 4) persistent
// workgroups, wave w of the grid takes the regions w, w + waves, ...
//
// LDS form: per wave one table PRIVATE to the wave, u32 count[nF] and, by op, i32 agg[nF] (MIN: INT32_MAX, MAX: INT32_MIN when
//   empty) or u64 agg[nF] (SUM: the values sign-extended, added modulo 2^64 -- the exact sum in two's complement).  The 64-bit
//   tables of the four waves come first in the workgroup's LDS, so that every one of them is 8-byte aligned for any nF.
//   step     a lane with a counted record adds 1 to count[idx] and folds its value into agg[idx] with LDS atomics that return
//            nothing (ds_add_u32; ds_min_i32 / ds_max_i32; ds_add_u64).
//   row      after the region the wave streams its nF counts to count[q] (int32) and its nF aggregates, widened to 64 bits, to
//            agg[q] with plain coalesced vector stores, 64 cells per step, and stores the empty value over what it has read.  A
//            cell with count 0 stores agg 0 (the table's word is the empty value there).  Op COUNT has no agg table; when the
//            caller hands it an agg row all the same, the count is stored there too (a call defines every word it is given).
//   order    nearest_dev.hpp's and member_dev.hpp's argument: one wave only touches its tables, a wave's LDS operations are
//            executed by the LDS unit in the order they were issued, so the reads of the row come after every atomic of the
//            region and the next region's atomics after the resets; the wave-scope fences keep the compiler from moving the
//            accesses across each other.
//   no hit   A region with no counted record (wave-uniform: the ballots, or query_span said no) STORES zeros over its rows
//            without reading its tables; there is no memset of the rows before the launch.
//   bound    IGD_MAP_LDS_WAVE_BYTES = 16 KiB of tables per wave, 64 KiB per workgroup (igd_nearest_rows' budget: two workgroups
//            per CU stay resident at the limit), divided by the bytes per file: 4 (COUNT), 8 (MIN, MAX), 12 (SUM) -- 4 096, 2 048
//            and 1 365 files.  At 1 900 files COUNT and MIN / MAX take this form (30 and 59 KiB per workgroup) and SUM the wide one.
// Wide form (LDS = false, more files): the rows are filled on the stream before the launch -- count with 0, agg with 0 (SUM),
//   0x7f bytes (MIN) or 0x80 bytes (MAX): a 64-bit word above, respectively below, every sign-extended int32 -- and a lane
//   folds straight into cell idx of row q with device-scope atomics that return nothing (global_atomic_add, _add_x2, _smin_x2,
//   _smax_x2); row q belongs to one wave during the launch.  igd_map_rowfix, a small kernel launched behind this one (the
//   pattern of igd_nearest_rowmin), turns the agg of the cells with count 0 into 0 (MIN, MAX) or copies the counts (COUNT with
//   an agg row); SUM needs none.
// igd_map_reduce adds the rows of a chunk into the three resident matrices of igd_hip_map_sets; see there.
// All stores to memory are vector stores or vector atomics.
#define IGD_MAP_LDS_WAVE_BYTES 16384                 // tables of one wave: 64 KiB per workgroup, two workgroups per CU stay resident
#define IGD_MAP_LDS_FILES_COUNT (IGD_MAP_LDS_WAVE_BYTES / 4)
#define IGD_MAP_LDS_FILES_MINMAX (IGD_MAP_LDS_WAVE_BYTES / 8)
#define IGD_MAP_LDS_FILES_SUM (IGD_MAP_LDS_WAVE_BYTES / 12)

typedef __attribute__((address_space(3))) int igd_lds_i32;

// files the LDS form of `op` takes, and the bytes of LDS one file costs a wave
__host__ __device__ constexpr int map_lds_files(int op)
{
    return op == IGD_HIP_MAP_COUNT ? IGD_MAP_LDS_FILES_COUNT : op == IGD_HIP_MAP_SUM ? IGD_MAP_LDS_FILES_SUM : IGD_MAP_LDS_FILES_MINMAX;
}
__host__ __device__ constexpr int map_lds_file_bytes(int op) { return op == IGD_HIP_MAP_COUNT ? 4 : op == IGD_HIP_MAP_SUM ? 12 : 8; }
// the empty value of an agg word while the minimum or maximum is taken (SUM: 0)
__host__ __device__ constexpr int map_agg_empty(int op) { return op == IGD_HIP_MAP_MIN ? INT_MAX : op == IGD_HIP_MAP_MAX ? INT_MIN : 0; }

template <bool USE_V, int OP, bool LDS>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_map_rows(DbView db, const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                           const int32_t *__restrict__ q_qe, int nq, int krule, int v,
                                                           int32_t *__restrict__ count, int64_t *__restrict__ agg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WAVES = IGD_SETS_WG / IGD_WAVE;
    constexpr bool SUM = OP == IGD_HIP_MAP_SUM, MINMAX = OP == IGD_HIP_MAP_MIN || OP == IGD_HIP_MAP_MAX;
    constexpr int EMPTY = map_agg_empty(OP);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    // the workgroup's LDS: [SUM: u64 agg[WAVES][nF]] [MIN, MAX: i32 agg[WAVES][nF]] u32 count[WAVES][nF]
    igd_lds_u64 *ta64 = (igd_lds_u64 *)smem + (LDS && SUM ? wave * nF : 0);
    igd_lds_i32 *ta32 = (igd_lds_i32 *)smem + (LDS && MINMAX ? wave * nF : 0);
    igd_lds_u32 *tc = (igd_lds_u32 *)(smem + (LDS ? (size_t)(WAVES * nF) * (SUM ? 8 : MINMAX ? 4 : 0) : 0)) + (LDS ? wave * nF : 0);
    if (LDS) {
        for (int f = lane; f < nF; f += IGD_WAVE) {                       // (each wave its own tables)
            tc[f] = 0;
            if (SUM) ta64[f] = 0;
            if (MINMAX) ta32[f] = EMPTY;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    const int waves = (int)gridDim.x * WAVES;
    for (int q = (int)blockIdx.x * WAVES + wave; q < nq; q += waves) {
        const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
        const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
        const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
        unsigned *crow = (unsigned *)count + (size_t)q * (size_t)nF;
        int64_t *arow = agg ? agg + (size_t)q * (size_t)nF : nullptr;
        int ws, we;
        igd_hip_nearest_widen(qs, qe, 0, &ws, &we);
        int gt0 = 0, ntl = 0;
        if (!query_span(db, cc, ws, we, krule, gt0, ntl)) ntl = 0;       // (rows of zeros, stored below)
        gt0 = __builtin_amdgcn_readfirstlane(gt0);
        ntl = __builtin_amdgcn_readfirstlane(ntl);
        u64 any = 0;
        walk_query_tiles<USE_V, false, true, OP != IGD_HIP_MAP_COUNT>(db, lane, nF, ws, we, gt0, ntl, v, 0, MinOv{0, 0, 0},
                                                                      [&](int, int, int x0, bool h0, int v0, int, int, int x1, bool h1, int v1) {
            if (LDS) {
                if (h0) (void)__hip_atomic_fetch_add(tc + x0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h1) (void)__hip_atomic_fetch_add(tc + x1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (SUM) {
                    if (h0) (void)__hip_atomic_fetch_add(ta64 + x0, (u64)(int64_t)v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_add(ta64 + x1, (u64)(int64_t)v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (OP == IGD_HIP_MAP_MIN) {
                    if (h0) (void)__hip_atomic_fetch_min(ta32 + x0, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_min(ta32 + x1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else if (OP == IGD_HIP_MAP_MAX) {
                    if (h0) (void)__hip_atomic_fetch_max(ta32 + x0, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (h1) (void)__hip_atomic_fetch_max(ta32 + x1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                if (h0) (void)__hip_atomic_fetch_add(crow + x0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (h1) (void)__hip_atomic_fetch_add(crow + x1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (SUM) {
                    if (h0) (void)__hip_atomic_fetch_add((u64 *)arow + x0, (u64)(int64_t)v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h1) (void)__hip_atomic_fetch_add((u64 *)arow + x1, (u64)(int64_t)v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (OP == IGD_HIP_MAP_MIN) {
                    if (h0) (void)__hip_atomic_fetch_min((long long *)arow + x0, (long long)v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h1) (void)__hip_atomic_fetch_min((long long *)arow + x1, (long long)v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (OP == IGD_HIP_MAP_MAX) {
                    if (h0) (void)__hip_atomic_fetch_max((long long *)arow + x0, (long long)v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h1) (void)__hip_atomic_fetch_max((long long *)arow + x1, (long long)v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            any |= __ballot(h0) | __ballot(h1);
        });
        if (LDS) {
            if (any) {
                // the region's atomics, then the reads of the rows, then the resets, then the next region's atomics: one wave,
                // one LDS unit, program order (see the head of this file)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                for (int w = lane; w < nF; w += IGD_WAVE) {
                    const unsigned c = __hip_atomic_load(tc + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(tc + w, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    crow[w] = c;
                    if (SUM) {
                        const u64 a = __hip_atomic_load(ta64 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(ta64 + w, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        arow[w] = (int64_t)a;
                    } else if (MINMAX) {
                        const int a = __hip_atomic_load(ta32 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(ta32 + w, EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        arow[w] = c ? (int64_t)a : 0;
                    } else if (arow) {
                        arow[w] = (int64_t)c;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            } else {
                for (int w = lane; w < nF; w += IGD_WAVE) {
                    crow[w] = 0;
                    if (arow) arow[w] = 0;
                }
            }
        }
    }
}

// wide form, launched behind igd_map_rows<., OP, false> when OP is not SUM: over the n = nq * nF cells, MIN and MAX turn the agg
// of a cell without a counted record (still the fill of the rows) into 0; COUNT with an agg row copies the count
template <int OP>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_map_rowfix(const int32_t *__restrict__ count, int64_t *__restrict__ agg, size_t n)
{
    const size_t step = (size_t)gridDim.x * IGD_SETS_WG;
    for (size_t i = (size_t)blockIdx.x * IGD_SETS_WG + threadIdx.x; i < n; i += step) {
        const int c = count[i];
        if (OP == IGD_HIP_MAP_COUNT) agg[i] = (int64_t)c;
        else if (c == 0) agg[i] = 0;
    }
}

// igd_map_reduce.  The rows of one chunk of regions (count: nF words each; agg: nF 64-bit words each, NULL under op COUNT, whose
// agg IS the count) and a slice table: slice = (row k of the matrices, regions [a, b) of the chunk), cut on the host so that a
// slice lies in one set.  Each of the three matrices is int64[rows][nF]; stat = n_hit, then pairs at + matWords, then agg_sum
// at + 2 matWords.  The shape of igd_nearest_reduce: workgroup (x, y) owns the 64 columns [64 x, 64 x + 64), one per lane, and
// the slices y, y + gridDim.y, ..; the rows of a slice are strided over the four waves, waves 1..3 hand their three partial sums
// to wave 0 through LDS (3 x 3 x 64 words = 4.5 KiB), and wave 0 issues one device-scope 64-bit atomic add per NON-ZERO statistic
// and column (nothing returned).  Everything is an integer modulo 2^64: the order of slices, chunks and workgroups does not matter.
__global__ __launch_bounds__(IGD_SETS_WG) void igd_map_reduce(const int32_t *__restrict__ count, const int64_t *__restrict__ agg, int nF,
                                                             const SetSlice *__restrict__ slices, int nSlices, u64 *__restrict__ stat,
                                                             int64_t matWords)
{
    __shared__ u64 part[3][IGD_SETS_WG / IGD_WAVE - 1][IGD_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6);
    const int col = (int)blockIdx.x * IGD_WAVE + lane;
    const bool live = col < nF;
    for (int s = blockIdx.y; s < nSlices; s += gridDim.y) {
        const SetSlice sl = slices[s];
        u64 nh = 0, np = 0, sa = 0;
        if (live)
            for (int r = sl.a + wave; r < sl.b; r += IGD_SETS_WG / IGD_WAVE) {
                const size_t i = (size_t)r * (size_t)nF + (size_t)col;
                const unsigned c = (unsigned)count[i];
                nh += c > 0;
                np += c;
                sa += agg ? (u64)agg[i] : (u64)c;
            }
        if (wave > 0) {
            part[0][wave - 1][lane] = nh; part[1][wave - 1][lane] = np; part[2][wave - 1][lane] = sa;
        }
        __syncthreads();
        if (wave == 0 && live) {
            for (int w = 0; w < IGD_SETS_WG / IGD_WAVE - 1; w++) {
                nh += part[0][w][lane]; np += part[1][w][lane]; sa += part[2][w][lane];
            }
            u64 *dst = stat + (size_t)sl.row * (size_t)nF + (size_t)col;
            if (nh) (void)__hip_atomic_fetch_add(dst, nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (np) (void)__hip_atomic_fetch_add(dst + matWords, np, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sa) (void)__hip_atomic_fetch_add(dst + 2 * matWords, sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();                                                  // (wave 0 has read part[] before the next slice's writes)
    }
}
