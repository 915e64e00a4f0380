// engine/flank_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_flank_rows, igd_flank_reldist: the nearest record on EACH side of every region per dataset, and the histogram of the
// relative distance min(up, down) / (up + down) per set and dataset
// (igd_hip_flank / igd_hip_flank_dev / igd_hip_flank_reldist; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// igd_flank_rows is igd_nearest_rows (nearest_dev.hpp) with TWO minima per (region, dataset): the same grid
// (igd_hip_nearest_grid), the same widened interval, walk_query_tiles<USE_V, false> unchanged -- its predicate IS "counted" --
// and a step that asks igd_hip_flank_pair (MID: the measure, a template argument) for the record's side and distance: a lane's
// record goes to at most one of the two tables.
//
// LDS form (at most IGD_FLANK_LDS_FILES files): two tables of nF words per wave, up then down, PRIVATE to the wave, 0xffffffff =
//   none; unsigned minima by LDS atomics that return nothing (ds_min_u32).
//   row      after the region the wave streams each table to its row with plain coalesced vector stores (0xffffffff IS -1),
//            stores 0xffffffff over the words it has read and min-reduces them across the wave into upmin[q] / downmin[q].
//   order    nearest_dev.hpp's argument: one wave only touches its tables, a wave's LDS operations are executed in the order
//            they were issued, so the reads of a row come after every minimum of the region and the next region's minima after
//            the resets; the wave-scope fences keep the compiler from moving the accesses across each other.
//   no hit   A call DEFINES every word.  A table that took no minimum in this region (wave-uniform: the ballots) is not read:
//            its row is STORED as -1.  A region with no counted record reads neither.  There is no memset before the launch.
//   bound    IGD_FLANK_LDS_FILES = 2048 files are 2 x 8 KiB per wave, 64 KiB per workgroup: 32 B per file and workgroup, 59 KiB
//            at 1 900 files.  A CU's 160 KiB hold two workgroups = 8 waves at 1 900 files and at the limit: the occupancy
//            igd_nearest_rows has at ITS limit of 4 096 files, where its bound was put for the same reason (two workgroups per
//            CU still overlap each other's load latency) -- arithmetic, not a measurement.
// Wide form (LDS = false): both rows are filled with 0xff bytes on the stream before the launch and a lane takes its minimum
//   straight into word idx of its side's row with a device-scope atomic that returns nothing (global_atomic_umin); the rows of
//   region q belong to one wave during the launch.  The minima come from igd_nearest_rowmin, launched once per row behind
//   this kernel when the caller wants them.
// igd_flank_reldist counts the two rows of a chunk into the resident histogram of igd_hip_flank_reldist; see there.
// All stores to memory are vector stores or vector atomics.
#define IGD_FLANK_LDS_FILES 2048                     // 2 x 32 KiB of tables per workgroup: two workgroups per CU stay resident

// a wave-uniform pointer kept in vector registers: igd_nearest_rows already sits at the scalar registers' limit, and the second
// row, table and minimum of this kernel would be spilt scalars; the stores and LDS operations take a vector address anyway
template <typename T>
static __device__ __forceinline__ T *flank_in_vgprs(T *p)
{
    asm volatile("" : "+v"(p));
    return p;
}

template <bool USE_V, bool LDS, bool MID>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_flank_rows(DbView db, const int32_t *__restrict__ q_ichr,
                                                             const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                             int nq, int window, int krule, int v, int32_t *__restrict__ up,
                                                             int32_t *__restrict__ down, int32_t *__restrict__ upmin,
                                                             int32_t *__restrict__ downmin)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    igd_lds_u32 *tu = flank_in_vgprs((igd_lds_u32 *)smem + (LDS ? 2 * wave * nF : 0));      // this wave's tables (LDS form): up, then down
    igd_lds_u32 *td = tu + (LDS ? nF : 0);
    up = flank_in_vgprs(up); down = flank_in_vgprs(down);
    upmin = flank_in_vgprs(upmin); downmin = flank_in_vgprs(downmin);
    if (LDS) {
        for (int f = threadIdx.x; f < 2 * (IGD_SETS_WG / IGD_WAVE) * nF; f += IGD_SETS_WG) ((igd_lds_u32 *)smem)[f] = IGD_NEAREST_NONE;
        __syncthreads();
    }
    const int waves = (int)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int q = (int)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; q < nq; q += waves) {
        const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
        const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
        const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
        unsigned *rowU = (unsigned *)up + (size_t)q * (size_t)nF;
        unsigned *rowD = (unsigned *)down + (size_t)q * (size_t)nF;
        int ws, we;
        igd_hip_nearest_widen(qs, qe, window, &ws, &we);
        int gt0 = 0, ntl = 0;
        if (!query_span(db, cc, ws, we, krule, gt0, ntl)) ntl = 0;       // (rows of -1, stored below)
        gt0 = __builtin_amdgcn_readfirstlane(gt0);
        ntl = __builtin_amdgcn_readfirstlane(ntl);
        bool hitU = false, hitD = false;                                  // (per lane; one ballot each after the walk)
        walk_query_tiles<USE_V, false>(db, lane, nF, ws, we, gt0, ntl, v, 0, MinOv{0, 0, 0}, [&](int s0, int e0, int x0, bool h0, int s1, int e1, int x1, bool h1) {
            // (a lane without a counted record computes a side nobody reads)
            unsigned d0 = 0, d1 = 0;
            const int k0 = igd_hip_flank_pair(MID ? IGD_HIP_FLANK_MIDPOINTS : IGD_HIP_FLANK_EDGES, window, qs, qe, s0, e0, &d0);
            const int k1 = igd_hip_flank_pair(MID ? IGD_HIP_FLANK_MIDPOINTS : IGD_HIP_FLANK_EDGES, window, qs, qe, s1, e1, &d1);
            const bool u0 = h0 && k0 == IGD_HIP_FLANK_UP, w0 = h0 && k0 == IGD_HIP_FLANK_DOWN;
            const bool u1 = h1 && k1 == IGD_HIP_FLANK_UP, w1 = h1 && k1 == IGD_HIP_FLANK_DOWN;
            if (LDS) {
                if (u0 || w0) (void)__hip_atomic_fetch_min((u0 ? tu : td) + x0, d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (u1 || w1) (void)__hip_atomic_fetch_min((u1 ? tu : td) + x1, d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                if (u0 || w0) (void)__hip_atomic_fetch_min((u0 ? rowU : rowD) + x0, d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (u1 || w1) (void)__hip_atomic_fetch_min((u1 ? rowU : rowD) + x1, d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            hitU |= u0 | u1;
            hitD |= w0 | w1;
        });
        if (LDS) {
            const bool anyU = __any(hitU), anyD = __any(hitD);
            // the region's minima, then the reads of the rows, then the resets, then the next region's minima: one wave, one
            // LDS unit, program order (see the head of nearest_dev.hpp)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int side = 0; side < 2; side++) {
                igd_lds_u32 *tb = side ? td : tu;
                unsigned *row = side ? rowD : rowU;
                int32_t *rmin = side ? downmin : upmin;
                unsigned m = IGD_NEAREST_NONE;
                if (side ? anyD : anyU) {
                    for (int w = lane; w < nF; w += IGD_WAVE) {
                        const unsigned x = __hip_atomic_load(tb + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(tb + w, IGD_NEAREST_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        row[w] = x;
                        m = x < m ? x : m;
                    }
                    if (rmin)
                        for (int o = 32; o > 0; o >>= 1) {
                            const unsigned y = (unsigned)__shfl_xor((int)m, o);
                            m = y < m ? y : m;
                        }
                } else {
                    for (int w = lane; w < nF; w += IGD_WAVE) row[w] = IGD_NEAREST_NONE;
                }
                if (rmin && lane == 0) rmin[q] = (int32_t)m;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    }
}

// igd_flank_reldist.  The two rows of one chunk of regions (up, down: nF words each; upmin, downmin: one word each, read as
// column nF), igd_nearest_reduce's slice table and the number of bins nb.  hist is u64[rows][nb][nF + 1].  The shape of
// igd_nearest_hist: workgroup (x, y) owns the 64 columns [64 x, 64 x + 64), one per lane, and the slices y, y + gridDim.y, ..;
// the rows of a slice are strided over the four waves.  LDS: u32 h[64][64] addressed bin * 64 + lane (16 KiB; the lanes of a
// wave hit distinct banks, and a lane only ever touches its own column's counters, which the four waves share).  Per element:
// both words are loaded, a pair that is not flanked (igd_hip_flank_flanked) is skipped, and the bin -- the largest k <= nb - 1
// with k (up + down) <= 2 nb min(up, down), which IS min(nb - 1, floor(2 nb min / (up + down))) -- is found by a branch-free
// six-step bisection over k = 0 .. 63: "k <= nb - 1 && k t <= n" is monotone in k; each step is one 64-bit multiply-add
// (v_mad_u64_u32) and a compare, k t <= 63 x 2^31 and n <= 128 x 2^30 stay under 2^38.  No division: a 64-bit division is a
// called routine of some hundred instructions per element here, the bisection about twenty; which is faster on the device is
// unmeasured.  Then one LDS add that returns nothing (ds_add_u32).  Per slice: bins 0 .. nb - 1 are zeroed, the slice is
// counted, and behind a barrier wave w issues for the bins w, w + 4, .. one device-scope 64-bit atomic add (nothing returned) per
// NON-ZERO (bin, column) into hist[row][bin][col], coalesced across the lanes.  A slice holds at most IGD_NEAREST_SLICE = 256
// regions, so a u32 counter holds at most 256.  Only integers are added: no order matters.
__global__ __launch_bounds__(IGD_SETS_WG) void igd_flank_reldist(const int32_t *__restrict__ up, const int32_t *__restrict__ down,
                                                                const int32_t *__restrict__ upmin, const int32_t *__restrict__ downmin,
                                                                int nF, const SetSlice *__restrict__ slices, int nSlices, int nb,
                                                                u64 *__restrict__ hist)
{
    __shared__ unsigned h[IGD_HIP_FLANK_MAX_BINS * IGD_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6);
    const int col = (int)blockIdx.x * IGD_WAVE + lane;
    const bool live = col <= nF;
    const bool fromMin = col == nF;
    for (int s = blockIdx.y; s < nSlices; s += gridDim.y) {
        const SetSlice sl = slices[s];
        for (int i = threadIdx.x; i < nb * IGD_WAVE; i += IGD_SETS_WG) h[i] = 0;
        __syncthreads();
        if (live)
            for (int r = sl.a + wave; r < sl.b; r += IGD_SETS_WG / IGD_WAVE) {
                const size_t at = (size_t)r * (size_t)nF + (size_t)col;
                const int u = fromMin ? upmin[r] : up[at];
                const int d = fromMin ? downmin[r] : down[at];
                if (!igd_hip_flank_flanked(u, d)) continue;
                const u64 t = (u64)(unsigned)u + (u64)(unsigned)d, n = (u64)(2 * nb) * (u64)(unsigned)(u < d ? u : d);
                int pos = 0;
#pragma unroll
                for (int st = 32; st > 0; st >>= 1) pos += (pos + st < nb && (u64)(unsigned)(pos + st) * t <= n) ? st : 0;
                (void)__hip_atomic_fetch_add(&h[pos * IGD_WAVE + lane], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        __syncthreads();
        if (live) {
            u64 *dst = hist + (size_t)sl.row * (size_t)nb * (size_t)(nF + 1) + (size_t)col;
            for (int b = wave; b < nb; b += IGD_SETS_WG / IGD_WAVE) {
                const unsigned c = h[b * IGD_WAVE + lane];
                if (c) (void)__hip_atomic_fetch_add(dst + (size_t)b * (size_t)(nF + 1), (u64)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                                                  // (h[] has been read before the next slice's zeroes)
    }
}
