// engine/nearest_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_nearest_rows, igd_nearest_rowmin, igd_nearest_reduce: the nearest record per dataset within a window
// (igd_hip_nearest / igd_hip_nearest_dev / igd_hip_nearest_sets; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// dist[q][f] = min d over the records of file f within W of region q, -1 when there is none; dmin[q] the minimum over the
// files.  A window search IS the tile walk of the set kernels over the widened interval: the wave computes
//       ws = max(qs - W, 0),  we = min(qe + W, INT_MAX)              (64 bits; igd_hip_nearest_widen)
// asks query_span for the tiles of (ws, we) under rule FLAT and runs walk_query_tiles<USE_V, false> over them, whose predicate
//       lob <= start < we  &&  end > ws  [&& value >= v]  &&  idx < nFiles
// is "within the window" (records have 0 <= start < end, so neither clamp changes it) with every record met once.  The step
// computes d from the TRUE qs, qe in 64 bits (igd_hip_nearest_dist: nothing wraps for coordinates at the ends of int32); a
// counted record has d <= W <= 2^30, so d fits the unsigned word it is minimised in.  The shape is igd_member_rows': 256
// threads, items_grid(nq, 4) persistent workgroups, wave w of the grid takes the regions w, w + waves, ...
//
// LDS form (at most IGD_NEAREST_LDS_FILES files): one table of nF words per wave, PRIVATE to the wave, 0xffffffff = none.
//   min      a lane with a counted record takes an unsigned minimum into word idx with an LDS atomic that returns nothing
//            (ds_min_u32).
//   row      after the region the wave streams its nF words to dist[q] with plain coalesced vector stores, 64 words (256
//            bytes) per step -- 0xffffffff IS -1 -- stores 0xffffffff over the words it has read, and min-reduces them across
//            the wave into dmin[q] (unsigned: "none" is the largest value; one lane stores it).
//   order    member_dev.hpp's argument: one wave only touches its table, a wave's LDS operations are executed by the LDS unit
//            in the order they were issued, so the reads of the row come after every minimum of the region and the next
//            region's minima after the resets; the wave-scope fences keep the compiler from moving the accesses across each
//            other.
//   no hit   A call DEFINES every word.  A region with no counted record (wave-uniform: the ballots, or query_span said no)
//            STORES -1 over its row without reading its table; there is no memset of the rows before the launch.
//   bound    IGD_NEAREST_LDS_FILES = 4096 files are 16 KiB per wave, 64 KiB per workgroup: 16 B per file and workgroup, 30 KiB
//            at 1 900 files.  A CU's 160 KiB hold five workgroups = 20 waves at 1 900 files and two = 8 waves at the limit
//            (of the 32 that the registers allow); the walk is bound by its loads' latency, so the limit sits where two
//            workgroups per CU still overlap each other's -- arithmetic, not a measurement.
// Wide form (LDS = false, more files): the rows are filled with 0xff bytes on the stream before the launch and a lane takes
//   its minimum straight into word idx of row q with a device-scope atomic that returns nothing (global_atomic_umin); row q
//   belongs to one wave during the launch.  dmin comes from igd_nearest_rowmin, a small kernel launched behind this one
//   (the pattern of igd_member_popc); it is not launched when the caller wants no dmin.
// igd_nearest_reduce adds the rows of a chunk into the three resident matrices of igd_hip_nearest_sets; see there.
// SIGNED (igd_hip_nearest_signed / _signed_dev / igd_hip_nearest_hist): the step minimises igd_hip_nearest_key -- 2 d + (d > 0
//   && downstream) -- instead of d: the same table, the same 0xffffffff "none", the same atomics that return nothing (a minimum
//   does not depend on the order of the records).  The stream-out decodes the key on its way to the row
//   (igd_hip_nearest_key_decode: INT32_MIN = none), dmin is decoded after the wave's min-reduction of the KEYS, and a region
//   without a counted record stores INT32_MIN words.  Wide form: the minimum goes into the row as a key and
//   igd_nearest_rowdecode, launched behind (igd_nearest_rowmin's role), takes the row's minimum and decodes the row in place;
//   it runs in every signed call, whether the caller wants sdmin or not.  The unsigned instantiations are what they were.
// igd_nearest_hist counts the signed rows of a chunk into the resident histogram of igd_hip_nearest_hist; see there.
// All stores to memory are vector stores or vector atomics.
#define IGD_NEAREST_LDS_FILES 4096                   // 64 KiB of tables per workgroup: two workgroups per CU stay resident
#define IGD_NEAREST_NONE 0xffffffffu

template <bool USE_V, bool LDS, bool SIGNED = false>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_nearest_rows(DbView db, const int32_t *__restrict__ q_ichr,
                                                               const int32_t *__restrict__ q_qs, const int32_t *__restrict__ q_qe,
                                                               int nq, int window, int krule, int v, int32_t *__restrict__ dist,
                                                               int32_t *__restrict__ dmin)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nF = db.nFiles;
    igd_lds_u32 *tb = (igd_lds_u32 *)smem + (LDS ? wave * nF : 0);       // this wave's table (LDS form)
    if (LDS) {
        for (int f = threadIdx.x; f < (IGD_SETS_WG / IGD_WAVE) * nF; f += IGD_SETS_WG) ((igd_lds_u32 *)smem)[f] = IGD_NEAREST_NONE;
        __syncthreads();
    }
    const int waves = (int)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int q = (int)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; q < nq; q += waves) {
        const int qs = __builtin_amdgcn_readfirstlane(q_qs[q]);
        const int qe = __builtin_amdgcn_readfirstlane(q_qe[q]);
        const int cc = __builtin_amdgcn_readfirstlane(q_ichr[q]);
        unsigned *row = (unsigned *)dist + (size_t)q * (size_t)nF;
        int ws, we;
        igd_hip_nearest_widen(qs, qe, window, &ws, &we);
        int gt0 = 0, ntl = 0;
        if (!query_span(db, cc, ws, we, krule, gt0, ntl)) ntl = 0;       // (a row of -1, stored below)
        gt0 = __builtin_amdgcn_readfirstlane(gt0);
        ntl = __builtin_amdgcn_readfirstlane(ntl);
        u64 any = 0;
        walk_query_tiles<USE_V, false>(db, lane, nF, ws, we, gt0, ntl, v, 0, MinOv{0, 0, 0}, [&](int s0, int e0, int x0, bool h0, int s1, int e1, int x1, bool h1) {
            // (a lane without a counted record computes a d nobody reads)
            const unsigned d0 = SIGNED ? igd_hip_nearest_key(qs, qe, s0, e0) : (unsigned)igd_hip_nearest_dist(qs, qe, s0, e0);
            const unsigned d1 = SIGNED ? igd_hip_nearest_key(qs, qe, s1, e1) : (unsigned)igd_hip_nearest_dist(qs, qe, s1, e1);
            if (LDS) {
                if (h0) (void)__hip_atomic_fetch_min(tb + x0, d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h1) (void)__hip_atomic_fetch_min(tb + x1, d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                if (h0) (void)__hip_atomic_fetch_min(row + x0, d0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (h1) (void)__hip_atomic_fetch_min(row + x1, d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            any |= __ballot(h0) | __ballot(h1);
        });
        if (LDS) {
            if (any) {
                // the region's minima, then the reads of the row, then the resets, then the next region's minima: one wave,
                // one LDS unit, program order (see the head of this file)
                unsigned m = IGD_NEAREST_NONE;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                for (int w = lane; w < nF; w += IGD_WAVE) {
                    const unsigned x = __hip_atomic_load(tb + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(tb + w, IGD_NEAREST_NONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    row[w] = SIGNED ? (unsigned)igd_hip_nearest_key_decode(x) : x;
                    m = x < m ? x : m;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (dmin) {
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned y = (unsigned)__shfl_xor((int)m, o);
                        m = y < m ? y : m;
                    }
                    if (lane == 0) dmin[q] = SIGNED ? igd_hip_nearest_key_decode(m) : (int32_t)m;
                }
            } else {
                for (int w = lane; w < nF; w += IGD_WAVE) row[w] = SIGNED ? (unsigned)IGD_HIP_NEAREST_NO_RECORD : IGD_NEAREST_NONE;
                if (dmin && lane == 0) dmin[q] = SIGNED ? IGD_HIP_NEAREST_NO_RECORD : -1;
            }
        }
    }
}

// wide form: dmin[q] = the unsigned minimum of row q (0xffffffff = -1 = none), one wave per row and step (launched behind
// igd_nearest_rows<., false>)
__global__ __launch_bounds__(IGD_SETS_WG) void igd_nearest_rowmin(const int32_t *__restrict__ dist, int nq, int nF, int32_t *__restrict__ dmin)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int q = (int)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; q < nq; q += waves) {
        const unsigned *row = (const unsigned *)dist + (size_t)q * (size_t)nF;
        unsigned m = IGD_NEAREST_NONE;
        for (int w = lane; w < nF; w += IGD_WAVE) {
            const unsigned x = row[w];
            m = x < m ? x : m;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned y = (unsigned)__shfl_xor((int)m, o);
            m = y < m ? y : m;
        }
        if (lane == 0) dmin[q] = (int32_t)m;
    }
}

// wide form, SIGNED: row q holds minimum keys (0xffffffff = none); the wave takes their minimum, decodes the row IN PLACE
// (every word is read and then written by the same lane) and one lane stores the decoded minimum when dmin is wanted
__global__ __launch_bounds__(IGD_SETS_WG) void igd_nearest_rowdecode(int32_t *__restrict__ dist, int nq, int nF, int32_t *__restrict__ dmin)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)gridDim.x * (IGD_SETS_WG / IGD_WAVE);
    for (int q = (int)blockIdx.x * (IGD_SETS_WG / IGD_WAVE) + wave; q < nq; q += waves) {
        unsigned *row = (unsigned *)dist + (size_t)q * (size_t)nF;
        unsigned m = IGD_NEAREST_NONE;
        for (int w = lane; w < nF; w += IGD_WAVE) {
            const unsigned x = row[w];
            row[w] = (unsigned)igd_hip_nearest_key_decode(x);
            m = x < m ? x : m;
        }
        if (dmin) {
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned y = (unsigned)__shfl_xor((int)m, o);
                m = y < m ? y : m;
            }
            if (lane == 0) dmin[q] = igd_hip_nearest_key_decode(m);
        }
    }
}

// igd_nearest_reduce.  The rows of one chunk of regions (dist: nF words each; dmin: one word each, read as column nF) and a
// slice table: slice = (row k of the matrices, regions [a, b) of the chunk), cut on the host so that a slice lies in one
// set.  Each of the three matrices is int64[rows][nF + 1]; stat = n_within, then n_overlap at + matWords, then sum_dist at
// + 2 matWords.  Workgroup (x, y) owns the 64 columns [64 x, 64 x + 64), one per lane -- a wave's load of a row is 256
// contiguous bytes -- and the slices y, y + gridDim.y, ..; the rows of a slice are strided over the four waves, waves 1..3
// hand their three partial sums to wave 0 through LDS (3 x 3 x 64 words = 4.5 KiB), and wave 0 issues one device-scope
// 64-bit atomic add per NON-ZERO statistic and column (nothing returned).  Everything is an integer: the order in which
// slices, chunks and workgroups arrive does not matter.
__global__ __launch_bounds__(IGD_SETS_WG) void igd_nearest_reduce(const int32_t *__restrict__ dist, const int32_t *__restrict__ dmin,
                                                                 int nF, const SetSlice *__restrict__ slices, int nSlices,
                                                                 u64 *__restrict__ stat, int64_t matWords)
{
    __shared__ u64 part[3][IGD_SETS_WG / IGD_WAVE - 1][IGD_WAVE];
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6);
    const int col = (int)blockIdx.x * IGD_WAVE + lane;
    const bool live = col <= nF;
    const bool fromMin = col == nF;
    for (int s = blockIdx.y; s < nSlices; s += gridDim.y) {
        const SetSlice sl = slices[s];
        u64 nw = 0, no = 0, sd = 0;
        if (live)
            for (int r = sl.a + wave; r < sl.b; r += IGD_SETS_WG / IGD_WAVE) {
                const int x = fromMin ? dmin[r] : dist[(size_t)r * (size_t)nF + (size_t)col];
                nw += x >= 0;
                no += x == 0;
                sd += x >= 0 ? (u64)x : 0;
            }
        if (wave > 0) {
            part[0][wave - 1][lane] = nw; part[1][wave - 1][lane] = no; part[2][wave - 1][lane] = sd;
        }
        __syncthreads();
        if (wave == 0 && live) {
            for (int w = 0; w < IGD_SETS_WG / IGD_WAVE - 1; w++) {
                nw += part[0][w][lane]; no += part[1][w][lane]; sd += part[2][w][lane];
            }
            u64 *dst = stat + (size_t)sl.row * (size_t)(nF + 1) + (size_t)col;
            if (nw) (void)__hip_atomic_fetch_add(dst, nw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (no) (void)__hip_atomic_fetch_add(dst + matWords, no, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sd) (void)__hip_atomic_fetch_add(dst + 2 * matWords, sd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();                                                  // (wave 0 has read part[] before the next slice's writes)
    }
}

// igd_nearest_hist.  The SIGNED rows of one chunk of regions (sdist: nF words each; sdmin: one word each, read as column nF),
// igd_nearest_reduce's slice table, and ne strictly ascending edges.  hist is u64[rows][ne + 1][nF + 1].  The shape of
// igd_nearest_reduce: workgroup (x, y) owns the 64 columns [64 x, 64 x + 64), one per lane, and the slices y, y + gridDim.y,
// ..; the rows of a slice are strided over the four waves.  LDS: u32 h[64][64] addressed bin * 64 + lane (16 KiB; the lanes of
// a wave hit distinct banks, and a lane only ever touches its own column's counters, which the four waves share) and the
// edges as 64 words padded with INT32_MAX -- no sdist is INT32_MAX (|sdist| <= 2^30, or INT32_MIN, which is skipped), so the
// padding is never counted.  Per element: a branch-free six-step bisection, pos += s if edges[pos + s - 1] <= x for s = 32 ..
// 1 (pos + s - 1 <= 62: the 64th word is never read as an edge; pos ends as bin(x) <= ne), then one LDS add that returns
// nothing (ds_add_u32).  Per slice: bins 0 .. ne are zeroed, the slice is counted, and behind a barrier wave w issues for the
// bins w, w + 4, .. one device-scope 64-bit atomic add (nothing returned) per NON-ZERO (bin, column) into hist[row][bin][col],
// coalesced across the lanes.  A slice holds at most IGD_NEAREST_SLICE = 256 regions, so a u32 counter holds at most 256.
// Only integers are added: no order matters.
#define IGD_NEAREST_HIST_BINS 64                     // IGD_HIP_NEAREST_MAX_EDGES + 1
__global__ __launch_bounds__(IGD_SETS_WG) void igd_nearest_hist(const int32_t *__restrict__ sdist, const int32_t *__restrict__ sdmin,
                                                               int nF, const SetSlice *__restrict__ slices, int nSlices,
                                                               const int32_t *__restrict__ edges, int ne, u64 *__restrict__ hist)
{
    __shared__ unsigned h[IGD_NEAREST_HIST_BINS * IGD_WAVE];
    __shared__ int32_t edg[IGD_NEAREST_HIST_BINS];
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6);
    const int col = (int)blockIdx.x * IGD_WAVE + lane;
    const bool live = col <= nF;
    const bool fromMin = col == nF;
    const int nb = ne + 1;
    if (threadIdx.x < IGD_NEAREST_HIST_BINS) edg[threadIdx.x] = (int)threadIdx.x < ne ? edges[threadIdx.x] : INT32_MAX;
    for (int s = blockIdx.y; s < nSlices; s += gridDim.y) {
        const SetSlice sl = slices[s];
        for (int i = threadIdx.x; i < nb * IGD_WAVE; i += IGD_SETS_WG) h[i] = 0;
        __syncthreads();                                                  // (the first slice: the edges are in place too)
        if (live)
            for (int r = sl.a + wave; r < sl.b; r += IGD_SETS_WG / IGD_WAVE) {
                const int x = fromMin ? sdmin[r] : sdist[(size_t)r * (size_t)nF + (size_t)col];
                if (x == IGD_HIP_NEAREST_NO_RECORD) continue;
                int pos = 0;
#pragma unroll
                for (int st = 32; st > 0; st >>= 1) pos += edg[pos + st - 1] <= x ? st : 0;
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
