// engine/cooccur_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_bits_transpose, igd_bitrows_gram: dataset x dataset co-occurrence over a region list (igd_hip_cooccur) and the generic
// entries igd_hip_bits_transpose / igd_hip_bitrows_gram
// ------------------------------------------------------------------------------------------
// cooc[f][g] = #{ q : member[q][f] and member[q][g] } = popc(column f AND column g) of the membership matrix.  The rows of
// igd_member_rows are per query; the product needs them per file, so the rows are transposed into bit COLUMNS first and the
// Gram product then runs over rows of 64-bit words.
//
// igd_bits_transpose.  Input n rows of nW uint32 words (row r at bits + r * nW); output 32 * nW columns of cw = ceil(n / 64)
// uint64 words (column c at cols + c * cw): row r is bit r & 63 of word r >> 6 of column c, c = 32 * w + the bit of word w.
// A workgroup of four waves takes ONE word column w and IGD_TR_BLOCKS = 8 consecutive blocks of 64 rows, two per wave.  A
// wave loads word w of its 64 rows, one row per lane (rows >= n are not read: their lane holds 0), and takes 32 ballots;
// ballot j is the column word of file 32 w + j and is kept by lane j.  The lanes 0..31 put them into an LDS tile [32][8];
// behind the barrier thread t stores word t & 7 of column t >> 3: every column leaves in one run of 8 words = 64 bytes
// (a ragged last group: the words below cw).  Every output word is stored, the zero tails included: no memset before it.
// Workgroup ids run over w fastest, so that the workgroups that read the same rows (each uses 4 of a row's bytes) are
// resident together and share the rows' lines in L2.  LDS 2 KiB.
//
// igd_bitrows_gram.  out[i * ldo + j] += popc(A_i & B_j) for A = m rows, B = n rows of `stride` uint64 words each, over the
// words [0, nwords).  A workgroup of 256 threads owns a tile of IGD_GRAM_TILE x IGD_GRAM_TILE = 64 x 64 outputs and one
// SLICE of the word range; thread (tx, ty) = (t & 15, t >> 4) owns the 4 x 4 cells (ty + 16 a, tx + 16 b).  Per K-step of
// IGD_GRAM_KSTEP = 16 words the two row tiles (rows past the edge and words past the slice as 0) are staged in LDS, the
// next step's words being loaded into registers while this one is counted.  Per word a thread reads 4 + 4 operands
// (ds_read_b64) and per cell does two ANDs and two accumulating bit counts (v_bcnt_u32_b32 with its addend): 64 vector
// instructions per 8 LDS reads -- the kernel is bound by VECTOR ISSUE, not by memory: a tile reads 2 x 64 rows once per
// 4 096 cells.
//   LDS      2 tiles x 64 rows x (16 + 1) words x 8 B = 17 408 B.  The row stride of 17 words is odd: the 16 rows tx + 16 b
//            that the lanes of a half-wave read lie 17 words = 34 dwords apart, so their 64-bit words fall on 16 different
//            bank pairs of the 64-dword modulus of ds_read_b64; the A operand is one address per 16 lanes (broadcast).
//   32 bits  a cell gains at most 64 per word; a slice is at most IGD_GRAM_SLICE_MAX = 2^25 words (host), 2^31 per cell.
//   slices   the host cuts the word range so that tiles x slices fill the device (igd_hip_gram_slices); blockIdx.y is the
//            slice.  Every workgroup ADDS its cells into out with 64-bit device-scope atomics that return nothing
//            (global_atomic_add_x2), zero cells skipped: out is zeroed (generic entry) or carried over chunks (co-occurrence)
//            by the host.
//   SYM      B == A: only tiles ti <= tj are launched (blockIdx.x numbers them row by row); a tile off the diagonal also adds
//            its cells to the mirror positions out[j * ldo + i]; a diagonal tile computes all its 64 x 64 cells and adds
//            each once.
// All stores to memory are vector stores or vector atomics.
#define IGD_TR_BLOCKS 8                              // 64-row blocks per workgroup of igd_bits_transpose: runs of 64 bytes per column
#define IGD_GRAM_TILE 64                             // output tile edge
#define IGD_GRAM_KSTEP 16                            // 64-bit words per row and K-step
#define IGD_GRAM_LDS_STRIDE (IGD_GRAM_KSTEP + 1)     // odd: see LDS above
#define IGD_GRAM_SLICE_MAX ((int64_t)1 << 25)        // words per slice: 64 x 2^25 = 2^31 fits a 32-bit accumulator
#define IGD_GRAM_TARGET 2048                         // workgroups wanted in flight (8 per CU of the MI355X's 256)
#define IGD_GRAM_SLICE_MIN 64                        // words: a slice below four K-steps is dominated by its 4 096 atomics

__global__ __launch_bounds__(IGD_SETS_WG) void igd_bits_transpose(const unsigned *__restrict__ bits, int64_t n, int nW, int64_t cw,
                                                                 u64 *__restrict__ cols)
{
    __shared__ u64 tile[32 * IGD_TR_BLOCKS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = (int)(blockIdx.x % (unsigned)nW);
    const int64_t b0 = (int64_t)(blockIdx.x / (unsigned)nW) * IGD_TR_BLOCKS;         // this workgroup's first 64-row block
    for (int k = wave; k < IGD_TR_BLOCKS; k += IGD_SETS_WG / IGD_WAVE) {
        const int64_t r = (b0 + k) * 64 + lane;
        const unsigned x = r < n ? bits[(size_t)r * (size_t)nW + (size_t)w] : 0u;
        u64 mine = 0;
#pragma unroll
        for (int j = 0; j < 32; j++) {
            const u64 bal = __ballot((x >> j) & 1u);
            if (lane == j) mine = bal;
        }
        if (lane < 32) tile[lane * IGD_TR_BLOCKS + k] = mine;
    }
    __syncthreads();
    const int c = (int)(threadIdx.x >> 3), k = (int)(threadIdx.x & 7);               // 256 threads = 32 columns x 8 words
    if (b0 + k < cw) cols[((size_t)w * 32 + (size_t)c) * (size_t)cw + (size_t)(b0 + k)] = tile[c * IGD_TR_BLOCKS + k];
}

template <bool SYM>
__global__ __launch_bounds__(IGD_SETS_WG) void igd_bitrows_gram(const u64 *__restrict__ A, int64_t m, const u64 *__restrict__ B, int64_t n,
                                                               int64_t stride, int64_t nwords, int64_t sliceLen, int tilesN,
                                                               u64 *__restrict__ out, int64_t ldo)
{
    __shared__ u64 sA[IGD_GRAM_TILE * IGD_GRAM_LDS_STRIDE];
    __shared__ u64 sB[IGD_GRAM_TILE * IGD_GRAM_LDS_STRIDE];
    // the tile: (ti, tj) of the rectangular grid, or the blockIdx.x-th pair ti <= tj of the symmetric one (tilesN per side)
    int ti, tj;
    if (SYM) {
        int p = (int)blockIdx.x;
        ti = 0;
        while (p >= tilesN - ti) { p -= tilesN - ti; ti++; }
        tj = ti + p;
    } else {
        ti = (int)(blockIdx.x / (unsigned)tilesN);
        tj = (int)(blockIdx.x % (unsigned)tilesN);
    }
    const int64_t i0 = (int64_t)ti * IGD_GRAM_TILE, j0 = (int64_t)tj * IGD_GRAM_TILE;
    const int64_t k0 = (int64_t)blockIdx.y * sliceLen;
    const int64_t k1 = k0 + sliceLen < nwords ? k0 + sliceLen : nwords;
    const int tx = threadIdx.x & 15, ty = (int)(threadIdx.x >> 4);
    // staging: thread t moves word t & 15 of the rows (t >> 4) + 16 a of both tiles
    u64 ra[4], rb[4];
    auto fetch = [&](int64_t kb) {
        const int64_t kw = kb + tx;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int64_t ia = i0 + ty + 16 * a, jb = j0 + ty + 16 * a;
            ra[a] = (kw < k1 && ia < m) ? A[(size_t)ia * (size_t)stride + (size_t)kw] : 0;
            rb[a] = (kw < k1 && jb < n) ? B[(size_t)jb * (size_t)stride + (size_t)kw] : 0;
        }
    };
    unsigned acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0;
    if (k0 < k1) fetch(k0);
    for (int64_t kb = k0; kb < k1; kb += IGD_GRAM_KSTEP) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            sA[(ty + 16 * a) * IGD_GRAM_LDS_STRIDE + tx] = ra[a];
            sB[(ty + 16 * a) * IGD_GRAM_LDS_STRIDE + tx] = rb[a];
        }
        __syncthreads();
        if (kb + IGD_GRAM_KSTEP < k1) fetch(kb + IGD_GRAM_KSTEP);
#pragma unroll 4
        for (int k = 0; k < IGD_GRAM_KSTEP; k++) {
            u64 va[4], vb[4];
#pragma unroll
            for (int a = 0; a < 4; a++) {
                va[a] = sA[(ty + 16 * a) * IGD_GRAM_LDS_STRIDE + k];
                vb[a] = sB[(tx + 16 * a) * IGD_GRAM_LDS_STRIDE + k];
            }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[a][b] += (unsigned)__popcll(va[a] & vb[b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < m && j < n && acc[a][b]) {
                (void)__hip_atomic_fetch_add(out + (size_t)i * (size_t)ldo + (size_t)j, (u64)acc[a][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (SYM && ti != tj)
                    (void)__hip_atomic_fetch_add(out + (size_t)j * (size_t)ldo + (size_t)i, (u64)acc[a][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
}
