// engine/permute_bp_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_merge_row_offsets, igd_merge_slices, igd_merge_row_bp: the resident hand-over from the merge launches (merge_dev.hpp) to
// igd_sets_coverage (coverage_dev.hpp), for igd_hip_permute_bp (host_permute_bp.hpp; the definitions are in include/igd_hip.h)
// ------------------------------------------------------------------------------------------
// The merge leaves the runs of `rows` rows in one array, row r at [m_off[r], m_off[r + 1]), and only the device knows m_off.
// The coverage kernel wants a slice table {row, a, b} that the host has always cut, because the host knew the offsets.  Here
// the host knows an upper bound instead -- a row of nq regions has at most nq runs -- so every row gets the SAME number of
// slice slots, perRow = ceil(nq / sliceLen), and the table has rows * perRow entries whatever the merge found: its length,
// the grid and the workspace are known without a read-back.
//
// igd_merge_slices fills slot j of row r with
//     a = min(m_off[r] + j * sliceLen, m_off[r + 1]),  b = min(a + sliceLen, m_off[r + 1]).
// A slot behind the row's last run has a == b.  igd_sets_coverage takes such a slice as it takes any other: its query loop
// `for (q = sl.a + wave; q < sl.b; ..)` has no turn, every lane's sum stays 0, and the flush at the slice's end adds only
// non-zero counters and a non-zero total -- so an empty slot reads no run, writes nothing, and only sl.row (a valid row) is
// used to form a pointer.  No slot reaches into the next row's runs: both ends are capped at m_off[r + 1].
// a and b are positions in the run arrays of one chunk, below 2^31 (the chunk holds at most igd_hip_max_batch() regions).
//
// igd_merge_row_bp: one wave per row; the lanes stride over the row's runs, each adds qe - qs in 64 bits (a row of 2^26 runs
// of up to 2^31 bp passes 32 bits at once), a butterfly over the wave brings the sum to every lane, lane 0 stores it and the
// number of runs.  Rows are independent: no atomics, no LDS.
// Occupancy: the three kernels keep a handful of registers and no LDS; they are launch-bound (a few hundred rows, a few
// thousand slots), so the workgroup is IGD_MERGE_WG as for the other merge kernels and the grid is cut the same way.
// All stores to memory are vector stores.

// set_off[r] = r * nq, r = 0 .. rows: the regular offsets of a chunk of permutations
static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_row_offsets(int64_t nq, int64_t rows, int64_t *__restrict__ set_off)
{
    for (int64_t r = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; r <= rows; r += (int64_t)gridDim.x * IGD_MERGE_WG) set_off[r] = r * nq;
}

static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_slices(const int64_t *__restrict__ m_off, int64_t rows, int64_t perRow,
                                                                       int64_t sliceLen, SetSlice *__restrict__ slices)
{
    const int64_t total = rows * perRow;
    for (int64_t t = (int64_t)blockIdx.x * IGD_MERGE_WG + threadIdx.x; t < total; t += (int64_t)gridDim.x * IGD_MERGE_WG) {
        const int64_t r = t / perRow, j = t - r * perRow;
        const int64_t end = m_off[r + 1];
        int64_t a = m_off[r] + j * sliceLen;
        a = a < end ? a : end;
        const int64_t b = a + sliceLen < end ? a + sliceLen : end;
        slices[t] = SetSlice{(int32_t)r, (int32_t)a, (int32_t)b, 0};
    }
}

static __global__ void __launch_bounds__(IGD_MERGE_WG) igd_merge_row_bp(const int32_t *__restrict__ m_qs, const int32_t *__restrict__ m_qe,
                                                                       const int64_t *__restrict__ m_off, int64_t rows,
                                                                       int64_t *__restrict__ set_bp, int64_t *__restrict__ n_merged)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t waves = IGD_MERGE_WG / WAVE;
    for (int64_t r = (int64_t)blockIdx.x * waves + threadIdx.x / WAVE; r < rows; r += (int64_t)gridDim.x * waves) {
        const int64_t a = m_off[r], b = m_off[r + 1];
        u64 bp = 0;
        for (int64_t i = a + lane; i < b; i += WAVE) bp += (u64)((int64_t)m_qe[i] - (int64_t)m_qs[i]);
        for (int d = WAVE / 2; d > 0; d >>= 1) bp += __shfl_xor(bp, d, WAVE);
        if (lane == 0) {
            set_bp[r] = (int64_t)bp;
            n_merged[r] = b - a;
        }
    }
}
