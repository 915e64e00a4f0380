// engine/permute_ws_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_permute_workspace: region sets placed inside a workspace (mode IGD_HIP_PERM_WORKSPACE of the three permutation nulls)
// ------------------------------------------------------------------------------------------
// The launch shape and the three outputs of igd_permute_regions (permute_dev.hpp): output t is region i = t % nq under
// permutation p0 + t / nq, IGD_SETS_WG threads, igd_hip_permute_grid workgroups striding over the outputs.  The placement is
// igd_hip_perm_place_ws of include/igd_hip.h, evaluated per output: the table (w_off, w_start, w_len, w_pre) is read from device
// memory -- a workspace of 10^5 segments is 1.2 MB and stays in the L2 -- by two binary searches of at most 32 steps each, the
// first over the descending lengths of the region's contig, the second over the prefix sums of the segments it fits in.  The
// host has run igd_hip_workspace_valid over the table before it is uploaded, so every index is inside the four arrays and
// every output on its contig.  No atomics, no LDS; all stores to memory are vector stores.
__global__ __launch_bounds__(IGD_SETS_WG) void igd_permute_workspace(const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                                    const int32_t *__restrict__ q_qe, unsigned nq,
                                                                    const int32_t *__restrict__ ctg_len, int nctg,
                                                                    const int64_t *__restrict__ w_off, const int32_t *__restrict__ w_start,
                                                                    const int32_t *__restrict__ w_len, const int32_t *__restrict__ w_pre,
                                                                    u64 seed, u64 p0, unsigned total, int32_t *__restrict__ out_ichr,
                                                                    int32_t *__restrict__ out_qs, int32_t *__restrict__ out_qe)
{
    const unsigned stride = gridDim.x * IGD_SETS_WG;
    for (unsigned t = blockIdx.x * IGD_SETS_WG + threadIdx.x; t < total; t += stride) {
        const unsigned p = t / nq, i = t - p * nq;
        const int32_t c = q_ichr[i];
        int32_t s = q_qs[i], e = q_qe[i];
        (void)igd_hip_perm_place_ws(igd_hip_perm_base(seed, p0 + p), c, (int64_t)i, ctg_len, nctg, w_off, w_start, w_len, w_pre, &s, &e);
        if (out_ichr) out_ichr[t] = c;
        out_qs[t] = s;
        out_qe[t] = e;
    }
}
