// engine/shift_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_shift_regions: a region set under rigid shifts (igd_hip_shift_support, igd_hip_shift_regions)
// ------------------------------------------------------------------------------------------
// The launch shape and the three outputs of igd_permute_regions (permute_dev.hpp): output t is region i = t % nq under offset
// offsets[j0 + t / nq]; the placement is igd_hip_shift_place of include/igd_hip.h (one add and two clamps in 64 bits), evaluated
// per output.  The offset table (at most IGD_HIP_SHIFT_MAX words) and the contig lengths are read from global memory through the
// cached path: the nq lanes of one shift read the same word.  One output per lane at a time, IGD_SETS_WG threads, at most
// IGD_SETS_GRID persistent workgroups striding over the outputs (t < 2^31: the host cuts).  out_ichr, when given, receives the
// contig numbers once more per shift.  All stores to memory are plain vector stores; nothing is kept in scratch.
__global__ __launch_bounds__(IGD_SETS_WG) void igd_shift_regions(const int32_t *__restrict__ q_ichr, const int32_t *__restrict__ q_qs,
                                                                const int32_t *__restrict__ q_qe, unsigned nq,
                                                                const int32_t *__restrict__ ctg_len, int nctg,
                                                                const int32_t *__restrict__ offsets, unsigned j0, unsigned total,
                                                                int32_t *__restrict__ out_ichr, int32_t *__restrict__ out_qs,
                                                                int32_t *__restrict__ out_qe)
{
    const unsigned stride = gridDim.x * IGD_SETS_WG;
    for (unsigned t = blockIdx.x * IGD_SETS_WG + threadIdx.x; t < total; t += stride) {
        const unsigned j = t / nq, i = t - j * nq;
        const int32_t c = q_ichr[i];
        int32_t s = q_qs[i], e = q_qe[i];
        igd_hip_shift_place(offsets[j0 + j], c, ctg_len, nctg, &s, &e);
        if (out_ichr) out_ichr[t] = c;
        out_qs[t] = s;
        out_qe[t] = e;
    }
}
