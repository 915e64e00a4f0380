// engine/resample_dev.hpp -- part of igd_hip.hip (included there once; not a stand-alone header).
// igd_resample_regions: draws without replacement from a pool of regions (igd_hip_permute_*_rs, igd_hip_resample_regions)
// ------------------------------------------------------------------------------------------
// The launch shape and the three outputs of igd_permute_regions (permute_dev.hpp): output t is draw i = t % nq of permutation
// p0 + t / nq, and that is pool region igd_hip_resample_index(base(seed, p0 + t / nq), i, npool) of include/igd_hip.h (THE DRAW:
// a four-round Feistel network on 2^(2h) >= npool points, walked until it is back below npool), copied as it stands.  No sort
// and no table per permutation: a draw is distinct from the others of its permutation because the network is a bijection.  One
// output per lane at a time, IGD_SETS_WG threads, at most IGD_SETS_GRID persistent workgroups striding over the outputs
// (t < 2^31: the host cuts).  Per output: the base once per change of permutation, the walk (four mix64 per step; fewer than
// four steps on average since the domain is below 4 npool; it diverges within a wave, which is accepted), three gathered loads,
// three plain vector stores.  out_ichr is ALWAYS written: an output's contig is the pool region's.  The hosts refuse nq > npool;
// a draw i >= npool, whose walk need not end, would read pool region i % npool without walking.  No LDS, no atomics, no floating
// point; nothing is kept in scratch.
__global__ __launch_bounds__(IGD_SETS_WG) void igd_resample_regions(const int32_t *__restrict__ pool_ichr, const int32_t *__restrict__ pool_qs,
                                                                   const int32_t *__restrict__ pool_qe, unsigned npool, unsigned nq,
                                                                   u64 seed, u64 p0, unsigned total, int32_t *__restrict__ out_ichr,
                                                                   int32_t *__restrict__ out_qs, int32_t *__restrict__ out_qe)
{
    const unsigned stride = gridDim.x * IGD_SETS_WG;
    const int h = igd_hip_resample_bits(npool);
    unsigned pBase = ~0u;
    u64 base = 0;
    for (unsigned t = blockIdx.x * IGD_SETS_WG + threadIdx.x; t < total; t += stride) {
        const unsigned p = t / nq, i = t - p * nq;
        if (p != pBase) {
            base = igd_hip_perm_base(seed, p0 + p);
            pBase = p;
        }
        const unsigned k = i < npool ? (unsigned)igd_hip_resample_walk(base, i, npool, h) : i % npool;
        out_ichr[t] = pool_ichr[k];
        out_qs[t] = pool_qs[k];
        out_qe[t] = pool_qe[k];
    }
}
