// beta_marginals.hip -- per-pixel marginals of the Beta output head, the reference's DEFAULT output distribution (CT_VAE.pixel_dist,
// ctvae/main_ct_vae.py:648-731: output_dist_vec[s].sample(100) on a tfd.Beta): for decoder outputs alpha, beta [n][pix] and K draws,
// the histogram, the sum and the sum of squares of the n * K samples of every pixel, accumulated into caller-owned state.  No sample is
// written to memory.
//
// Sample (o, pixel, k) IS the x that ctpvae_beta_head_fwd_f32 writes for object o and that pixel with draw = draw0 + k and the same
// seed and first_object: beta_head.h's beta_prep / beta_draw, the code beta_head.hip runs -- e = (first_object + o) * pix + pixel, one
// Philox block per (pixel, gamma, attempt) under kBetaTag, at most 16 attempts, the gammas in log space, x = 1 / (1 + exp(lg_1 -
// lg_0)) unclamped (sqrt_reg plays no part in x).  y, the clamps, lp and its three lgamma are not evaluated.  A NaN alpha or beta gives
// a NaN x for that pixel (16 refused attempts, as in the head): it counts in column 0 and makes that pixel's s1, s2 NaN; no other
// pixel is touched.
//
// The bin rule, the state, the cut of the draws into units of 25, the launch shape, the counts and the fixed order of the float64 sums
// are marginals.hip's (its header states them), through marginals.h: the same code.  Per unit a thread evaluates beta_prep of its quad
// once -- the two expf per pixel and cb, d, s, log(d) per gamma: once per pixel, object and slice of 25 draws, not once per sample --
// and per draw beta_draw of each pixel: the attempt loop, log(v) and the boost.
//
// Divergence: the attempt loop (#pragma unroll 1, as in the head) diverges per lane.  An attempt is refused with probability at most
// 0.046, so at the worst cells some lane of a 64-lane wave takes a second attempt in most waves (1 - 0.954^64 = 0.95) and the wave
// pays for two; a third is rare (64 * 0.046^2 = 0.13).  Pixels past the end of a ragged quad draw nothing.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in either kernel; registers and occupancy are stated next
// to each kernel.
#include "beta_head.h"
#include "marginals.h"

namespace ctpvae {

struct BetaQuadSampler {
    BetaPrep pr[4];
    __device__ __forceinline__ void prep(const float (&al)[4], const float (&be)[4])
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) pr[q] = beta_prep(al[q], be[q]);
    }
    __device__ __forceinline__ void draw(unsigned long long e, unsigned draw, unsigned k0, unsigned k1, int cnt, float (&x)[4]) const
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = q < cnt ? beta_draw(pr[q], e + q, draw, k0, k1).x : 0.0f;
    }
};

// 127 VGPRs (the four pixels' preps are 32 of them, the eight float64 partial sums 16), no scratch: 4 waves per SIMD by registers, i.e.
// four 256-thread workgroups per CU; the dynamic LDS (16 KiB + 256 (bins + 2) B) allows five at 50 bins and two at 254
__global__ __launch_bounds__(kMargThreads) void beta_marginals_kernel(const float *__restrict__ alpha, const float *__restrict__ beta,
                                                                      MargShape sh, int ptr_aligned, unsigned long long *__restrict__ hist,
                                                                      double *__restrict__ ws)
{
    extern __shared__ __align__(16) unsigned char marg_lds[];
    marg_workgroup<BetaQuadSampler>(alpha, beta, sh, ptr_aligned, hist, ws, marg_lds);
}

// 8 VGPRs, no scratch: 8 waves per SIMD
__global__ __launch_bounds__(kMargThreads) void beta_marginals_finish_kernel(const double *__restrict__ ws, int pix, int groups,
                                                                             double *__restrict__ s1, double *__restrict__ s2)
{
    marg_finish(ws, pix, groups, s1, s2);
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

long long ctpvae_beta_marginals_workspace_bytes(int n, int pix, unsigned draws)
{
    if (int rc = marg_check("beta_marginals_workspace_bytes", n, pix, draws)) return rc;
    return (long long)marg_groups(n, draws) * 2 * pix * (long long)sizeof(double);
}

int ctpvae_beta_marginals_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                              unsigned long long seed, unsigned draw0, unsigned draws, float lo, float width, int bins,
                              long long *hist_dev, double *s1_dev, double *s2_dev, void *workspace_dev, ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    MargShape sh;
    if (int rc = marg_launch_shape("beta_marginals", alpha_dev, beta_dev, n, pix, first_object, seed, draw0, draws, lo, width, bins, hist_dev,
                                   s1_dev, s2_dev, workspace_dev, sh))
        return rc;
    const int aligned = head_aligned16({alpha_dev, beta_dev}) ? 1 : 0;
    CTPVAE_SET_MAX_LDS_ONCE(beta_marginals_kernel, attr_set);
    hipLaunchKernelGGL(beta_marginals_kernel, dim3(ceil_div(pix, kMargTilePix), sh.groups), dim3(kMargThreads), marg_lds_bytes(bins),
                       (hipStream_t)stream, alpha_dev, beta_dev, sh, aligned, reinterpret_cast<unsigned long long *>(hist_dev),
                       static_cast<double *>(workspace_dev));
    CTPVAE_LAUNCH_CHECK("beta_marginals_kernel");
    hipLaunchKernelGGL(beta_marginals_finish_kernel, dim3(marg_finish_blocks(pix)), dim3(kMargThreads), 0, (hipStream_t)stream,
                       static_cast<const double *>(workspace_dev), pix, sh.groups, s1_dev, s2_dev);
    CTPVAE_LAUNCH_CHECK("beta_marginals_finish_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
