// marginals.hip -- per-pixel marginals of the TruncatedNormal output head (the reference's CT_VAE.pixel_dist, ctvae/main_ct_vae.py:648-731):
// for decoder outputs alpha, beta [n][pix] and K draws, the histogram, the sum and the sum of squares of the n * K samples of every
// pixel, accumulated into caller-owned state.  No sample is written to memory: it is drawn, binned and added in registers / LDS.
//
// Sample (o, pixel, k) IS the x that ctpvae_tn_head_fwd_f32 writes for object o and that pixel with draw = draw0 + k and the same seed
// and first_object: tn_head.h's tn_prep / tn_draw on the uniform of head_uniforms4 (word e & 3 of the block of e = (first_object + o) *
// pix + pixel), the code head.hip runs.  The lp terms are not evaluated.
//
// Bin of a sample, fp32 (marginals_bin, host and device; ctpvae_tn_marginals_bin_host_f32 applies it to an array):
//   t = (x - lo) / width         one subtraction, one correctly rounded division
//   column 0 if !(t >= 0) (NaN too), column bins + 1 if t >= bins, else column 1 + (int)t
//
// State: hist [pix][bins + 2] int64, s1, s2 [pix] float64 (sum of the samples and of their squares, each fp32 sample widened to double
// first; the square of a float is exact in double).  All n objects add into the same pix rows.  A launch ADDS to the state.
//
// Layout.  The draws 0 .. K-1 are cut into S = ceil(K / 25) slices of kMargSlice = 25 consecutive draws (the last may be shorter; 25
// divides the reference's 100 draws per decoder output).  Unit j = o * S + s is slice s of object o, n * S units in all.  A workgroup
// of 256 threads covers a tile of 16 quads = 64 pixels (grid x) and has 16 unit lanes: thread t = 16 * lane + quad.  There are
// G = min(ceil(n * S / 16), kMargMaxGroups = 64) workgroups per tile (grid y); lane l of group g takes the units
//   j = 16 g + l,  16 (g + G) + l,  16 (g + 2 G) + l, ...                                       (ascending)
// and walks the draws of each ascending.  Per unit it loads its quad of alpha, beta and evaluates tn_prep once (so the part that
// does not depend on u is evaluated once per pixel, object and slice of 25 draws, not once per sample); per draw it takes one Philox
// block for the quad when the quad is whole-block aligned ((first_object + o) * pix a multiple of 4), two otherwise.
//
// Counts: one LDS add per sample into the workgroup's [64][bins + 2] 32-bit image (n * K < 2^32, so it cannot wrap), then at most one
// 64-bit integer atomic add per pixel, column and workgroup into hist, zeros skipped.  Integer addition commutes: any order, same bits.
//
// The float64 sums, in this fixed order and with no floating-point atomics (s1 shown; s2 alike with the squares):
//   thread (g, l), pixel p:  P_gl = (((0 + x_1) + x_2) + ...)      its samples of p in the order it draws them (units ascending as
//                                                                  above, draws ascending inside a unit); a thread without samples: 0
//   workgroup g:             W_g  = ((P_g0 + P_g1) + ...) + P_g15  lanes ascending, through LDS
//   launch:                  T    = ((W_0 + W_1) + ...) + W_(G-1)  groups ascending, by a second kernel from the workspace [G][2][pix]
//   state:                   s1[p] = s1[p] + T
// The workspace is G * 2 * pix doubles: at most 64 * 16 * pix bytes whatever K is.
//
// marginals.h holds all of the above but the sampler (beta_marginals.hip runs the same code on the Beta head's samples).
#include "marginals.h"

namespace ctpvae {

struct TnQuadSampler {
    TnPrep pr[4];
    __device__ __forceinline__ void prep(const float (&al)[4], const float (&be)[4])
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) pr[q] = tn_prep(al[q], be[q]);
    }
    __device__ __forceinline__ void draw(unsigned long long e, unsigned draw, unsigned k0, unsigned k1, int cnt, float (&x)[4]) const
    {
        float u[4];
        head_uniforms4(e, draw, k0, k1, u);
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = tn_draw(pr[q], u[q]).x;
    }
};

__global__ __launch_bounds__(kMargThreads) void tn_marginals_kernel(const float *__restrict__ alpha, const float *__restrict__ beta,
                                                                    MargShape sh, int ptr_aligned, unsigned long long *__restrict__ hist,
                                                                    double *__restrict__ ws)
{
    extern __shared__ __align__(16) unsigned char marg_lds[];
    marg_workgroup<TnQuadSampler>(alpha, beta, sh, ptr_aligned, hist, ws, marg_lds);
}

__global__ __launch_bounds__(kMargThreads) void tn_marginals_finish_kernel(const double *__restrict__ ws, int pix, int groups,
                                                                           double *__restrict__ s1, double *__restrict__ s2)
{
    marg_finish(ws, pix, groups, s1, s2);
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

long long ctpvae_tn_marginals_workspace_bytes(int n, int pix, unsigned draws)
{
    if (int rc = marg_check("tn_marginals_workspace_bytes", n, pix, draws)) return rc;
    return (long long)marg_groups(n, draws) * 2 * pix * (long long)sizeof(double);
}

int ctpvae_tn_marginals_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                            unsigned long long seed, unsigned draw0, unsigned draws, float lo, float width, int bins,
                            long long *hist_dev, double *s1_dev, double *s2_dev, void *workspace_dev, ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    MargShape sh;
    if (int rc = marg_launch_shape("tn_marginals", alpha_dev, beta_dev, n, pix, first_object, seed, draw0, draws, lo, width, bins, hist_dev,
                                   s1_dev, s2_dev, workspace_dev, sh))
        return rc;
    const int aligned = head_aligned16({alpha_dev, beta_dev}) ? 1 : 0;
    CTPVAE_SET_MAX_LDS_ONCE(tn_marginals_kernel, attr_set);
    hipLaunchKernelGGL(tn_marginals_kernel, dim3(ceil_div(pix, kMargTilePix), sh.groups), dim3(kMargThreads), marg_lds_bytes(bins),
                       (hipStream_t)stream, alpha_dev, beta_dev, sh, aligned, reinterpret_cast<unsigned long long *>(hist_dev),
                       static_cast<double *>(workspace_dev));
    CTPVAE_LAUNCH_CHECK("tn_marginals_kernel");
    hipLaunchKernelGGL(tn_marginals_finish_kernel, dim3(marg_finish_blocks(pix)), dim3(kMargThreads), 0, (hipStream_t)stream,
                       static_cast<const double *>(workspace_dev), pix, sh.groups, s1_dev, s2_dev);
    CTPVAE_LAUNCH_CHECK("tn_marginals_finish_kernel");
    return CTPVAE_OK;
}

int ctpvae_tn_marginals_bin_host_f32(const float *x_host, long long count, float lo, float width, int bins, int *col_out_host)
{
    CTPVAE_REQUIRE(x_host && col_out_host, "tn_marginals_bin_host: null pointer");
    CTPVAE_REQUIRE(count >= 0, "tn_marginals_bin_host: count must be >= 0 (got %lld)", count);
    if (int rc = marg_grid_check("tn_marginals_bin_host", lo, width, bins)) return rc;
    for (long long i = 0; i < count; ++i) col_out_host[i] = marginals_bin(x_host[i], lo, width, bins);
    return CTPVAE_OK;
}

}  // extern "C"
