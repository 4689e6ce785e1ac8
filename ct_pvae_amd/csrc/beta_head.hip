// beta_head.hip -- the P-VAE decoder's DEFAULT output head, tfd.Beta(positive_range(alpha), positive_range(beta))
// (ctvae/helper_functions.py:275-285; ct_pvae_amd/trainer.py positive_range / Beta.rsample / clamp / .log_prob) as ONE forward and
// ONE backward launch: the reparameterised sample of every pixel, its log-density at the clamped sample and the per-object sum of
// the log-densities; the backward gives what TensorFlow's tape gives on that composition.
//
// The function, per pixel, fp32 (EPS = FLT_EPSILON; sr = sqrt_reg, an argument, 0 < sr < 0.5; hi = 1 - sr in fp32):
//   pr(t) = t >= 1 ? t : exp(t - 1) + EPS;      a = pr(alpha), b = pr(beta)                       (quad_io.h's positive_range)
//   for the two gammas j = 0 (c = a) and j = 1 (c = b):
//       cb = c < 1 ? c + 1 : c;   d = cb - 1/3;   s = 1 / sqrt(9 d)                         (Marsaglia-Tsang, boosted below 1)
//       attempts k = 0 .. 15:   block = Philox4x32-10((lo32(e), hi32(e), draw, kBetaTag | j << 8 | k), key = seed)
//           zn = ndtri(u24(word 0)),  ua = u24(word 1),  ub = u24(word 2)            (u24(w) = ((w >> 8) + 0.5f) 2^-24, tn_head.h's)
//           w = 1 + s zn;  v = w^3;   accept iff w > 0 and log(ua) < ((0.5 zn^2 + d) - d v) + d log(v)
//       the first accepted attempt is taken; after 16 refusals attempt 15 is taken (v = 1 if its w <= 0)
//       lg_j = (log(d) + log(v)) + (c < 1 ? log(ub) / c : 0)                                (the gamma sample stays in LOG space)
//   x  = 1 / (1 + exp(lg_1 - lg_0))             (what goes to the projector, not clamped; may round to 0 or 1)
//   y  = 1 / (1 + exp(lg_0 - lg_1))             (1 - x without cancellation)
//   xc = clamp(x, sr, hi);   yc = hi where x < sr, 1 - hi where x > hi, y otherwise;  x > hi is tested as y < 1 - hi (next to 1 x has
//                            lost the relative accuracy that y keeps: at sr = EPS the fp32 x = hi covers y from 0.5 to 1.5 sr)
//   lp = ((a - 1) log(xc) + (b - 1) log(yc)) - ((lgamma(a) + lgamma(b)) - lgamma(a + b))
// The attempt loop is bounded by construction (kBetaAttempts = 16): the refusal probability of an attempt is at most 0.046 for
// concentrations from 1e-7 to 40, so the cap binds with probability < 1e-21; NaN operands refuse every attempt and leave after 16 (a NaN
// alpha or beta gives a NaN x for that pixel and a NaN LP for its object; no other object is touched).  Log space (TensorFlow
// Probability's Beta sampler: log-space gammas, a sigmoid of their difference) keeps concentrations down to EPS finite: log(ub) / c
// is about -1e7 there and x saturates.
//
// The backward, for the cotangents g_x (per pixel) and G = g_LP[object]: the IMPLICIT reparameterisation gradient of each gamma
// (what TensorFlow's tape gives; torch's Beta.rsample uses another, equally unbiased estimator that differs per sample):
//   dlg_j   = d lg_j / d c = -(dP(c, g) / dc) / (g p(g; c)) at g = exp(lg_j)   (P: regularised lower incomplete gamma, p: density)
//   dx/da   = x y dlg_0,   dx/db = -x y dlg_1
//   gx0     = g_x + [sr <= x and 1 - hi <= y] G ((a - 1) / xc - (b - 1) / yc)
//   g_a     = gx0 dx/da + G ((log xc - digamma(a)) + digamma(a + b)),    g_b alike with log yc and digamma(b)
//   g_alpha = g_a pr'(alpha),   g_beta = g_b pr'(beta),   pr'(t) = t >= 1 ? 1 : exp(t - 1)
// Nothing is saved for it: it redraws and re-evaluates the pixel from alpha, beta with the forward's own code (the same fp32
// operations, so the same accepted attempts and the same clamp decisions).  ARITHMETIC: the forward is fp32 throughout; the backward
// takes the forward's fp32 a, b, lg_j, x, y, xc, yc and evaluates dlg, the digammas and the combination above in FLOAT64, rounding
// g_alpha and g_beta once.  Why: dlg is a sum of up to 9 sqrt(c) terms whose two halves (log g - digamma) S and dS/dc are each of
// the size of the result times sqrt(c), and digamma(a) - digamma(a + b) cancels for a >> b; in fp32 the honest bar of that is tens
// of ulps and grows with c, in fp64 its rounding (2^-53 times the number of terms) disappears under the fp32 rounding of the operands.
// fp64 throughput is not what bounds this kernel.  beta_head.h states the series, the continued fraction and the digamma;
// their iteration count is bounded by kDlgMaxTerms = 2048 (the series needs about 9.5 sqrt(c) terms for 1e-17, the continued fraction
// fewer: the bound is reached only beyond c ~ 4e4, and a sum that has not converged there gives a NaN gradient for that pixel, not a
// truncated value; no asymptotic form is switched to, so the bar has no truncation term).
//
// Random numbers: ONE Philox block per (pixel, gamma, attempt).  Pixel `pixel` of object o has the 64-bit flat index
// e = (first_object + o) * pix + pixel; the draws depend on (seed, draw, e) alone, so a batch cut into calls (or ranks) with
// first_object draws what the whole batch draws.  kBetaTag = 0x42000000u (in use elsewhere: 0x544E48, 0x484D43, 0x4C000000 | ..,
// 0x44000000 | .., 0x51000000 | .. -- beta_latent.hip's, which runs this sampler under its own fourth counter word --, 0).
//
// Layout and the order of the per-object sum LP[o]: quad_io.h states them (head_fwd_body, head_bwd_body) -- one workgroup of 1024
// threads per object, no atomics, the same bits whatever n, first_object and the object's alignment in memory are; the backward has
// no sum and walks the n * pix pixels as memory quads, 256 threads per workgroup.
//
// Resources: no scratch and no VGPR spills in either kernel, 5 waves per SIMD each (profiles/sampling_refactor_resources.txt); a forward
// workgroup is 4 waves per SIMD, so one per CU at a time; the backward runs five 256-thread workgroups per CU.
#include "beta_head.h"

namespace ctpvae {

static_assert(kBetaTag == 0x42000000u, "kBetaTag = 0x42000000u is part of the stream's definition (include/ctpvae_radon.h)");

__global__ __launch_bounds__(kObjectSumThreads) void beta_head_fwd_kernel(const float *__restrict__ alpha, const float *__restrict__ beta,
                                                                          int pix, QuadRng rng, float sr, int ptr_aligned,
                                                                          float *__restrict__ x_out, float *__restrict__ lp_sum,
                                                                          float *__restrict__ lp_elem, float *__restrict__ aux)
{
    head_fwd_body(alpha, beta, pix, ptr_aligned, x_out, lp_sum, lp_elem,
                  [&](const float (&al)[4], const float (&be)[4], size_t i, int cnt, bool, float (&x)[4], float (&lp)[4]) {
#pragma unroll
                      for (int j = 0; j < 4; ++j) {
                          const BetaPixel px = beta_pixel<false>(al[j], be[j], rng.first + i + j, rng.draw, rng.k0, rng.k1, sr);
                          x[j] = px.x, lp[j] = px.lp;
                          if (aux != nullptr && j < cnt) {
                              float *w = aux + 8 * (i + j);
                              w[0] = px.g0.zn, w[1] = px.g0.ub, w[2] = (float)px.g0.k, w[3] = px.g0.lg;
                              w[4] = px.g1.zn, w[5] = px.g1.ub, w[6] = (float)px.g1.k, w[7] = px.g1.lg;
                          }
                      }
                  });
}

// (the float64 loops diverge per lane: occupancy hides them)
__global__ __launch_bounds__(kQuadBwdThreads) void beta_head_bwd_kernel(const float *__restrict__ alpha, const float *__restrict__ beta,
                                                                        long long total, int pix, QuadRng rng, float sr, int ptr_aligned,
                                                                        const float *__restrict__ g_x, const float *__restrict__ g_lp,
                                                                        float *__restrict__ g_alpha, float *__restrict__ g_beta)
{
    head_bwd_body(alpha, beta, total, pix, ptr_aligned, g_x, g_lp, g_alpha, g_beta,
                  [&](const float (&al)[4], const float (&be)[4], size_t i, int, bool, const float (&gx)[4], const float (&G)[4],
                      float (&ga)[4], float (&gb)[4]) {
#pragma unroll
                      for (int j = 0; j < 4; ++j) {
                          const BetaPixel px = beta_pixel<true>(al[j], be[j], rng.first + i + j, rng.draw, rng.k0, rng.k1, sr);
                          beta_pixel_grad(px, gx[j], G[j], ga[j], gb[j]);
                      }
                  });
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_beta_head_fwd_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                             unsigned long long seed, unsigned draw, float sqrt_reg, float *x_out_dev, float *lp_sum_out_dev,
                             float *lp_elem_out_dev, float *aux_out_dev, ctpvae_stream_t stream)
{
    if (int rc = beta_head_check("beta_head_fwd", alpha_dev, beta_dev, n, pix, first_object, sqrt_reg)) return rc;
    CTPVAE_REQUIRE(x_out_dev && lp_sum_out_dev, "beta_head_fwd: null output pointer");
    const QuadRng rng = quad_rng(first_object, pix, seed, draw);
    const int aligned = head_aligned16({alpha_dev, beta_dev, x_out_dev, lp_elem_out_dev}) ? 1 : 0;
    hipLaunchKernelGGL(beta_head_fwd_kernel, dim3(n), dim3(kObjectSumThreads), 0, (hipStream_t)stream, alpha_dev, beta_dev, pix, rng,
                       sqrt_reg, aligned, x_out_dev, lp_sum_out_dev, lp_elem_out_dev, aux_out_dev);
    CTPVAE_LAUNCH_CHECK("beta_head_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_beta_head_bwd_f32(const float *alpha_dev, const float *beta_dev, int n, int pix, long long first_object,
                             unsigned long long seed, unsigned draw, float sqrt_reg, const float *g_x_dev, const float *g_lp_dev,
                             float *g_alpha_out_dev, float *g_beta_out_dev, ctpvae_stream_t stream)
{
    if (int rc = beta_head_check("beta_head_bwd", alpha_dev, beta_dev, n, pix, first_object, sqrt_reg)) return rc;
    CTPVAE_REQUIRE(g_alpha_out_dev && g_beta_out_dev, "beta_head_bwd: null output pointer");
    const QuadRng rng = quad_rng(first_object, pix, seed, draw);
    const int aligned = head_aligned16({alpha_dev, beta_dev, g_x_dev, g_alpha_out_dev, g_beta_out_dev}) ? 1 : 0;
    const long long total = (long long)n * pix;
    hipLaunchKernelGGL(beta_head_bwd_kernel, dim3(head_bwd_grid(total)), dim3(kQuadBwdThreads), 0, (hipStream_t)stream, alpha_dev, beta_dev, total, pix, rng,
                       sqrt_reg, aligned, g_x_dev, g_lp_dev, g_alpha_out_dev, g_beta_out_dev);
    CTPVAE_LAUNCH_CHECK("beta_head_bwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_beta_head_words_host_u32(int n, int pix, long long first_object, unsigned long long seed, unsigned draw, int gamma,
                                    int attempt, unsigned *out_host)
{
    CTPVAE_REQUIRE(out_host, "beta_head_words_host: null pointer");
    if (int rc = head_size_check("beta_head_words_host", n, pix, first_object)) return rc;
    CTPVAE_REQUIRE(gamma >= 0 && gamma <= 1 && attempt >= 0 && attempt < kBetaAttempts,
                   "beta_head_words_host: gamma must be 0 or 1 and 0 <= attempt < 16 (got %d, %d)", gamma, attempt);
    const QuadRng rng = quad_rng(first_object, pix, seed, draw);
    const long long total = (long long)n * pix;
    for (long long i = 0; i < total; ++i) {
        const Philox4 b = beta_block(rng.first + (unsigned long long)i, draw, (unsigned)gamma, (unsigned)attempt, rng.k0, rng.k1);
        for (int w = 0; w < 4; ++w) out_host[4 * i + w] = b.w[w];
    }
    return CTPVAE_OK;
}

}  // extern "C"
