// latent.hip -- the P-VAE's Normal latent block at one skip level (ctvae/helper_functions.py:247-252, :267, :325-327;
// ct_pvae_amd/trainer.py chunk / positive_range / + sqrt_reg / repeat / randn / kl_normal_std and its sum) as ONE forward and ONE
// backward launch: the ns reparameterised samples of every latent element, its KL term against N(0, 1) and the per-object sum of the
// KL terms; the backward gives what autograd gives on that composition.
//
// Input: skip [B][2C][H][W], contiguous, the encoder's output at the level.  Channels 0 .. C-1 are loc, C .. 2C-1 are log_scale: with
// len = C H W, object b's loc is at b * 2 len and its log_scale at b * 2 len + len.  Per element i of object b and sample s, fp32
// (EPS = FLT_EPSILON):
//   pr(t)   = t >= 1 ? t : exp(t - 1) + EPS                         (quad_io.h's positive_range)
//   scale   = pr(log_scale) + sqrt_reg
//   z[s * B + b][i] = loc + scale * eps(s, b, i)                    (sample-major: the layout the decoder is fed)
//   kl[b][i] = 0.5f * (scale * scale + loc * loc - 1.0f) - logf(scale)     (trainer.kl_normal_std, the same association)
//   KL[b]   = sum over i of kl[b][i]
// The backward, for the cotangents g_z [ns * B][len] and G = g_KL[b] (a null pointer: zero):
//   g_loc   = ((0 + g_z[0, b, i]) + g_z[1, b, i]) + ... + G * loc                           (ascending s, then the KL term)
//   g_scale = ((0 + g_z[0] * eps[0]) + g_z[1] * eps[1]) + ... + G * (scale - 1 / scale)
//   g_skip[b][i] = g_loc;   g_skip[b][len + i] = g_scale * (log_scale >= 1 ? 1 : exp(log_scale - 1))
// Nothing is saved for it but the input: it regenerates eps with the forward's own code, so it gets the same bits.
//
// Random numbers: Philox4x32-10 (philox.h), key = seed.  Element i of object b has the 64-bit flat index e = (first_object + b) * len + i
// and takes word e & 3 of the block with counter (lo32(e >> 2), hi32(e >> 2), draw, 0x4C000000 | level << 16 | s), level < 256,
// s < 65536 (the top byte 0x4C keeps the fourth counter word apart from head.hip's 0x544E48, hmc.hip's 0x484D43 and poisson.hip's 0).
// From the word w:
//   k = (w >> 7) & 0xFFFFFF;   t = ((float)k + 0.5f) * 2^-25   in [2^-26, 0.5] (k + 0.5 rounds to 2^24 at the top: t = 0.5 exactly)
//   eps = bit 31 of w set ? normcdfinvf(t) : -normcdfinvf(t)
// -- exactly symmetric and always finite (|eps| <= 5.5): the quantile is always taken from the nearer tail, where t's resolution is
// relative, and no clamp is needed.  eps depends on (seed, draw, level, s, global object, i) alone, so a batch cut over calls or ranks
// with first_object draws what the whole batch draws, for any ns.  A non-null eps_in [ns * B][len] replaces the generator (tests).
//
// Layout and the order of the per-object sum KL[b]: quad_io.h states them (latent_kl_walk, whose pass over a quad also draws and
// stores the quad's ns samples), so KL[b] has the same bits whatever B, first_object and the object's alignment in memory are.  The
// row offsets whose multiple of 4 decides a quad's 16-byte access are 2 b len, 2 b len + len, (s B + b) len and b len.  The backward
// has no sum: 256 threads per workgroup, ceil(quads / 256) workgroups per object.
#include "quad_io.h"

namespace ctpvae {

constexpr unsigned kLatentTag = 0x4C000000u;   // 'L' in the top byte of the fourth counter word; level in bits 16 .. 23, s below
constexpr int kLatentMaxNs = 65535;

// the tail probability of a word: ((w >> 7) & 0xFFFFFF) + 0.5 in units of 2^-25; bit 31 is the sign of the draw
__host__ __device__ inline float latent_tail(unsigned w) { return ((float)((w >> 7) & 0xFFFFFFu) + 0.5f) * 2.98023223876953125e-08f; }

__host__ __device__ inline Philox4 latent_block(unsigned long long blk, unsigned draw, unsigned tag_s, unsigned k0, unsigned k1)
{
    return philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), draw, tag_s, k0, k1);
}

__device__ __forceinline__ float latent_eps(unsigned w)
{
    const float q = normcdfinvf(latent_tail(w));   // <= 0
    return (w >> 31) != 0 ? q : -q;
}

struct LatentRng : QuadRng {
    unsigned tag;                    // kLatentTag | level << 16
    const float *eps_in;             // [ns * B][len] or nullptr
};

// eps of sample s for the four elements e .. e+3 (one block when e is a multiple of 4, two otherwise)
__device__ __forceinline__ void latent_eps4(unsigned long long e, const LatentRng &rng, unsigned s, float (&eps)[4])
{
    const unsigned sh = (unsigned)e & 3u;
    const Philox4 A = latent_block(e >> 2, rng.draw, rng.tag | s, rng.k0, rng.k1);
    Philox4 B = A;
    if (sh != 0) B = latent_block((e >> 2) + 1, rng.draw, rng.tag | s, rng.k0, rng.k1);
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) eps[j] = latent_eps(sh + j < 4 ? philox_word(A, sh + j) : philox_word(B, sh + j - 4));
}

// the draws of sample s for the quad at r of object b (its row of a [ns * B][len] array starts at `row`): drawn, or loaded from eps_in
__device__ __forceinline__ void latent_quad_eps(const LatentRng &rng, const LatentRows &w, size_t row, int r, int cnt, bool vec_z, int s,
                                                float (&eps)[4])
{
    if (rng.eps_in != nullptr) quad_load(rng.eps_in, row + r, cnt, vec_z, 0.0f, eps);
    else latent_eps4(rng.first + w.el0 + r, rng, (unsigned)s, eps);
}

__global__ __launch_bounds__(kObjectSumThreads) void latent_fwd_kernel(const float *__restrict__ skip, int B, int len, int ns, float sqrt_reg,
                                                                       LatentRng rng, int ptr_aligned, float *__restrict__ z_out,
                                                                       float *__restrict__ kl_sum, float *__restrict__ kl_elem,
                                                                       float *__restrict__ eps_out)
{
    const int b = blockIdx.x;
    latent_kl_walk(skip, b, len, ptr_aligned, 0.0f, kl_sum, kl_elem,
                   [&](const LatentRows &w, int r, int cnt, const float (&loc)[4], const float (&ls)[4], float (&kl)[4]) {
                       float scale[4], unused;
#pragma unroll
                       for (int j = 0; j < 4; ++j) {
                           scale[j] = positive_range(ls[j], unused) + sqrt_reg;
                           kl[j] = 0.5f * (scale[j] * scale[j] + loc[j] * loc[j] - 1.0f) - logf(scale[j]);
                       }
                       for (int s = 0; s < ns; ++s) {        // the quad's samples, in the same pass
                           const size_t row = ((size_t)s * B + b) * (size_t)len;
                           const bool vec_z = w.al && (row & 3) == 0;
                           float eps[4], z[4];
                           latent_quad_eps(rng, w, row, r, cnt, vec_z, s, eps);
#pragma unroll
                           for (int j = 0; j < 4; ++j) z[j] = loc[j] + scale[j] * eps[j];
                           quad_store(z_out, row + r, cnt, vec_z, z);
                           if (eps_out != nullptr) quad_store(eps_out, row + r, cnt, vec_z, eps);
                       }
                   });
}

__global__ __launch_bounds__(kQuadBwdThreads) void latent_bwd_kernel(const float *__restrict__ skip, int B, int len, int ns, float sqrt_reg,
                                                                     LatentRng rng, int ptr_aligned, int blocks_per_object,
                                                                     const float *__restrict__ g_z, const float *__restrict__ g_kl,
                                                                     float *__restrict__ g_skip)
{
    int b, r, cnt;
    if (!latent_bwd_quad(len, blocks_per_object, b, r, cnt)) return;
    const LatentRows w = latent_rows(b, len, ptr_aligned);
    float loc[4], ls[4], gloc[4], gscale[4];
    quad_load(skip, w.loc0 + r, cnt, w.vec_loc, 0.0f, loc);
    quad_load(skip, w.ls0 + r, cnt, w.vec_ls, 1.0f, ls);
    gloc[0] = gloc[1] = gloc[2] = gloc[3] = 0.0f;
    gscale[0] = gscale[1] = gscale[2] = gscale[3] = 0.0f;
    if (g_z != nullptr)
        for (int s = 0; s < ns; ++s) {
            const size_t row = ((size_t)s * B + b) * (size_t)len;
            const bool vec_z = w.al && (row & 3) == 0;
            float eps[4], gz[4];
            latent_quad_eps(rng, w, row, r, cnt, vec_z, s, eps);
            quad_load(g_z, row + r, cnt, vec_z, 0.0f, gz);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gloc[j] += gz[j];
                gscale[j] += gz[j] * eps[j];
            }
        }
    const float G = g_kl != nullptr ? g_kl[b] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float dscale;
        const float scale = positive_range(ls[j], dscale) + sqrt_reg;
        gloc[j] = gloc[j] + G * loc[j];
        gscale[j] = (gscale[j] + G * (scale - 1.0f / scale)) * dscale;
    }
    quad_store(g_skip, w.loc0 + r, cnt, w.vec_loc, gloc);
    quad_store(g_skip, w.ls0 + r, cnt, w.vec_ls, gscale);
}

static LatentRng latent_rng(int len, long long first_object, unsigned long long seed, unsigned draw, unsigned level, const float *eps_in)
{
    return LatentRng{quad_rng(first_object, len, seed, draw), kLatentTag | (level << 16), eps_in};
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_latent_fwd_f32(const float *skip_dev, int B, int len, int ns, float sqrt_reg, long long first_object, unsigned long long seed,
                          unsigned draw, unsigned level, const float *eps_dev, float *z_out_dev, float *kl_sum_out_dev,
                          float *kl_elem_out_dev, float *eps_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(skip_dev && z_out_dev && kl_sum_out_dev, "latent_fwd: null pointer");
    if (int rc = latent_check("latent_fwd", B, len, ns, kLatentMaxNs, first_object, level)) return rc;
    const LatentRng rng = latent_rng(len, first_object, seed, draw, level, eps_dev);
    const int aligned = head_aligned16({skip_dev, eps_dev, z_out_dev, kl_elem_out_dev, eps_out_dev}) ? 1 : 0;
    hipLaunchKernelGGL(latent_fwd_kernel, dim3(B), dim3(kObjectSumThreads), 0, (hipStream_t)stream, skip_dev, B, len, ns, sqrt_reg, rng, aligned,
                       z_out_dev, kl_sum_out_dev, kl_elem_out_dev, eps_out_dev);
    CTPVAE_LAUNCH_CHECK("latent_fwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_latent_bwd_f32(const float *skip_dev, int B, int len, int ns, float sqrt_reg, long long first_object, unsigned long long seed,
                          unsigned draw, unsigned level, const float *eps_dev, const float *g_z_dev, const float *g_kl_dev,
                          float *g_skip_out_dev, ctpvae_stream_t stream)
{
    CTPVAE_REQUIRE(skip_dev && g_skip_out_dev, "latent_bwd: null pointer");
    if (int rc = latent_check("latent_bwd", B, len, ns, kLatentMaxNs, first_object, level)) return rc;
    const LatentRng rng = latent_rng(len, first_object, seed, draw, level, eps_dev);
    const int aligned = head_aligned16({skip_dev, eps_dev, g_z_dev, g_skip_out_dev}) ? 1 : 0;
    const int bpo = latent_blocks_per_object(len);
    hipLaunchKernelGGL(latent_bwd_kernel, dim3((unsigned)B * (unsigned)bpo), dim3(kQuadBwdThreads), 0, (hipStream_t)stream, skip_dev, B, len,
                       ns, sqrt_reg, rng, aligned, bpo, g_z_dev, g_kl_dev, g_skip_out_dev);
    CTPVAE_LAUNCH_CHECK("latent_bwd_kernel");
    return CTPVAE_OK;
}

int ctpvae_latent_draws_host_f32(int n, int len, int ns, long long first_object, unsigned long long seed, unsigned draw, unsigned level,
                                 float *v_out_host)
{
    CTPVAE_REQUIRE(v_out_host, "latent_draws_host: null pointer");
    if (int rc = latent_check("latent_draws_host", n, len, ns, kLatentMaxNs, first_object, level)) return rc;
    const LatentRng rng = latent_rng(len, first_object, seed, draw, level, nullptr);
    const long long per_sample = (long long)n * len;
    for (int s = 0; s < ns; ++s)
        for (long long i = 0; i < per_sample; ++i) {
            const unsigned long long e = rng.first + (unsigned long long)i;
            const unsigned w = philox_word(latent_block(e >> 2, draw, rng.tag | (unsigned)s, rng.k0, rng.k1), (unsigned)e & 3u);
            const float t = latent_tail(w);
            v_out_host[(long long)s * per_sample + i] = (w >> 31) != 0 ? -t : t;
        }
    return CTPVAE_OK;
}

}  // extern "C"
