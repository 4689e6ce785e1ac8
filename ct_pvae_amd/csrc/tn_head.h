// tn_head.h -- what head.hip (the TruncatedNormal output head) and marginals.hip (per-pixel histograms of that head's samples) share: the
// constants, the layout of the random numbers, and the pixel's function cut into the part that does not depend on the uniform
// (tn_prep) and the part that does (tn_draw).  head.hip's header states the function; both files evaluate it through this code alone,
// so one (alpha, beta, u) gives one x wherever it is computed (-ffp-contract=off: the same fp32 operations, the same bits).
#pragma once
#include "quad_io.h"

namespace ctpvae {

constexpr unsigned kHeadTag = 0x544E48u;     // "TNH": the fourth counter word (hmc.hip: 0x484D43, poisson.hip: 0)
constexpr float kHeadPLo = 1e-7f;
constexpr float kHeadQLo = 1.1920928955078125e-07f;    // 1 - HI, HI = (float)(1 - 1e-7) = 1 - 2^-23
constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kSqrt2Pi = 2.50662827463100050242f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;

__host__ __device__ inline float head_u24(unsigned w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-08f; }

__host__ __device__ inline Philox4 head_block(unsigned long long blk, unsigned draw, unsigned k0, unsigned k1)
{
    return philox4x32_10((unsigned)blk, (unsigned)(blk >> 32), draw, kHeadTag, k0, k1);
}
// the uniforms of the four pixels e .. e+3 (one block when e is a multiple of 4, two otherwise)
__device__ __forceinline__ void head_uniforms4(unsigned long long e, unsigned draw, unsigned k0, unsigned k1, float (&u)[4])
{
    const unsigned s = (unsigned)e & 3u;
    const Philox4 A = head_block(e >> 2, draw, k0, k1);
    Philox4 B = A;
    if (s != 0) B = head_block((e >> 2) + 1, draw, k0, k1);
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) u[j] = head_u24(s + j < 4 ? philox_word(A, s + j) : philox_word(B, s + j - 4));
}

// the pixel before its uniform: loc = pr(alpha), scale = pr(beta), their slopes, a = -loc / scale, Pa = Phi(a), Z = max(1 - Pa, 1e-30)
struct TnPrep {
    float loc, scale, dloc, dscale;
    float a, Pa, Z;
};

__device__ __forceinline__ TnPrep tn_prep(float alpha, float beta)
{
    TnPrep r;
    r.loc = positive_range(alpha, r.dloc);
    r.scale = positive_range(beta, r.dscale);
    r.a = -r.loc / r.scale;
    const float t = r.a * kInvSqrt2;
    r.Pa = 0.5f * erfcf(-t);
    r.Z = fmaxf(0.5f * erfcf(t), 1e-30f);
    return r;
}

// the pixel's sample for the uniform u: the quantile (from the complement on the upper half) and x = max(loc + scale z, 0)
struct TnDraw {
    float omu, z, x;
    bool pass_p, pass_x;         // the clamps of p and of x let the gradient through
};

__device__ __forceinline__ TnDraw tn_draw(const TnPrep &pr, float u)
{
    TnDraw r;
    r.omu = 1.0f - u;
    const float p0 = pr.Pa + u * pr.Z, q0 = pr.Z * r.omu;
    const bool upper = p0 > 0.5f;
    r.pass_p = upper ? q0 >= kHeadQLo : p0 >= kHeadPLo;
    const float zt = normcdfinvf(upper ? fmaxf(q0, kHeadQLo) : fmaxf(p0, kHeadPLo));
    r.z = upper ? -zt : zt;
    const float x0 = pr.loc + pr.scale * r.z;
    r.pass_x = x0 >= 0.0f;
    r.x = fmaxf(x0, 0.0f);
    return r;
}

struct TnPixel {
    float scale, dloc, dscale;   // pr(beta), pr'(alpha), pr'(beta)
    float a, Z, omu, z, D;       // D = ndtri'(p) (backward only)
    float x, zeta, lp;
    bool pass_p, pass_x;
};

template <bool BWD>
__device__ __forceinline__ TnPixel tn_pixel(float alpha, float beta, float u)
{
    const TnPrep pr = tn_prep(alpha, beta);
    const TnDraw d = tn_draw(pr, u);
    TnPixel r;
    r.scale = pr.scale, r.dloc = pr.dloc, r.dscale = pr.dscale;
    r.a = pr.a, r.Z = pr.Z, r.omu = d.omu, r.z = d.z;
    r.x = d.x, r.pass_p = d.pass_p, r.pass_x = d.pass_x;
    r.zeta = (r.x - pr.loc) / r.scale;
    r.lp = ((-0.5f * (r.zeta * r.zeta) - kHalfLog2Pi) - logf(r.scale)) - logf(r.Z);
    if constexpr (BWD) r.D = kSqrt2Pi * expf(0.5f * (r.z * r.z));
    else r.D = 0.0f;
    return r;
}

}  // namespace ctpvae
