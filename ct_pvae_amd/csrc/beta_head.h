// beta_head.h -- what beta_head.hip (the Beta output head) shares with beta_latent.hip (the Beta latents) and beta_marginals.hip (the
// per-pixel marginals of the head's samples): the layout of the random numbers, the log-space gamma sampler cut into the part that does
// not depend on the random numbers (beta_gamma_prep, beta_prep) and the part that does (beta_gamma_draw, beta_draw), the pixel's
// function and the implicit reparameterisation gradient of a gamma's logarithm.  beta_head.hip's header states the function; every
// file evaluates it through this code alone, so one (alpha, beta, e, draw, seed) gives one x wherever it is computed
// (-ffp-contract=off: the same operations, the same bits).
#pragma once
#include "tn_head.h"

namespace ctpvae {

constexpr unsigned kBetaTag = 0x42000000u;   // "B": the head's fourth counter word is kBetaTag | gamma << 8 | attempt
constexpr unsigned kBetaLatentTag = 0x51000000u;   // "Q": the latents' is kBetaLatentTag | level << 16 | s << 5 | gamma << 4 | attempt
constexpr int kBetaAttempts = 16;            // Marsaglia-Tsang attempts per gamma: refusal <= 0.046 each, the cap binds with p < 1e-21
constexpr int kDlgMaxTerms = 2048;           // hard bound on the iterations of beta_dlg's series / continued fraction
constexpr float kBetaThird = 1.0f / 3.0f;

__host__ __device__ inline Philox4 beta_block(unsigned long long e, unsigned draw, unsigned gamma, unsigned attempt, unsigned k0, unsigned k1)
{
    return philox4x32_10((unsigned)e, (unsigned)(e >> 32), draw, kBetaTag | (gamma << 8) | attempt, k0, k1);
}

// the latents' fourth counter word without the attempt: level < 256, s < 2048, gamma 0 or 1 (the attempt takes bits 0 .. 3)
__host__ __device__ inline unsigned beta_latent_word3(unsigned level, unsigned s, unsigned gamma)
{
    return kBetaLatentTag | (level << 16) | (s << 5) | (gamma << 4);
}

// log of a Gamma(c, 1) sample: the accepted attempt's normal and boost uniform, its index, and lg = log(d) + log(v) + boost
struct BetaGamma {
    float zn, ub, lg;
    int k;
};

// a gamma before its random numbers: the concentration c, Marsaglia-Tsang's d = cb - 1/3 (cb = c below 1 boosted by one), s = 1 /
// sqrt(9 d) and log(d)
struct BetaGammaPrep {
    float c, d, s, logd;
};

__device__ __forceinline__ BetaGammaPrep beta_gamma_prep(float c)
{
    BetaGammaPrep p;
    const float cb = c < 1.0f ? c + 1.0f : c;
    p.c = c;
    p.d = cb - kBetaThird;
    p.s = 1.0f / sqrtf(9.0f * p.d);
    p.logd = logf(p.d);
    return p;
}

// the attempt loop, log(v) and the boost.  word3 is the fourth counter word WITHOUT the attempt (the head: kBetaTag | gamma << 8; the
// latents: beta_latent_word3); attempt k is ORed in here.
__device__ __forceinline__ BetaGamma beta_gamma_draw(const BetaGammaPrep &p, unsigned long long e, unsigned draw, unsigned word3, unsigned k0,
                                                     unsigned k1)
{
    const float c = p.c, d = p.d, s = p.s;
    BetaGamma r{0.0f, 0.5f, 0.0f, kBetaAttempts - 1};
    float v = 1.0f;
#pragma unroll 1
    for (int k = 0; k < kBetaAttempts; ++k) {      // bounded by construction: a NaN operand refuses every attempt
        const Philox4 blk = philox4x32_10((unsigned)e, (unsigned)(e >> 32), draw, word3 | (unsigned)k, k0, k1);
        const float zn = normcdfinvf(head_u24(blk.w[0])), ua = head_u24(blk.w[1]);
        const float w = 1.0f + s * zn;
        const float v3 = (w * w) * w;
        r.zn = zn, r.ub = head_u24(blk.w[2]), r.k = k;
        v = w <= 0.0f ? 1.0f : v3;
        if (w > 0.0f && logf(ua) < ((0.5f * (zn * zn) + d) - d * v3) + d * logf(v3)) break;
    }
    const float boost = c < 1.0f ? logf(r.ub) / c : 0.0f;
    r.lg = (p.logd + logf(v)) + boost;
    return r;
}

// prep and draw in one: a gamma whose concentration is used once (the latents)
__device__ __forceinline__ BetaGamma beta_log_gamma(float c, unsigned long long e, unsigned draw, unsigned word3, unsigned k0, unsigned k1)
{
    return beta_gamma_draw(beta_gamma_prep(c), e, draw, word3, k0, k1);
}

// the pixel before its random numbers: a = pr(alpha), b = pr(beta), their slopes, and the two gammas' preps
struct BetaPrep {
    float a, b, da, db;
    BetaGammaPrep g0, g1;
};

__device__ __forceinline__ BetaPrep beta_prep(float alpha, float beta)
{
    BetaPrep r;
    r.a = positive_range(alpha, r.da);
    r.b = positive_range(beta, r.db);
    r.g0 = beta_gamma_prep(r.a);
    r.g1 = beta_gamma_prep(r.b);
    return r;
}

// the pixel's sample for (e, draw, seed): the head's two gammas and x = 1 / (1 + exp(lg_1 - lg_0)), not clamped
struct BetaDraw {
    BetaGamma g0, g1;
    float x;
};

__device__ __forceinline__ BetaDraw beta_draw(const BetaPrep &pr, unsigned long long e, unsigned draw, unsigned k0, unsigned k1)
{
    BetaDraw r;
    r.g0 = beta_gamma_draw(pr.g0, e, draw, kBetaTag | (0u << 8), k0, k1);
    r.g1 = beta_gamma_draw(pr.g1, e, draw, kBetaTag | (1u << 8), k0, k1);
    r.x = 1.0f / (1.0f + expf(r.g1.lg - r.g0.lg));
    return r;
}

struct BetaPixel {
    float a, b, da, db;          // pr(alpha), pr(beta), pr'(alpha), pr'(beta)
    BetaGamma g0, g1;
    float x, y, xc, yc, lp;      // lp: forward only
    bool pass;                   // sr <= x and y >= 1 - hi (x <= hi): the clamp lets the gradient through
};

template <bool BWD>
__device__ __forceinline__ BetaPixel beta_pixel(float alpha, float beta, unsigned long long e, unsigned draw, unsigned k0, unsigned k1,
                                                float sr)
{
    const BetaPrep pr = beta_prep(alpha, beta);
    const BetaDraw dr = beta_draw(pr, e, draw, k0, k1);
    BetaPixel r;
    r.a = pr.a, r.b = pr.b, r.da = pr.da, r.db = pr.db;
    r.g0 = dr.g0, r.g1 = dr.g1;
    r.x = dr.x;
    r.y = 1.0f / (1.0f + expf(r.g0.lg - r.g1.lg));
    // the upper bound is tested on y: x > hi <=> y < 1 - hi, and next to 1 y keeps the relative accuracy that x has lost
    const float hi = 1.0f - sr, lo_y = 1.0f - hi;
    r.pass = r.x >= sr && r.y >= lo_y;
    r.xc = r.x < sr ? sr : (r.y < lo_y ? hi : r.x);        // (a NaN x stays NaN)
    r.yc = r.x < sr ? hi : (r.y < lo_y ? lo_y : r.y);
    if constexpr (!BWD) r.lp = ((r.a - 1.0f) * logf(r.xc) + (r.b - 1.0f) * logf(r.yc)) - ((lgammaf(r.a) + lgammaf(r.b)) - lgammaf(r.a + r.b));
    else r.lp = 0.0f;
    return r;
}

// ---- the backward's float64 part ------------------------------------------------------------------------------------------------
// digamma(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10 (at most 10 steps), then the asymptotic series
// log x - 1/2x - 1/12x^2 + 1/120x^4 - 1/252x^6 + 1/240x^8 - 1/132x^10 + 691/32760x^12 - 1/12x^14 (the next term is < 5e-16 at x = 10).
__device__ __forceinline__ double beta_digamma(double x)
{
    double r = 0.0;
#pragma unroll 1
    for (int i = 0; i < 10 && x < 10.0; ++i) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double inv = 1.0 / x, i2 = inv * inv;
    const double series = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 * (1.0 / 12)))))));
    return r + ((log(x) - 0.5 * inv) - series);
}

// lgamma(x) and digamma(x) together, x > 0, for the latents' KL term: ten straight-line steps of the recurrences lgamma(x) =
// lgamma(x + 1) - log x and psi(x) = psi(x + 1) - 1 / x, each taken while x < 10 -- the factors multiplied into p and ONE logarithm
// taken, the reciprocals kept as the fraction q / p (q <- q x + p: all terms positive, no cancellation) and ONE division made -- then,
// with one logarithm and one reciprocal of the shifted x shared by both, Stirling's series (x - 1/2) log x - x + log(2 pi) / 2 + 1/12x
// - 1/360x^3 + 1/1260x^5 - 1/1680x^7 + 1/1188x^9 - 691/360360x^11 + 1/156x^13 - 3617/122400x^15 (the next term is < 2e-17 at x = 10)
// and beta_digamma's series.  No loop and no branch: the chains of several arguments overlap each other's latencies.  (The
// library's float64 lgamma costs a kernel more than 128 registers.)
__device__ __forceinline__ void beta_lgamma_digamma(double x, double &lg, double &psi)
{
    double p = 1.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const bool low = x < 10.0;
        q = low ? q * x + p : q;
        p = low ? p * x : p;
        x = low ? x + 1.0 : x;
    }
    const double inv = 1.0 / x, i2 = inv * inv, lx = log(x);
    const double stirling = inv * (1.0 / 12 - i2 * (1.0 / 360 - i2 * (1.0 / 1260 - i2 * (1.0 / 1680 - i2 * (1.0 / 1188 - i2 * (691.0 / 360360 - i2 * (1.0 / 156 - i2 * (3617.0 / 122400))))))));
    const double series = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 * (1.0 / 12)))))));
    lg = ((((x - 0.5) * lx - x) + 0.91893853320467274178) + stirling) - log(p);
    psi = ((lx - 0.5 * inv) - series) - q / p;
}

// trigamma(x), x > 0: the recurrence psi'(x) = psi'(x + 1) + 1 / x^2 up to x >= 10 (at most 10 steps), then the asymptotic series
// 1/x + 1/2x^2 + 1/6x^3 - 1/30x^5 + 1/42x^7 - 1/30x^9 + 5/66x^11 - 691/2730x^13 + 7/6x^15 (the next term is < 4e-16 at x = 10).
__device__ __forceinline__ double beta_trigamma(double x)
{
    double r = 0.0;
#pragma unroll 1
    for (int i = 0; i < 10 && x < 10.0; ++i) {
        r += 1.0 / (x * x);
        x += 1.0;
    }
    const double inv = 1.0 / x, i2 = inv * inv;
    const double series = i2 * (1.0 / 6 - i2 * (1.0 / 30 - i2 * (1.0 / 42 - i2 * (1.0 / 30 - i2 * (5.0 / 66 - i2 * (691.0 / 2730 - i2 * (7.0 / 6)))))));
    return r + (inv + (0.5 * i2 + inv * series));
}

// d lg / d c of lg = log g, g ~ Gamma(c, 1), at a fixed uniform of the implicit form: -(dP(c, g) / dc) / (g p(g; c)), with the
// prefactor g^c e^-g / Gamma(c) cancelled analytically (g = exp(lg) may underflow to 0: the series then IS its limit
// -(lg - digamma(c + 1)) / c).  At most kDlgMaxTerms iterations, enough for every c <= 4e4 (the series needs about 9.5 sqrt(c) terms for
// 1e-17); a sum that has not converged at the bound -- a larger c, a NaN operand -- returns NaN instead of a truncated value (the
// trainer's NaN filter sees it).  No asymptotic form is switched to.
//   g <= c + 1:  S = sum_n t_n, t_n = g^n / ((c + 1) .. (c + n)), dS/dc = -sum_n t_n H_n, H_n = sum_(k <= n) 1 / (c + k)
//                dlg = -((lg - digamma(c + 1)) S + dS/dc) / c
//   g >  c + 1:  CF = A / B of Gamma(c, g) = e^-g g^c CF (b_i = g + 2i - 1 - c, a_1 = 1, a_i = -(i - 1)(i - 1 - c)), by the forward
//                recurrence of A, B and of their c-derivatives (rescaled together past 1e100);  dlg = (lg - digamma(c)) CF + dCF/dc
__device__ __forceinline__ double beta_dlg(double c, double lg)
{
    const double g = exp(lg);
    if (!(g > c + 1.0)) {
        double t = 1.0, S = 1.0, H = 0.0, dS = 0.0;
        bool conv = false;
#pragma unroll 1
        for (int n = 1; n <= kDlgMaxTerms && !conv; ++n) {
            const double r = 1.0 / (c + n);
            t *= g * r;
            H += r;
            S += t;
            dS -= t * H;
            conv = t * (c + n) < 1e-17 * S;
        }
        return conv ? -((lg - beta_digamma(c + 1.0)) * S + dS) / c : __builtin_nan("");
    }
    double A1 = 1.0, A0 = 0.0, B1 = 0.0, B0 = 1.0;      // A_(i-2), A_(i-1), B_(i-2), B_(i-1)
    double dA1 = 0.0, dA0 = 0.0, dB1 = 0.0, dB0 = 0.0;
    double cf = 0.0, dcf = 0.0;
    bool conv = false;
#pragma unroll 1
    for (int i = 1; i <= kDlgMaxTerms && !conv; ++i) {
        const double bi = g + (2 * i - 1) - c;
        const double ai = i == 1 ? 1.0 : -(double)(i - 1) * ((i - 1) - c);
        const double dai = i == 1 ? 0.0 : (double)(i - 1);
        double A = bi * A0 + ai * A1, B = bi * B0 + ai * B1;
        double dA = (bi * dA0 - A0) + (ai * dA1 + dai * A1), dB = (bi * dB0 - B0) + (ai * dB1 + dai * B1);
        A1 = A0, B1 = B0, dA1 = dA0, dB1 = dB0;
        A0 = A, B0 = B, dA0 = dA, dB0 = dB;
        if (fabs(B) > 1e100) {
            A1 *= 1e-100, A0 *= 1e-100, B1 *= 1e-100, B0 *= 1e-100;
            dA1 *= 1e-100, dA0 *= 1e-100, dB1 *= 1e-100, dB0 *= 1e-100;
        }
        const double ib = 1.0 / B0;
        const double ncf = A0 * ib, ndcf = (dA0 - ncf * dB0) * ib;
        conv = fabs(ncf - cf) <= 1e-16 * fabs(ncf) && fabs(ndcf - dcf) <= 1e-14 * fabs(ndcf) + 1e-300;
        cf = ncf, dcf = ndcf;
    }
    return conv ? (lg - beta_digamma(c)) * cf + dcf : __builtin_nan("");
}

// (g_alpha, g_beta) of one pixel for the cotangents gx (of x) and G (of the object's LP): float64 arithmetic on the forward's float32
// intermediates (why float64: beta_head.hip's header)
__device__ __forceinline__ void beta_pixel_grad(const BetaPixel &p, float gx, float G, float &g_alpha, float &g_beta)
{
    const double a = p.a, b = p.b, x = p.x, y = p.y, xc = p.xc, yc = p.yc, Gd = G;
    const double gx0 = p.pass ? (double)gx + Gd * ((a - 1.0) / xc - (b - 1.0) / yc) : (double)gx;
    const double xy = x * y;
    double pa = 0.0, pb = 0.0;
    if (!(gx0 == 0.0 || xy == 0.0)) {           // the path through x: exactly nothing where x saturated or no cotangent arrives
        pa = gx0 * xy * beta_dlg(a, (double)p.g0.lg);
        pb = -(gx0 * xy * beta_dlg(b, (double)p.g1.lg));
    }
    double da = 0.0, db = 0.0;
    if (G != 0.0f) {
        const double pab = beta_digamma(a + b);
        da = Gd * ((log(xc) - beta_digamma(a)) + pab);
        db = Gd * ((log(yc) - beta_digamma(b)) + pab);
    }
    g_alpha = (float)((pa + da) * (double)p.da);
    g_beta = (float)((pb + db) * (double)p.db);
}

inline int beta_head_check(const char *what, const void *alpha, const void *beta, int n, int pix, long long first_object, float sqrt_reg)
{
    if (int rc = head_check(what, alpha, beta, n, pix, first_object)) return rc;
    CTPVAE_REQUIRE(sqrt_reg > 0.0f && sqrt_reg < 0.5f, "%s: sqrt_reg must lie in (0, 0.5) (got %g)", what, (double)sqrt_reg);
    return CTPVAE_OK;
}

}  // namespace ctpvae
