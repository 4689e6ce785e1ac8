// hmc.h -- what hmc.hip (the HMC sampler's two kernels) and hmc_marginals.hip (the same transitions with the chains' histograms and
// moments accumulated inside the launch) share: the launch arguments, the scans over the wave, the bijector, the target and its
// gradient, the launch's tables in LDS, one whole transition, the LDS size and the checks of the model's arguments.  hmc.hip's header
// states all of it -- the density, the transition, the orders of the sums and the layout of the random numbers; every expression here
// is evaluated in one place, so a chain's bits are the same in either file.
#pragma once
#include <cfloat>

#include "common.h"
#include "loglik_math.h"
#include "philox.h"

namespace ctpvae {

constexpr int kHmcZeroTap = 64;              // O cell that holds 0: the forward tap of a row that misses the object
constexpr unsigned kHmcTag = 0x484D43u;      // "HMC": the fourth counter word
constexpr float kHmcLogFltMin = -87.336544750553102f;   // log(FLT_MIN)
constexpr float kHmcLogTarget = -0.28768207245178096f;  // log(0.75), the acceptance target of the step-size rule
constexpr float kTwoPi = 6.28318530717958647692f;

struct HmcParams {
    float *state;                 // [C][2K + 1]
    unsigned first_chain;
    int cpo, N, K, A, npass;      // npass = ceil(A * N / 64)
    const float *T8, *Tinv8, *mask, *meas;
    float pnm;
    int M;
    const float *logw, *alpha, *lbeta;
    const float *start;           // INIT: [C][K] simplex points or nullptr
    float step_size;              // INIT
    int L, n_steps;
    unsigned keep_from, n_adapt, k0, k1;
    float *samples, *lar, *acc, *target;
    int C;
};

template <int CTRL, int ROW = 0xf>
__device__ __forceinline__ float hmc_dpp0(float v)   // the DPP-moved value, +0.0f where the source lane does not exist / the row is masked
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW, 0xf, false));
}
// inclusive prefix sum over the lanes of the wave
__device__ __forceinline__ float wave_scan_incl(float v)
{
    v = v + hmc_dpp0<0x111>(v);        // row_shr:1
    v = v + hmc_dpp0<0x112>(v);        // row_shr:2
    v = v + hmc_dpp0<0x114>(v);        // row_shr:4
    v = v + hmc_dpp0<0x118>(v);        // row_shr:8
    v = v + hmc_dpp0<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v = v + hmc_dpp0<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}
// sum over the lanes above this one: the same scan on the mirrored wave
__device__ __forceinline__ float wave_suffix_excl(float v, int lane)
{
    const float inc = wave_scan_incl(__shfl(v, 63 - lane));
    const float up = __shfl(inc, 62 - lane);   // lane 63 reads lane 63 (the index wraps): replaced by 0 below
    return lane < 63 ? up : 0.0f;
}

struct HmcLds {
    float *O, *g, *meas, *mask;
    unsigned char *ftap, *btap;
};
struct HmcLane {
    int lane, N, A, npass, M, zslot;
    bool act, pix;          // lane holds a coordinate of x / a pixel
    float c, kmj, pnm;      // log(K-1-lane), K - lane
    float am1[4], logw[4], lbeta[4];
};
struct HmcSimplex {
    float z, omz, lz, l1mz, logr, logO, O;
};

__device__ __forceinline__ HmcSimplex hmc_simplex(float x, const HmcLane &q)
{
    HmcSimplex s;
    const float t = q.act ? x - q.c : 0.0f;
    const float e = expf(-fabsf(t)), l = log1pf(e);
    const float inv = 1.0f / (1.0f + e);
    const bool pos = t >= 0.0f;
    s.z = q.act ? (pos ? inv : e * inv) : 0.0f;
    s.omz = pos ? e * inv : inv;
    s.lz = q.act ? -(fmaxf(-t, 0.0f) + l) : 0.0f;
    s.l1mz = q.act ? -(fmaxf(t, 0.0f) + l) : 0.0f;
    const float inc = wave_scan_incl(s.l1mz);
    const float prev = __shfl_up(inc, 1);
    s.logr = q.lane == 0 ? 0.0f : prev;
    s.logO = s.lz + s.logr;
    s.O = q.pix ? expf(s.logO) : 0.0f;
    return s;
}

// T (when WANT_T is set) and dT/dx at x; sp: the bijector's values there
__device__ __forceinline__ void hmc_eval(float x, bool want_T, const HmcLane &q, const HmcLds &m, HmcSimplex &sp, float &T, float &grad)
{
    sp = hmc_simplex(x, q);
    const bool bind = sp.O < FLT_MIN;
    const float Oc = bind ? FLT_MIN : sp.O, logOc = bind ? kHmcLogFltMin : sp.logO;
    m.O[q.lane] = q.pix ? Oc : 0.0f;
    __syncthreads();
    float lp = 0.0f;
    for (int pass = 0; pass < q.npass; ++pass) {
        const unsigned char *tap = m.ftap + (size_t)pass * q.N * 64 + q.lane;
        float proj = 0.0f;
        for (int i = 0; i < q.N; ++i) proj += m.O[tap[i * 64]];
        const int e = pass * 64 + q.lane;
        const float mk = m.mask[e], xm = m.meas[e];
        m.g[e] = poisson_dlogp(proj, mk, xm, q.pnm);
        if (want_T) lp += poisson_logp(proj, mk, xm, q.pnm);
    }
    __syncthreads();
    float G = 0.0f;
    for (int a = 0; a < q.A; ++a) {
        const int b = m.btap[a * 64 + q.lane];
        G += m.g[b == 255 ? q.zslot : a * q.N + b];
    }
    // the mixture: a_m = log of component m's weighted density, softmax over m
    float am[4], mx = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        am[k] = -__builtin_inff();
        if (k < q.M) {
            const float s = wave_sum(q.pix ? q.am1[k] * logOc : 0.0f);
            am[k] = (q.logw[k] + s) - q.lbeta[k];
            mx = fmaxf(mx, am[k]);
        }
    }
    float den = 0.0f, pe[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pe[k] = k < q.M ? expf(am[k] - mx) : 0.0f;   // (a NaN a_m is dropped by fmaxf and comes back here)
        den += pe[k];
    }
    float wprior = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < q.M) wprior += (pe[k] / den) * q.am1[k];
    const float w = (q.pix && !bind) ? Oc * G + wprior : 0.0f;
    const float above = wave_suffix_excl(w, q.lane);
    grad = q.act ? (w * sp.omz - sp.z * above) + (1.0f - q.kmj * sp.z) : 0.0f;
    if (want_T) {
        const float prior = mx + logf(den);
        const float lik = wave_sum(lp);
        const float fldj = wave_sum(q.act ? (sp.lz + sp.l1mz) + sp.logr : 0.0f);
        T = (prior + lik) + fldj;
    }
}

__device__ __forceinline__ float hmc_u24(unsigned w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-08f; }

// The launch's set-up for chain c = blockIdx.x: the lane's constants q, the LDS layout m over `lds` (hmc_lds_bytes() bytes) and the
// tables in it.  Ends with the barrier that orders the tables before their first read.
__device__ __forceinline__ void hmc_setup(const HmcParams &p, float *lds, HmcLds &m, HmcLane &q)
{
    const int lane = threadIdx.x, c = blockIdx.x;
    const int N = p.N, K = p.K, A = p.A, AN = A * N, cells = p.npass * 64;
    m.O = lds;                       // [64] pixels + the zero cell (+ padding to 68)
    m.g = m.O + 68;                  // [cells] + the zero cell (+ padding to cells + 4)
    m.meas = m.g + cells + 4;        // [cells]
    m.mask = m.meas + cells;         // [cells]
    m.ftap = reinterpret_cast<unsigned char *>(m.mask + cells);   // [npass][N][64]
    m.btap = m.ftap + (size_t)cells * N;                          // [A][64]
    q.lane = lane, q.N = N, q.A = A, q.npass = p.npass, q.M = p.M, q.zslot = cells;
    q.act = lane < K - 1, q.pix = lane < K;
    q.c = q.act ? logf((float)(K - 1 - lane)) : 0.0f;
    q.kmj = (float)(K - lane);
    q.pnm = p.pnm;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool on = k < p.M;
        q.am1[k] = (on && q.pix) ? p.alpha[k * K + lane] - 1.0f : 0.0f;
        q.logw[k] = on ? p.logw[k] : 0.0f;
        q.lbeta[k] = on ? p.lbeta[k] : 0.0f;
    }

    // ---- the launch's tables
    const int obj = c / p.cpo;
    if (lane == 0) m.O[kHmcZeroTap] = 0.0f, m.g[cells] = 0.0f;
    for (int pass = 0; pass < p.npass; ++pass) {
        const int e = pass * 64 + lane;
        const bool live = e < AN;
        const int a = live ? e / N : 0, j = e - a * N;
        m.meas[e] = live ? p.meas[(size_t)obj * AN + e] : 0.0f;
        m.mask[e] = live ? p.mask[(size_t)obj * A + a] : 0.0f;
        const float *t = p.T8 + 8 * a;
        const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4], t5 = t[5];
        const float xj = t0 * (float)j, yj = t3 * (float)j;
        for (int i = 0; i < N; ++i) {
            const float fi = (float)i;
            const float x = (xj + t1 * fi) + t2;
            const float y = (yj + t4 * fi) + t5;
            const int ix = (int)__builtin_roundf(x), iy = (int)__builtin_roundf(y);
            const bool hit = live && (unsigned)iy < (unsigned)N && (unsigned)ix < (unsigned)N;
            m.ftap[((size_t)pass * N + i) * 64 + lane] = (unsigned char)(hit ? iy * N + ix : kHmcZeroTap);
        }
    }
    {
        const int r = lane / N, col = lane - r * N;
        const float fx = (float)col, fy = (float)r;
        for (int a = 0; a < A; ++a) {
            const float *t = p.Tinv8 + 8 * a;
            const float x = (t[0] * fx + t[1] * fy) + t[2];
            const float y = (t[3] * fx + t[4] * fy) + t[5];
            const int ix = (int)__builtin_roundf(x), iy = (int)__builtin_roundf(y);
            const bool hit = q.pix && (unsigned)iy < (unsigned)N && (unsigned)ix < (unsigned)N;
            m.btap[a * 64 + lane] = (unsigned char)(hit ? ix : 255);
        }
    }
    __syncthreads();
}

// A chain's carried state in registers: x and g = dT/dx per lane, T and the step size, and O, the simplex point of x.
struct HmcChain {
    float x, g, T, eps, O;
};

// One whole transition of step t (hmc.hip's header): the momentum draw, L leapfrogs, the accept test and the step-size rule.
// Leaves the log accept ratio in lar and returns the decision.
__device__ __forceinline__ bool hmc_transition(const HmcParams &p, const HmcLane &q, const HmcLds &m, unsigned t, unsigned chain,
                                               HmcChain &s, float &lar)
{
    const int lane = q.lane;
    HmcSimplex sp;
    float mom;
    {
        const Philox4 b = philox4x32_10(t, chain, (unsigned)(lane >> 2), kHmcTag, p.k0, p.k1);
        const bool hi = (lane & 2) != 0;
        const float u1 = hmc_u24(hi ? b.w[2] : b.w[0]), u2 = hmc_u24(hi ? b.w[3] : b.w[1]);
        const float r = sqrtf(-2.0f * logf(u1)), ang = kTwoPi * u2;
        mom = q.act ? ((lane & 1) ? r * sinf(ang) : r * cosf(ang)) : 0.0f;
    }
    const float kin0 = 0.5f * wave_sum(mom * mom);
    const float half = 0.5f * s.eps;
    mom = mom + half * s.g;
    float xn = s.x, Tn = 0.0f, gn = 0.0f;
    for (int l = 0; l < p.L; ++l) {
        const bool last = l == p.L - 1;
        xn = xn + s.eps * mom;
        hmc_eval(xn, last, q, m, sp, Tn, gn);
        mom = mom + (last ? half : s.eps) * gn;
    }
    const float kin1 = 0.5f * wave_sum(mom * mom);
    lar = (Tn - kin1) - (s.T - kin0);
    const Philox4 b = philox4x32_10(t, chain, 0xFFFFFFFFu, kHmcTag, p.k0, p.k1);
    const bool accept = logf(hmc_u24(b.w[0])) < lar;   // a NaN ratio rejects
    if (accept) s.x = xn, s.T = Tn, s.g = gn, s.O = sp.O;
    if (t < p.n_adapt) {
        const bool up = lar == lar && fminf(lar, 0.0f) > kHmcLogTarget;
        s.eps = up ? s.eps * 1.01f : s.eps / 1.01f;
    }
    return accept;
}

// the chain's state of this launch, and the index of its first step
__device__ __forceinline__ HmcChain hmc_load_chain(const float *st, int K, const HmcLane &q, unsigned &t0)
{
    HmcChain s;
    s.x = q.act ? st[q.lane] : 0.0f, s.g = q.act ? st[K - 1 + q.lane] : 0.0f;
    s.T = st[2 * K - 2], s.eps = st[2 * K - 1];
    t0 = __float_as_uint(st[2 * K]);
    s.O = hmc_simplex(s.x, q).O;
    return s;
}
__device__ __forceinline__ void hmc_store_chain(float *st, int K, const HmcLane &q, const HmcChain &s, unsigned t_next)
{
    if (q.act) st[q.lane] = s.x, st[K - 1 + q.lane] = s.g;
    if (q.lane == 0) st[2 * K - 2] = s.T, st[2 * K - 1] = s.eps, st[2 * K] = __uint_as_float(t_next);
}

// the per-step outputs of a kept step: row r of samples [rows][C][K] and of the three traces [rows][C]
__device__ __forceinline__ void hmc_store_step(const HmcParams &p, const HmcLane &q, unsigned r, int c, const HmcChain &s, float lar,
                                               bool accept)
{
    const size_t row = (size_t)r * p.C + c;
    if (q.pix) p.samples[row * p.K + q.lane] = s.O;
    if (q.lane == 0) p.lar[row] = lar, p.acc[row] = accept ? 1.0f : 0.0f, p.target[row] = s.T;
}

inline size_t hmc_lds_bytes(int N, int A)
{
    const size_t cells = (size_t)ceil_div(A * N, 64) * 64;
    return (68 + (cells + 4) + 2 * cells) * sizeof(float) + cells * N + (size_t)A * 64;
}

inline int hmc_check_model(const char *what, const void *state, int C, int cpo, int N, const void *T8, const void *Tinv8, int A,
                           const void *mask, const void *meas, float pnm, int M, const void *logw, const void *alpha, const void *lbeta)
{
    CTPVAE_REQUIRE(state && T8 && Tinv8 && mask && meas && logw && alpha && lbeta, "%s: null pointer", what);
    CTPVAE_REQUIRE(C > 0 && cpo > 0 && C % cpo == 0, "%s: need C > 0 chains, a multiple of chains_per_object > 0 (got C=%d, %d per object)",
                   what, C, cpo);
    CTPVAE_REQUIRE(N >= 2 && N <= 8, "%s: objects of 2 x 2 .. 8 x 8 pixels only, one pixel per lane (got N=%d)", what, N);
    CTPVAE_REQUIRE(A >= 1 && A <= CTPVAE_HMC_MAX_ANGLES, "%s: 1 .. %d angles (got A=%d)", what, CTPVAE_HMC_MAX_ANGLES, A);
    CTPVAE_REQUIRE(pnm > 0.0f, "%s: the noise multiplier must be positive (got %g)", what, (double)pnm);
    CTPVAE_REQUIRE(M >= 1 && M <= CTPVAE_HMC_MAX_COMPONENTS, "%s: 1 .. %d mixture components (got M=%d)", what, CTPVAE_HMC_MAX_COMPONENTS, M);
    return CTPVAE_OK;
}

// the launch arguments every run entry point fills alike
inline HmcParams hmc_run_params(float *state, int C, unsigned first_chain, int cpo, int N, const float *T8, const float *Tinv8, int A,
                                const float *mask, const float *meas, float pnm, int M, const float *logw, const float *alpha,
                                const float *lbeta, int L, int n_steps, unsigned n_keep_from, unsigned n_adapt, unsigned long long seed,
                                float *samples, float *lar, float *acc, float *target)
{
    HmcParams p{};
    p.state = state, p.first_chain = first_chain, p.cpo = cpo, p.N = N, p.K = N * N, p.A = A;
    p.npass = ceil_div(A * N, 64);
    p.T8 = T8, p.Tinv8 = Tinv8, p.mask = mask, p.meas = meas, p.pnm = pnm;
    p.M = M, p.logw = logw, p.alpha = alpha, p.lbeta = lbeta;
    p.L = L, p.n_steps = n_steps, p.keep_from = n_keep_from, p.n_adapt = n_adapt;
    p.k0 = (unsigned)seed, p.k1 = (unsigned)(seed >> 32);
    p.samples = samples, p.lar = lar, p.acc = acc, p.target = target, p.C = C;
    return p;
}

}  // namespace ctpvae
