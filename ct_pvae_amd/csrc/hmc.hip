// hmc.hip -- Hamiltonian Monte Carlo on the posterior of a small object, one 64-lane wave per chain (bin/toy_mcmc_v2.py,
// ctvae/toy_mcmc_v2_functions.py:66-95): a persistent kernel runs n_steps whole transitions -- momentum draw, L leapfrogs (each one
// bijector + prior + rotate-and-sum + Poisson likelihood + the tape's backward), accept test, step-size adaptation -- without
// returning to the host.  One workgroup IS one wave, so nothing here waits on another wave (the __syncthreads() below only order
// this wave's own LDS traffic); every loop's trip count is a launch argument.
//
// Scope: square objects of K = N * N <= 64 pixels (pixel k = row * N + column lives in lane k), the rotate model with NEAREST
// sampling on the unpadded canvas (P = N), A <= 256 angles, fp32.
//
// The target [3P-recalled: TFP 0.14's TransformedTransitionKernel(HamiltonianMonteCarlo, IteratedSigmoidCentered) -- restated from
// memory of its source, not copied; tests/np_twin_hmc.py restates it again in numpy and pins the derivative against autograd]:
//   state x in R^(K-1), lane k < K-1;   t_k = x_k - log(K-1-k),  z_k = sigmoid(t_k)
//   log z_k = -softplus(-t_k),  log(1 - z_k) = -softplus(t_k)           (softplus(t) = max(t, 0) + log1p(exp(-|t|)))
//   log r_k = sum_{j<k} log(1 - z_j)                                    (exclusive prefix scan over lanes)
//   log O_k = log z_k + log r_k (k < K-1),  log O_(K-1) = log r_(K-1);  O_k = exp(log O_k): the simplex point, = z_k prod_{j<k}(1 - z_j)
//   fldj    = sum_{k<K-1} [log z_k + log(1 - z_k) + log r_k]
//   O'      = max(O, FLT_MIN) (joint_log_prob:85; its derivative is 0 where it binds, and a NaN stays a NaN)
//   prior   = log sum_m exp((logw_m + sum_k (alpha_mk - 1) log O'_k) - lbeta_m),  M <= 4 Dirichlet components
//   lik     = sum_{a,j} poisson_logp(proj[a][j], mask[a], meas[a][j], pnm),  proj = the nearest rotate-and-sum of O' as [N][N]
//   T(x)    = (prior + lik) + fldj
// and its gradient, the way TensorFlow's tape gives it:
//   g[a][j] = poisson_dlogp(...);  G_k = sum_a g[a][round(x'_in)] with Tinv8 (the tf_compat rule of rotate_bwd_tfcompat_kernel)
//   w_k     = O'_k G_k + sum_m softmax_m (alpha_mk - 1)   (= O_k dT/dO_k; 0 where the clamp binds)
//   dT/dx_j = (w_j (1 - z_j) - z_j sum_{k>j} w_k) + (1 - (K - j) z_j)          (J^T of the bijector: a reverse scan; + grad fldj)
//
// The transition at step t, from x with its carried T and g = dT/dx and the chain's step size eps [3P-recalled:
// tfp.mcmc.HamiltonianMonteCarlo's leapfrog integrator and Metropolis test, restated from memory]:
//   p ~ N(0, I) over the K-1 coordinates;  kin0 = 0.5 |p|^2
//   p += (0.5 eps) g
//   l = 0 .. L-1:  x' += eps p  (x' starts at x);  p += eps dT/dx(x'), with 0.5 eps in place of eps at l = L-1
//   lar = (T(x') - 0.5 |p|^2) - (T(x) - kin0)                                   (the log accept ratio)
//   accept iff log u < lar, u uniform on (0, 1): x, T, g <- x', T(x'), dT/dx(x').  A NaN lar compares false and rejects.
//   T and dT/dx of the current state are carried from the step that accepted it, never recomputed; T(x') is evaluated at l = L-1 only.
//
// Step-size adaptation, per chain, after the accept test of every step t < num_adaptation_steps [3P-recalled:
// tfp.mcmc.SimpleStepSizeAdaptation with target_accept_prob 0.75 and adaptation_rate 0.01, restated from memory]:
//   eps <- eps * 1.01f   if min(lar, 0) > logf(0.75f)
//   eps <- eps / 1.01f   otherwise, a NaN lar included
// one fp32 operation on fp32 values either way, so the host can replay the rule on the returned log accept ratios bit for bit.
//
// Projector taps.  The forward's tap of ray (a, j) at canvas row i and the backward's bin of pixel k at angle a depend on the
// tables alone, so each launch evaluates them ONCE, with the unfused fp32 expressions of rotate_fwd_kernel / rotate_bwd_tfcompat_kernel
// (rotate.hip; this file is compiled with -ffp-contract=off like them), into byte tables in LDS; a miss points at a cell that holds 0.
//
// Orders of the sums (fixed, so that a chain's bits do not depend on how it was launched):
//   ray-sum    rows i = 0 .. N-1 ascending from +0.0f (rotate_fwd_kernel's order: the bits of project_tf_fast)
//   lik        sinogram entry e = a * N + j belongs to lane e % 64, pass e / 64; a lane adds its passes ascending from +0.0f
//              (entries past A * N add -0.0f), the 64 lane sums are added by wave_sum's xor butterfly 32, 16, 8, 4, 2, 1
//   G_k        angles ascending from +0.0f (rotate_bwd_tfcompat_kernel's order)
//   scans      wave_scan_incl below: Kogge-Stone inside a row of 16 (row_shr 1, 2, 4, 8), then row_bcast 15 and 31
//   other sums over lanes (prior's, fldj, |p|^2): wave_sum, idle lanes add +0.0f
//
// Random numbers: Philox4x32-10 (philox.h), key = (seed lo, seed hi), counter = (t, chain_id, block, 0x484D43) -- a chain's draws
// depend on (seed, chain id, step index t) alone.  block b < 16: the momenta of coordinates 4b .. 4b+3 by Box-Muller on the word
// pairs (0, 1) and (2, 3), u = ((w >> 8) + 0.5f) * 2^-24 in fp32, r = sqrt(-2 log u1): r cos(2 pi u2), r sin(2 pi u2).  block
// 0xFFFFFFFF: word 0 gives the accept test's u.
//
// State of a chain, 2K + 1 floats: x [K-1], dT/dx [K-1], T, step size, and the BITS of the unsigned 32-bit index of the next step.
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

template <bool INIT>
__global__ __launch_bounds__(64) void hmc_kernel(HmcParams p)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x, c = blockIdx.x;
    const int N = p.N, K = p.K, A = p.A, AN = A * N, cells = p.npass * 64;
    HmcLds m;
    m.O = lds;                       // [64] pixels + the zero cell (+ padding to 68)
    m.g = m.O + 68;                  // [cells] + the zero cell (+ padding to cells + 4)
    m.meas = m.g + cells + 4;        // [cells]
    m.mask = m.meas + cells;         // [cells]
    m.ftap = reinterpret_cast<unsigned char *>(m.mask + cells);   // [npass][N][64]
    m.btap = m.ftap + (size_t)cells * N;                          // [A][64]
    HmcLane q;
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

    float *st = p.state + (size_t)c * (2 * K + 1);
    HmcSimplex sp;
    if constexpr (INIT) {
        float x = 0.0f;
        if (p.start != nullptr) {
            // the inverse bijector: z_k = O_k / sum_{j>=k} O_j, x_k = (log O_k - log sum_{j>k} O_j) + log(K-1-k)
            const float v = q.pix ? p.start[(size_t)c * K + lane] : 0.0f;
            const float above = wave_suffix_excl(v, lane);
            x = q.act ? (logf(v) - logf(above)) + q.c : 0.0f;
        }
        float T = 0.0f, g = 0.0f;
        hmc_eval(x, true, q, m, sp, T, g);
        if (q.act) st[lane] = x, st[K - 1 + lane] = g;
        if (lane == 0) st[2 * K - 2] = T, st[2 * K - 1] = p.step_size, st[2 * K] = __uint_as_float(0u);
        return;
    }

    float x = q.act ? st[lane] : 0.0f, g = q.act ? st[K - 1 + lane] : 0.0f;
    float T = st[2 * K - 2], eps = st[2 * K - 1];
    const unsigned t0 = __float_as_uint(st[2 * K]);
    float O = hmc_simplex(x, q).O;
    const unsigned chain = p.first_chain + (unsigned)c;
    // rows of the outputs: the first kept step of this launch is row 0
    const unsigned skip = p.keep_from > t0 ? p.keep_from - t0 : 0u;

    for (int s = 0; s < p.n_steps; ++s) {
        const unsigned t = t0 + (unsigned)s;
        float mom;
        {
            const Philox4 b = philox4x32_10(t, chain, (unsigned)(lane >> 2), kHmcTag, p.k0, p.k1);
            const bool hi = (lane & 2) != 0;
            const float u1 = hmc_u24(hi ? b.w[2] : b.w[0]), u2 = hmc_u24(hi ? b.w[3] : b.w[1]);
            const float r = sqrtf(-2.0f * logf(u1)), ang = kTwoPi * u2;
            mom = q.act ? ((lane & 1) ? r * sinf(ang) : r * cosf(ang)) : 0.0f;
        }
        const float kin0 = 0.5f * wave_sum(mom * mom);
        const float half = 0.5f * eps;
        mom = mom + half * g;
        float xn = x, Tn = 0.0f, gn = 0.0f;
        for (int l = 0; l < p.L; ++l) {
            const bool last = l == p.L - 1;
            xn = xn + eps * mom;
            hmc_eval(xn, last, q, m, sp, Tn, gn);
            mom = mom + (last ? half : eps) * gn;
        }
        const float kin1 = 0.5f * wave_sum(mom * mom);
        const float lar = (Tn - kin1) - (T - kin0);
        const Philox4 b = philox4x32_10(t, chain, 0xFFFFFFFFu, kHmcTag, p.k0, p.k1);
        const bool accept = logf(hmc_u24(b.w[0])) < lar;   // a NaN ratio rejects
        if (accept) x = xn, T = Tn, g = gn, O = sp.O;
        if (t < p.n_adapt) {
            const bool up = lar == lar && fminf(lar, 0.0f) > kHmcLogTarget;
            eps = up ? eps * 1.01f : eps / 1.01f;
        }
        if ((unsigned)s >= skip) {
            const size_t row = (size_t)((unsigned)s - skip) * p.C + c;
            if (q.pix) p.samples[row * K + lane] = O;
            if (lane == 0) p.lar[row] = lar, p.acc[row] = accept ? 1.0f : 0.0f, p.target[row] = T;
        }
    }
    if (q.act) st[lane] = x, st[K - 1 + lane] = g;
    if (lane == 0) st[2 * K - 2] = T, st[2 * K - 1] = eps, st[2 * K] = __uint_as_float(t0 + (unsigned)p.n_steps);
}

static size_t hmc_lds_bytes(int N, int A)
{
    const size_t cells = (size_t)ceil_div(A * N, 64) * 64;
    return (68 + (cells + 4) + 2 * cells) * sizeof(float) + cells * N + (size_t)A * 64;
}

static int hmc_check_model(const char *what, const void *state, int C, int cpo, int N, const void *T8, const void *Tinv8, int A,
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

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_hmc_state_floats(int K)
{
    CTPVAE_REQUIRE(K >= 4 && K <= 64, "hmc_state_floats: 4 <= K <= 64 (got %d)", K);
    return 2 * K + 1;
}

int ctpvae_hmc_init_f32(float *state_dev, int C, int chains_per_object, int N, const float *T8_dev, const float *Tinv8_dev, int A,
                        const float *mask_dev, const float *meas_dev, float pnm, int M, const float *logw_dev, const float *alpha_dev,
                        const float *lbeta_dev, const float *start_dev, float step_size, ctpvae_stream_t stream)
{
    if (int rc = hmc_check_model("hmc_init", state_dev, C, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M, logw_dev,
                                 alpha_dev, lbeta_dev))
        return rc;
    CTPVAE_REQUIRE(step_size > 0.0f, "hmc_init: the step size must be positive (got %g)", (double)step_size);
    HmcParams p{};
    p.state = state_dev, p.first_chain = 0, p.cpo = chains_per_object, p.N = N, p.K = N * N, p.A = A, p.npass = ceil_div(A * N, 64);
    p.T8 = T8_dev, p.Tinv8 = Tinv8_dev, p.mask = mask_dev, p.meas = meas_dev, p.pnm = pnm;
    p.M = M, p.logw = logw_dev, p.alpha = alpha_dev, p.lbeta = lbeta_dev;
    p.start = start_dev, p.step_size = step_size, p.C = C;
    hipLaunchKernelGGL(hmc_kernel<true>, dim3(C), dim3(64), hmc_lds_bytes(N, A), (hipStream_t)stream, p);
    CTPVAE_LAUNCH_CHECK("hmc_kernel<init>");
    return CTPVAE_OK;
}

int ctpvae_hmc_run_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                       const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                       const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps, unsigned n_keep_from,
                       unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev, float *lar_out_dev,
                       float *accepted_out_dev, float *target_out_dev, ctpvae_stream_t stream)
{
    if (int rc = hmc_check_model("hmc_run", state_dev, C, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M, logw_dev,
                                 alpha_dev, lbeta_dev))
        return rc;
    CTPVAE_REQUIRE(samples_out_dev && lar_out_dev && accepted_out_dev && target_out_dev, "hmc_run: null output pointer");
    CTPVAE_REQUIRE(L >= 1 && L <= CTPVAE_HMC_MAX_LEAPFROGS, "hmc_run: 1 .. %d leapfrog steps (got %d)", CTPVAE_HMC_MAX_LEAPFROGS, L);
    CTPVAE_REQUIRE(n_steps >= 1 && n_steps <= CTPVAE_HMC_MAX_STEPS, "hmc_run: 1 .. %d transitions per launch (got %d)",
                   CTPVAE_HMC_MAX_STEPS, n_steps);
    HmcParams p{};
    p.state = state_dev, p.first_chain = first_chain, p.cpo = chains_per_object, p.N = N, p.K = N * N, p.A = A;
    p.npass = ceil_div(A * N, 64);
    p.T8 = T8_dev, p.Tinv8 = Tinv8_dev, p.mask = mask_dev, p.meas = meas_dev, p.pnm = pnm;
    p.M = M, p.logw = logw_dev, p.alpha = alpha_dev, p.lbeta = lbeta_dev;
    p.L = L, p.n_steps = n_steps, p.keep_from = n_keep_from, p.n_adapt = num_adaptation_steps;
    p.k0 = (unsigned)seed, p.k1 = (unsigned)(seed >> 32);
    p.samples = samples_out_dev, p.lar = lar_out_dev, p.acc = accepted_out_dev, p.target = target_out_dev, p.C = C;
    hipLaunchKernelGGL(hmc_kernel<false>, dim3(C), dim3(64), hmc_lds_bytes(N, A), (hipStream_t)stream, p);
    CTPVAE_LAUNCH_CHECK("hmc_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
