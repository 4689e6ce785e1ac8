// hmc_wg.hip -- the HMC sampler of hmc.hip for objects beyond 64 pixels: one WORKGROUP of W = ceil(K / 64) waves per chain (W <= 16),
// thread k holds pixel k and coordinate x_k, K = N * N, 2 <= N <= 32.  An init kernel and a persistent run kernel, as in hmc.hip.
//
// Everything hmc.hip's header states holds here unchanged: the density, the clamp O' = max(O, FLT_MIN), the mixture of at most 4
// Dirichlets, the tape's gradient, the leapfrog and the accept test (a NaN ratio rejects), the step-size rule, the state of 2K + 1
// floats, and the Philox counters (t, chain, block, 0x484D43) -- the momenta of coordinates 4b .. 4b+3 from block b (now up to 255),
// block 0xFFFFFFFF for the accept test's u.  The expressions are hmc.h's, term for term (this file is compiled with
// -ffp-contract=off like hmc.hip); tests/np_twin_hmc.py is the specification at every N.
//
// Orders of the sums (fixed, so that a chain's bits do not depend on how it was launched).  Wave w = threads 64w .. 64w+63:
//   scans      (the bijector's log r; the suffix sums of the inverse bijector and of the gradient)  every wave runs wave_scan_incl
//              (hmc.h) on its own 64 values and its lane 63 leaves the wave's total in LDS.  A thread of wave w adds the totals of the
//              waves 0 .. w-1 ascending, ((t_0 + t_1) + ...) + t_(w-1), and then adds its in-wave value to that; a thread of wave 0
//              adds nothing.  The suffix scan is the same on the mirrored order: thread k sits at position 64 W - 1 - k, so wave w is
//              mirrored wave W-1-w and its threads add the totals of the waves W-1, W-2, .. w+1 in that order.
//   chain sums (the prior's, fldj, |p|^2, the likelihood)  wave_sum (loglik_math.h) per wave, then the W wave sums ascending,
//              ((s_0 + s_1) + ...) + s_(W-1); with W = 1 there is no further addition.  Idle threads k >= K add +0.0f.
//   ray-sums   sinogram entry e = a * N + j belongs to thread e % (64 W), pass e / (64 W); rows i = 0 .. N-1 ascending from +0.0f;
//              a thread adds its likelihood terms over its passes ascending from +0.0f.  Entries past A * N do not exist: a thread
//              without one adds nothing (the wave form adds -0.0f there, which changes no bit).
//   G_k        angles ascending from +0.0f.
// A workgroup of one wave (N <= 8) therefore does exactly the operations of hmc.hip's kernel: the two forms agree bit for bit there
// (tests/test_gpu_hmc_wg.py), which anchors this file to the one that is held to float64 at every N <= 8.
//
// Projector taps: evaluated once per launch with the unfused fp32 expressions of hmc_setup (hmc.h) into LDS tables.  A forward tap
// needs 11 bits (K <= 1024 pixels and the zero cell, index K): ftap [N][A N] of 16 bits, row i of entry e at i * A N + e, so the
// threads of a pass read consecutive half-words; btap [A][K] bytes (the bin, or 255: no bin).  Nothing is padded to whole passes.
//
// LDS (hmc_wg_lds_bytes): O [K + 1], g [A N + 1], meas [A N], mask [A N] (each rounded up to 4 floats), ten rows of 16 floats for the
// waves' totals and sums (every reduction has a row of its own, and two uses of a row are always more than one barrier apart),
// ftap, btap.  32 x 32 at 20 angles takes 74 KiB, 16 x 16 at 90 angles 88 KiB; a request above 160 KiB is refused on the host.
//
// Barriers: every __syncthreads() is reached by all 64 W threads -- they sit in straight-line code or under conditions that are
// launch arguments (M, want_T, the step index); threads k >= K run everything with +0.0f.  Four per evaluation of the target, two
// per transition.  No atomics, every loop's trip count is a launch argument (N, A, npass, W, M, L, n_steps).
#include <atomic>

#include "hmc.h"

namespace ctpvae {

constexpr int kHmcWgMaxN = 32;
constexpr int kHmcWgRows = 10;   // rows of 16 floats: 0 scan, 1 suffix scan, 2 .. 5 the prior's components, 6 fldj, 7 lik, 8 |p|^2 before, 9 after
enum { kRowScan = 0, kRowSuffix = 1, kRowPrior = 2, kRowFldj = 6, kRowLik = 7, kRowKin0 = 8, kRowKin1 = 9 };

struct HmcWgLds {
    float *O, *g, *meas, *mask, *red;
    unsigned short *ftap;
    unsigned char *btap;
};
struct HmcWgThread {
    int k, lane, wave, W, N, K, A, AN, npass, M;
    bool act, pix;          // thread holds a coordinate of x / a pixel
    float c, kmj, pnm;      // log(K-1-k), K - k
    float am1[4], logw[4], lbeta[4];
};

inline size_t hmc_wg_up4(size_t n) { return (n + 3) & ~(size_t)3; }
inline size_t hmc_wg_lds_bytes(int N, int A)
{
    const size_t K = (size_t)N * N, AN = (size_t)A * N;
    const size_t floats = hmc_wg_up4(K + 1) + hmc_wg_up4(AN + 1) + 2 * hmc_wg_up4(AN) + kHmcWgRows * 16;
    return floats * sizeof(float) + hmc_wg_up4(AN * N * sizeof(unsigned short)) + (size_t)A * K;
}

// ((r_0 + r_1) + ...) + r_(W-1) of a row that every wave has written and a barrier has passed
__device__ __forceinline__ float hmc_wg_total(const float *row, int W)
{
    float t = row[0];
    for (int j = 1; j < W; ++j) t += row[j];
    return t;
}
// the chain sum of v: one barrier
__device__ __forceinline__ float hmc_wg_sum(float v, float *row, const HmcWgThread &q)
{
    const float s = wave_sum(v);
    if (q.lane == 0) row[q.wave] = s;
    __syncthreads();
    return hmc_wg_total(row, q.W);
}
// sum over the threads above this one (the header's mirrored scan): one barrier
__device__ __forceinline__ float hmc_wg_suffix_excl(float v, float *row, const HmcWgThread &q)
{
    const float inc = wave_scan_incl(__shfl(v, 63 - q.lane));
    const float up = __shfl(inc, 62 - q.lane);   // lane 63 reads lane 63 (the index wraps): not used below
    if (q.lane == 63) row[q.wave] = inc;
    __syncthreads();
    if (q.wave == q.W - 1) return q.lane < 63 ? up : 0.0f;
    float pre = row[q.W - 1];
    for (int j = q.W - 2; j >= 1; --j) {
        const float t = row[j];
        pre = j > q.wave ? pre + t : pre;
    }
    return q.lane < 63 ? pre + up : pre;
}

// hmc_simplex (hmc.h) with the scan over the workgroup: one barrier
__device__ __forceinline__ HmcSimplex hmc_wg_simplex(float x, const HmcWgThread &q, const HmcWgLds &m)
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
    float *row = m.red + kRowScan * 16;
    if (q.lane == 63) row[q.wave] = inc;
    __syncthreads();
    if (q.wave == 0) {
        s.logr = q.lane == 0 ? 0.0f : prev;
    } else {
        float pre = row[0];
        for (int j = 1; j < q.W - 1; ++j) {
            const float v = row[j];
            pre = j < q.wave ? pre + v : pre;
        }
        s.logr = q.lane == 0 ? pre : pre + prev;
    }
    s.logO = s.lz + s.logr;
    s.O = q.pix ? expf(s.logO) : 0.0f;
    return s;
}

// hmc_eval (hmc.h): T (when want_T is set) and dT/dx at x; sp: the bijector's values there.  Four barriers.
__device__ __forceinline__ void hmc_wg_eval(float x, bool want_T, const HmcWgThread &q, const HmcWgLds &m, HmcSimplex &sp, float &T,
                                            float &grad)
{
    sp = hmc_wg_simplex(x, q, m);
    const bool bind = sp.O < FLT_MIN;
    const float Oc = bind ? FLT_MIN : sp.O, logOc = bind ? kHmcLogFltMin : sp.logO;
    if (q.pix) m.O[q.k] = Oc;
    // the wave sums of the prior's components and of fldj travel behind the same barrier as O
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < q.M) {
            const float s = wave_sum(q.pix ? q.am1[k] * logOc : 0.0f);
            if (q.lane == 0) m.red[(kRowPrior + k) * 16 + q.wave] = s;
        }
    if (want_T) {
        const float s = wave_sum(q.act ? (sp.lz + sp.l1mz) + sp.logr : 0.0f);
        if (q.lane == 0) m.red[kRowFldj * 16 + q.wave] = s;
    }
    __syncthreads();
    const int threads = q.W * 64;
    float lp = 0.0f;
    for (int pass = 0; pass < q.npass; ++pass) {
        const int e = pass * threads + q.k;
        if (e < q.AN) {
            const unsigned short *tap = m.ftap + e;
            float proj = 0.0f;
            for (int i = 0; i < q.N; ++i) proj += m.O[tap[i * q.AN]];
            const float mk = m.mask[e], xm = m.meas[e];
            m.g[e] = poisson_dlogp(proj, mk, xm, q.pnm);
            if (want_T) lp += poisson_logp(proj, mk, xm, q.pnm);
        }
    }
    if (want_T) {
        const float s = wave_sum(lp);
        if (q.lane == 0) m.red[kRowLik * 16 + q.wave] = s;
    }
    __syncthreads();
    float G = 0.0f;
    if (q.pix)
        for (int a = 0; a < q.A; ++a) {
            const int b = m.btap[a * q.K + q.k];
            G += m.g[b == 255 ? q.AN : a * q.N + b];
        }
    // the mixture: a_m = log of component m's weighted density, softmax over m
    float am[4], mx = -__builtin_inff();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        am[k] = -__builtin_inff();
        if (k < q.M) {
            const float s = hmc_wg_total(m.red + (kRowPrior + k) * 16, q.W);
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
    const float above = hmc_wg_suffix_excl(w, m.red + kRowSuffix * 16, q);
    grad = q.act ? (w * sp.omz - sp.z * above) + (1.0f - q.kmj * sp.z) : 0.0f;
    if (want_T) {
        const float prior = mx + logf(den);
        const float lik = hmc_wg_total(m.red + kRowLik * 16, q.W);
        const float fldj = hmc_wg_total(m.red + kRowFldj * 16, q.W);
        T = (prior + lik) + fldj;
    }
}

// hmc_setup (hmc.h) for chain c = blockIdx.x: the thread's constants q, the LDS layout m over `lds` (hmc_wg_lds_bytes() bytes) and
// the tables in it.  Ends with the barrier that orders the tables before their first read.
__device__ __forceinline__ void hmc_wg_setup(const HmcParams &p, float *lds, HmcWgLds &m, HmcWgThread &q)
{
    const int k = threadIdx.x, c = blockIdx.x;
    const int N = p.N, K = p.K, A = p.A, AN = A * N;
    const int W = (K + 63) >> 6, threads = W * 64;
    const int up_an = (AN + 3) & ~3;
    m.O = lds;                                           // [K] pixels + the zero cell
    m.g = m.O + ((K + 1 + 3) & ~3);                      // [A N] + the zero cell
    m.meas = m.g + ((AN + 1 + 3) & ~3);                  // [A N]
    m.mask = m.meas + up_an;                             // [A N]
    m.red = m.mask + up_an;                              // [kHmcWgRows][16]
    m.ftap = reinterpret_cast<unsigned short *>(m.red + kHmcWgRows * 16);                                 // [N][A N]
    m.btap = reinterpret_cast<unsigned char *>(m.ftap) + (((size_t)AN * N * sizeof(unsigned short) + 3) & ~(size_t)3);   // [A][K]
    q.k = k, q.lane = k & 63, q.wave = k >> 6, q.W = W, q.N = N, q.K = K, q.A = A, q.AN = AN, q.npass = p.npass, q.M = p.M;
    q.act = k < K - 1, q.pix = k < K;
    q.c = q.act ? logf((float)(K - 1 - k)) : 0.0f;
    q.kmj = (float)(K - k);
    q.pnm = p.pnm;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool on = i < p.M;
        q.am1[i] = (on && q.pix) ? p.alpha[i * K + k] - 1.0f : 0.0f;
        q.logw[i] = on ? p.logw[i] : 0.0f;
        q.lbeta[i] = on ? p.lbeta[i] : 0.0f;
    }

    // ---- the launch's tables
    const int obj = c / p.cpo;
    if (k == 0) m.O[K] = 0.0f, m.g[AN] = 0.0f;
    for (int pass = 0; pass < p.npass; ++pass) {
        const int e = pass * threads + k;
        if (e < AN) {
            const int a = e / N, j = e - a * N;
            m.meas[e] = p.meas[(size_t)obj * AN + e];
            m.mask[e] = p.mask[(size_t)obj * A + a];
            const float *t = p.T8 + 8 * a;
            const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4], t5 = t[5];
            const float xj = t0 * (float)j, yj = t3 * (float)j;
            for (int i = 0; i < N; ++i) {
                const float fi = (float)i;
                const float x = (xj + t1 * fi) + t2;
                const float y = (yj + t4 * fi) + t5;
                const int ix = (int)__builtin_roundf(x), iy = (int)__builtin_roundf(y);
                const bool hit = (unsigned)iy < (unsigned)N && (unsigned)ix < (unsigned)N;
                m.ftap[(size_t)i * AN + e] = (unsigned short)(hit ? iy * N + ix : K);
            }
        }
    }
    if (q.pix) {
        const int r = k / N, col = k - r * N;
        const float fx = (float)col, fy = (float)r;
        for (int a = 0; a < A; ++a) {
            const float *t = p.Tinv8 + 8 * a;
            const float x = (t[0] * fx + t[1] * fy) + t[2];
            const float y = (t[3] * fx + t[4] * fy) + t[5];
            const int ix = (int)__builtin_roundf(x), iy = (int)__builtin_roundf(y);
            const bool hit = (unsigned)iy < (unsigned)N && (unsigned)ix < (unsigned)N;
            m.btap[a * K + k] = (unsigned char)(hit ? ix : 255);
        }
    }
    __syncthreads();
}

// hmc_transition (hmc.h): one whole transition of step t.  Leaves the log accept ratio in lar and returns the decision, the same
// in every thread of the workgroup (all of them compute it from the same LDS words).
__device__ __forceinline__ bool hmc_wg_transition(const HmcParams &p, const HmcWgThread &q, const HmcWgLds &m, unsigned t, unsigned chain,
                                                  HmcChain &s, float &lar)
{
    const int k = q.k;
    HmcSimplex sp;
    float mom;
    {
        const Philox4 b = philox4x32_10(t, chain, (unsigned)(k >> 2), kHmcTag, p.k0, p.k1);
        const bool hi = (k & 2) != 0;
        const float u1 = hmc_u24(hi ? b.w[2] : b.w[0]), u2 = hmc_u24(hi ? b.w[3] : b.w[1]);
        const float r = sqrtf(-2.0f * logf(u1)), ang = kTwoPi * u2;
        mom = q.act ? ((k & 1) ? r * sinf(ang) : r * cosf(ang)) : 0.0f;
    }
    const float kin0 = 0.5f * hmc_wg_sum(mom * mom, m.red + kRowKin0 * 16, q);
    const float half = 0.5f * s.eps;
    mom = mom + half * s.g;
    float xn = s.x, Tn = 0.0f, gn = 0.0f;
    for (int l = 0; l < p.L; ++l) {
        const bool last = l == p.L - 1;
        xn = xn + s.eps * mom;
        hmc_wg_eval(xn, last, q, m, sp, Tn, gn);
        mom = mom + (last ? half : s.eps) * gn;
    }
    const float kin1 = 0.5f * hmc_wg_sum(mom * mom, m.red + kRowKin1 * 16, q);
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

template <bool INIT>
__global__ __launch_bounds__(1024) void hmc_wg_kernel(HmcParams p)
{
    extern __shared__ float lds[];
    const int k = threadIdx.x, c = blockIdx.x;
    const int K = p.K;
    HmcWgLds m;
    HmcWgThread q;
    hmc_wg_setup(p, lds, m, q);

    float *st = p.state + (size_t)c * (2 * K + 1);
    if constexpr (INIT) {
        float x = 0.0f;
        if (p.start != nullptr) {
            // the inverse bijector: z_k = O_k / sum_{j>=k} O_j, x_k = (log O_k - log sum_{j>k} O_j) + log(K-1-k)
            const float v = q.pix ? p.start[(size_t)c * K + k] : 0.0f;
            const float above = hmc_wg_suffix_excl(v, m.red + kRowSuffix * 16, q);
            x = q.act ? (logf(v) - logf(above)) + q.c : 0.0f;
        }
        HmcSimplex sp;
        float T = 0.0f, g = 0.0f;
        hmc_wg_eval(x, true, q, m, sp, T, g);
        if (q.act) st[k] = x, st[K - 1 + k] = g;
        if (k == 0) st[2 * K - 2] = T, st[2 * K - 1] = p.step_size, st[2 * K] = __uint_as_float(0u);
        return;
    }

    HmcChain s;
    s.x = q.act ? st[k] : 0.0f, s.g = q.act ? st[K - 1 + k] : 0.0f;
    s.T = st[2 * K - 2], s.eps = st[2 * K - 1];
    const unsigned t0 = __float_as_uint(st[2 * K]);
    s.O = hmc_wg_simplex(s.x, q, m).O;
    const unsigned chain = p.first_chain + (unsigned)c;
    // rows of the outputs: the first kept step of this launch is row 0
    const unsigned skip = p.keep_from > t0 ? p.keep_from - t0 : 0u;

    for (int i = 0; i < p.n_steps; ++i) {
        float lar;
        const bool accept = hmc_wg_transition(p, q, m, t0 + (unsigned)i, chain, s, lar);
        if ((unsigned)i >= skip) {
            const size_t row = (size_t)((unsigned)i - skip) * p.C + c;
            if (q.pix) p.samples[row * K + k] = s.O;
            if (k == 0) p.lar[row] = lar, p.acc[row] = accept ? 1.0f : 0.0f, p.target[row] = s.T;
        }
    }
    if (q.act) st[k] = s.x, st[K - 1 + k] = s.g;
    if (k == 0) st[2 * K - 2] = s.T, st[2 * K - 1] = s.eps, st[2 * K] = __uint_as_float(t0 + (unsigned)p.n_steps);
}

static int hmc_wg_check_model(const char *what, const void *state, int C, int cpo, int N, const void *T8, const void *Tinv8, int A,
                              const void *mask, const void *meas, float pnm, int M, const void *logw, const void *alpha, const void *lbeta)
{
    CTPVAE_REQUIRE(state && T8 && Tinv8 && mask && meas && logw && alpha && lbeta, "%s: null pointer", what);
    CTPVAE_REQUIRE(C > 0 && cpo > 0 && C % cpo == 0, "%s: need C > 0 chains, a multiple of chains_per_object > 0 (got C=%d, %d per object)",
                   what, C, cpo);
    CTPVAE_REQUIRE(N >= 2 && N <= kHmcWgMaxN, "%s: objects of 2 x 2 .. %d x %d pixels only, one pixel per thread (got N=%d)", what,
                   kHmcWgMaxN, kHmcWgMaxN, N);
    CTPVAE_REQUIRE(A >= 1 && A <= CTPVAE_HMC_MAX_ANGLES, "%s: 1 .. %d angles (got A=%d)", what, CTPVAE_HMC_MAX_ANGLES, A);
    CTPVAE_REQUIRE(pnm > 0.0f, "%s: the noise multiplier must be positive (got %g)", what, (double)pnm);
    CTPVAE_REQUIRE(M >= 1 && M <= CTPVAE_HMC_MAX_COMPONENTS, "%s: 1 .. %d mixture components (got M=%d)", what, CTPVAE_HMC_MAX_COMPONENTS, M);
    const size_t bytes = hmc_wg_lds_bytes(N, A);
    CTPVAE_REQUIRE(bytes <= (size_t)kMaxLdsBytes, "%s: N=%d, A=%d need %zu bytes of LDS per chain, a workgroup has %d: fewer angles", what, N,
                   A, bytes, kMaxLdsBytes);
    return CTPVAE_OK;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

int ctpvae_hmc_wg_state_floats(int K)
{
    CTPVAE_REQUIRE(K >= 4 && K <= kHmcWgMaxN * kHmcWgMaxN, "hmc_wg_state_floats: 4 <= K <= %d (got %d)", kHmcWgMaxN * kHmcWgMaxN, K);
    return 2 * K + 1;
}

long long ctpvae_hmc_wg_lds_bytes(int N, int A)
{
    CTPVAE_REQUIRE(N >= 2 && N <= kHmcWgMaxN, "hmc_wg_lds_bytes: 2 <= N <= %d (got %d)", kHmcWgMaxN, N);
    CTPVAE_REQUIRE(A >= 1 && A <= CTPVAE_HMC_MAX_ANGLES, "hmc_wg_lds_bytes: 1 .. %d angles (got A=%d)", CTPVAE_HMC_MAX_ANGLES, A);
    return (long long)hmc_wg_lds_bytes(N, A);
}

int ctpvae_hmc_wg_resident_chains(int N, int A, int *chains_out)
{
    static std::atomic<unsigned long long> attr_set{0};
    CTPVAE_REQUIRE(chains_out, "hmc_wg_resident_chains: null pointer");
    CTPVAE_REQUIRE(N >= 2 && N <= kHmcWgMaxN, "hmc_wg_resident_chains: 2 <= N <= %d (got %d)", kHmcWgMaxN, N);
    CTPVAE_REQUIRE(A >= 1 && A <= CTPVAE_HMC_MAX_ANGLES, "hmc_wg_resident_chains: 1 .. %d angles (got A=%d)", CTPVAE_HMC_MAX_ANGLES, A);
    const size_t bytes = hmc_wg_lds_bytes(N, A);
    CTPVAE_REQUIRE(bytes <= (size_t)kMaxLdsBytes, "hmc_wg_resident_chains: N=%d, A=%d need %zu bytes of LDS per chain, a workgroup has %d",
                   N, A, bytes, kMaxLdsBytes);
    int dev = 0, cus = 0, per_cu = 0;
    CTPVAE_HIP(hipGetDevice(&dev));
    CTPVAE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    CTPVAE_SET_MAX_LDS_ONCE(hmc_wg_kernel<false>, attr_set);
    CTPVAE_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hmc_wg_kernel<false>, 64 * ceil_div(N * N, 64), bytes));
    *chains_out = cus * (per_cu > 0 ? per_cu : 1);
    return CTPVAE_OK;
}

int ctpvae_hmc_wg_init_f32(float *state_dev, int C, int chains_per_object, int N, const float *T8_dev, const float *Tinv8_dev, int A,
                           const float *mask_dev, const float *meas_dev, float pnm, int M, const float *logw_dev, const float *alpha_dev,
                           const float *lbeta_dev, const float *start_dev, float step_size, ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    if (int rc = hmc_wg_check_model("hmc_wg_init", state_dev, C, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M,
                                    logw_dev, alpha_dev, lbeta_dev))
        return rc;
    CTPVAE_REQUIRE(step_size > 0.0f, "hmc_wg_init: the step size must be positive (got %g)", (double)step_size);
    const int threads = 64 * ceil_div(N * N, 64);
    HmcParams p{};
    p.state = state_dev, p.first_chain = 0, p.cpo = chains_per_object, p.N = N, p.K = N * N, p.A = A, p.npass = ceil_div(A * N, threads);
    p.T8 = T8_dev, p.Tinv8 = Tinv8_dev, p.mask = mask_dev, p.meas = meas_dev, p.pnm = pnm;
    p.M = M, p.logw = logw_dev, p.alpha = alpha_dev, p.lbeta = lbeta_dev;
    p.start = start_dev, p.step_size = step_size, p.C = C;
    CTPVAE_SET_MAX_LDS_ONCE(hmc_wg_kernel<true>, attr_set);
    hipLaunchKernelGGL(hmc_wg_kernel<true>, dim3(C), dim3(threads), hmc_wg_lds_bytes(N, A), (hipStream_t)stream, p);
    CTPVAE_LAUNCH_CHECK("hmc_wg_kernel<init>");
    return CTPVAE_OK;
}

int ctpvae_hmc_wg_run_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                          const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                          const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps, unsigned n_keep_from,
                          unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev, float *lar_out_dev,
                          float *accepted_out_dev, float *target_out_dev, ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    if (int rc = hmc_wg_check_model("hmc_wg_run", state_dev, C, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M,
                                    logw_dev, alpha_dev, lbeta_dev))
        return rc;
    CTPVAE_REQUIRE(samples_out_dev && lar_out_dev && accepted_out_dev && target_out_dev, "hmc_wg_run: null output pointer");
    CTPVAE_REQUIRE(L >= 1 && L <= CTPVAE_HMC_MAX_LEAPFROGS, "hmc_wg_run: 1 .. %d leapfrog steps (got %d)", CTPVAE_HMC_MAX_LEAPFROGS, L);
    CTPVAE_REQUIRE(n_steps >= 1 && n_steps <= CTPVAE_HMC_MAX_STEPS, "hmc_wg_run: 1 .. %d transitions per launch (got %d)",
                   CTPVAE_HMC_MAX_STEPS, n_steps);
    const int threads = 64 * ceil_div(N * N, 64);
    HmcParams p = hmc_run_params(state_dev, C, first_chain, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M, logw_dev,
                                 alpha_dev, lbeta_dev, L, n_steps, n_keep_from, num_adaptation_steps, seed, samples_out_dev, lar_out_dev,
                                 accepted_out_dev, target_out_dev);
    p.npass = ceil_div(A * N, threads);      // passes of the 64 W threads over the sinogram
    CTPVAE_SET_MAX_LDS_ONCE(hmc_wg_kernel<false>, attr_set);
    hipLaunchKernelGGL(hmc_wg_kernel<false>, dim3(C), dim3(threads), hmc_wg_lds_bytes(N, A), (hipStream_t)stream, p);
    CTPVAE_LAUNCH_CHECK("hmc_wg_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
