// hmc_diagnostics.hip -- hmc_marginals.hip's launch (the sampler's transitions with the chains' histograms, half-chain moments and
// accepted steps accumulated inside; that file's header stays the statement of those parts) with two more raw sums per chain, from
// which the host finishes the autocovariance, the effective sample size and the covariance between pixels without a stored sample.
//
// The transition, the random numbers, the adaptation and the carried state are hmc.h's, and this file is compiled with the flags of
// hmc.hip and hmc_marginals.hip.  After the accept test of kept step j = t - n_keep_from, with O the simplex point the run kernel
// stores as the sample and x = O_k, lane k < K does what hmc_stats_kernel does there and then, in this order:
//   lags      (max_lag = Lm >= 1)  ring[j mod (Lm + 1)][k] = x; if j < Lm, head[j][k] = x (written once); then for l = 0 ..
//             min(j, Lm) ascending  r[l][k] += (double)x * (double)ring[(j - l) mod (Lm + 1)][k].  ring holds the chain's last Lm + 1
//             kept values of pixel k.  The product of two floats is exact in a double, so r[l] is ((0 + p_l) + p_(l+1)) + ... over j
//             ascending, one rounding per kept step, and nothing else enters it.
//   cov       (cov on)  for i = 0 .. K - 1 ascending  xx[k][i] += (double)O_k * (double)O_i, O_i read from lane i.  Lane k alone owns
//             row k; the product commutes, so xx[k][i] and xx[i][k] see the same addends in the same order and are equal by bits.
// r, ring and xx live in LDS during a launch and in the state arrays lag [C][Lm + 1][K] float64, ring [C][Lm + 1][K] float32 and xx
// [C][K][K] float64 between launches: a launch that keeps a step loads them when it starts and stores them when it ends, as the moment
// pairs are handled; head [C][Lm][K] float32 is written straight to memory.  The bits therefore do not depend on the cut into launches
// or on how chains are spread over calls.  No floating-point atomics, and nothing that grows with the number of steps.
//
// LDS: the sampler's hmc_lds_bytes(N, A), the count table K * (bins + 2) * 4 bytes (rounded up to 8), then ring (Lm + 1) * K * 4
// (rounded up to 8), r (Lm + 1) * K * 8 and xx K * K * 8 bytes; r and xx are laid out [l][k] and [i][k], so that the lanes of a wave
// touch consecutive words.  With everything at its maximum (8 x 8, 256 angles, 254 bins, 64 lags, cov) that is 205,856 bytes, above the
// 163,840 a workgroup can have on gfx950: the run entry refuses such a request before any launch and names the knobs to lower.  One
// wave per workgroup as in hmc.hip: no wave waits on another, and every LDS cell past the sampler's block is touched by one lane only.
#include "hmc.h"
#include "marginals.h"

namespace ctpvae {

struct HmcDiag {
    unsigned half_from;              // index of the first step of half 1
    float lo, width;
    int bins;
    unsigned long long *hist;        // [B][K][bins + 2]
    double *mom;                     // [2][2][C][K]
    unsigned long long *accepted;    // [C]
    int Lm;                          // 0: no lagged products
    double *lag;                     // [C][Lm + 1][K]
    float *ring;                     // [C][Lm + 1][K]
    float *head;                     // [C][Lm][K]
    double *xx;                      // [C][K][K] or nullptr: no cross products
};

constexpr size_t hmc_diag_up8(size_t v) { return (v + 7) & ~(size_t)7; }

__global__ __launch_bounds__(64) void hmc_diag_kernel(HmcParams p, HmcDiag h)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x, c = blockIdx.x;
    const int K = p.K, cols = h.bins + 2;
    HmcLds m;
    HmcLane q;
    hmc_setup(p, lds, m, q);
    unsigned char *base = m.btap + (size_t)p.A * 64;                            // byte hmc_lds_bytes(N, A): a multiple of 16
    unsigned *cnt = reinterpret_cast<unsigned *>(base);                         // [K][cols]
    for (int i = lane; i < K * cols; i += 64) cnt[i] = 0u;
    unsigned *row = cnt + lane * cols;    // read by lanes < K only
    const int Lm = h.Lm, slots = Lm + 1;
    const bool lags = Lm > 0, cov = h.xx != nullptr;
    base += hmc_diag_up8((size_t)K * cols * sizeof(unsigned));
    float *ring = reinterpret_cast<float *>(base);                              // [slots][K]
    base += lags ? hmc_diag_up8((size_t)slots * K * sizeof(float)) : 0;
    double *r = reinterpret_cast<double *>(base);                               // [slots][K]
    base += lags ? (size_t)slots * K * sizeof(double) : 0;
    double *xx = reinterpret_cast<double *>(base);                              // [i][k]: lane k's row k, transposed

    float *st = p.state + (size_t)c * (2 * K + 1);
    unsigned t0;
    HmcChain s = hmc_load_chain(st, K, q, t0);
    const unsigned chain = p.first_chain + (unsigned)c;
    const unsigned skip = p.keep_from > t0 ? p.keep_from - t0 : 0u;
    const bool per_step = p.samples != nullptr;
    const bool keeps = skip < (unsigned)p.n_steps;       // this launch has a kept step: only then the lag and cov state moves

    // pair (half hf) of this lane's pixel: s1 at mom[2 hf][c][lane], s2 at mom[2 hf + 1][c][lane]
    const size_t CK = (size_t)p.C * K;
    double *pair = h.mom + (size_t)c * K + lane;
    int cur = t0 + skip >= h.half_from ? 1 : 0;
    double s1 = 0.0, s2 = 0.0;
    if (q.pix) s1 = pair[(size_t)(2 * cur) * CK], s2 = pair[(size_t)(2 * cur + 1) * CK];
    unsigned n_acc = 0u;

    double *lag_g = lags ? h.lag + (size_t)c * slots * K : nullptr;
    float *ring_g = lags ? h.ring + (size_t)c * slots * K : nullptr;
    float *head_g = lags ? h.head + (size_t)c * Lm * K : nullptr;
    double *xx_g = cov ? h.xx + (size_t)c * K * K : nullptr;
    if (keeps && lags)
        for (int i = lane; i < slots * K; i += 64) ring[i] = ring_g[i], r[i] = lag_g[i];
    if (keeps && cov)
        for (int e = lane; e < K * K; e += 64) {
            const int k = e / K, i = e - k * K;
            xx[i * K + k] = xx_g[e];
        }
    __syncthreads();

    unsigned j = t0 + skip - p.keep_from;                // index of the launch's first kept step among the kept steps
    int slot = (int)(j % (unsigned)slots);

    for (int i = 0; i < p.n_steps; ++i) {
        const unsigned t = t0 + (unsigned)i;
        float lar;
        const bool accept = hmc_transition(p, q, m, t, chain, s, lar);
        if ((unsigned)i >= skip) {
            if (per_step) hmc_store_step(p, q, (unsigned)i - skip, c, s, lar, accept);
            const int hf = t >= h.half_from ? 1 : 0;
            if (hf != cur) {
                if (q.pix) {
                    pair[(size_t)(2 * cur) * CK] = s1, pair[(size_t)(2 * cur + 1) * CK] = s2;
                    s1 = pair[(size_t)(2 * hf) * CK], s2 = pair[(size_t)(2 * hf + 1) * CK];
                }
                cur = hf;
            }
            const double xd = (double)s.O;
            if (q.pix) {
                row[marginals_bin(s.O, h.lo, h.width, h.bins)] += 1u;
                s1 += xd;
                s2 += xd * xd;
            }
            n_acc += accept ? 1u : 0u;
            if (lags) {
                if (q.pix) {
                    ring[slot * K + lane] = s.O;
                    if (j < (unsigned)Lm) head_g[(size_t)j * K + lane] = s.O;
                    const int top = j < (unsigned)Lm ? (int)j : Lm;
                    int at = slot;                       // (j - l) mod slots
                    for (int l = 0; l <= top; ++l) {
                        r[l * K + lane] += xd * (double)ring[at * K + lane];
                        at = at == 0 ? Lm : at - 1;
                    }
                }
                slot = slot == Lm ? 0 : slot + 1;
            }
            if (cov) {
                const int xb = __float_as_int(s.O);
                for (int i2 = 0; i2 < K; ++i2) {
                    const double oi = (double)__int_as_float(__builtin_amdgcn_readlane(xb, i2));
                    if (q.pix) xx[i2 * K + lane] += xd * oi;
                }
            }
            ++j;
        }
    }
    hmc_store_chain(st, K, q, s, t0 + (unsigned)p.n_steps);
    if (q.pix) pair[(size_t)(2 * cur) * CK] = s1, pair[(size_t)(2 * cur + 1) * CK] = s2;
    if (lane == 0 && n_acc != 0u) h.accepted[c] += n_acc;
    __syncthreads();
    if (keeps && lags)
        for (int i = lane; i < slots * K; i += 64) ring_g[i] = ring[i], lag_g[i] = r[i];
    if (keeps && cov)
        for (int e = lane; e < K * K; e += 64) {
            const int k = e / K, i = e - k * K;
            xx_g[e] = xx[i * K + k];
        }
    unsigned long long *hist = h.hist + (size_t)(c / p.cpo) * K * cols;
    for (int i = lane; i < K * cols; i += 64) {
        const unsigned v = cnt[i];
        if (v != 0u) atomicAdd(hist + i, (unsigned long long)v);
    }
}

static size_t hmc_diag_lds_bytes(int N, int A, int bins, int Lm, bool cov)
{
    const size_t K = (size_t)N * N, slots = (size_t)Lm + 1;
    size_t b = hmc_lds_bytes(N, A) + hmc_diag_up8(K * (bins + 2) * sizeof(unsigned));
    if (Lm > 0) b += hmc_diag_up8(slots * K * sizeof(float)) + slots * K * sizeof(double);
    if (cov) b += K * K * sizeof(double);
    return b;
}

static int hmc_diag_check_sizes(const char *what, int N, int A, int bins, int max_lag)
{
    CTPVAE_REQUIRE(N >= 2 && N <= 8, "%s: objects of 2 x 2 .. 8 x 8 pixels only (got N=%d)", what, N);
    CTPVAE_REQUIRE(A >= 1 && A <= CTPVAE_HMC_MAX_ANGLES, "%s: 1 .. %d angles (got A=%d)", what, CTPVAE_HMC_MAX_ANGLES, A);
    CTPVAE_REQUIRE(bins >= 1 && bins <= CTPVAE_MARGINALS_MAX_BINS, "%s: bins must be 1 .. %d (got %d)", what, CTPVAE_MARGINALS_MAX_BINS,
                   bins);
    CTPVAE_REQUIRE(max_lag >= 0 && max_lag <= CTPVAE_HMC_MAX_LAG, "%s: max_lag must be 0 .. %d (got %d)", what, CTPVAE_HMC_MAX_LAG, max_lag);
    return CTPVAE_OK;
}

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

long long ctpvae_hmc_diagnostics_lds_bytes(int N, int A, int bins, int max_lag, int cov)
{
    if (int rc = hmc_diag_check_sizes("hmc_diagnostics_lds_bytes", N, A, bins, max_lag)) return rc;
    return (long long)hmc_diag_lds_bytes(N, A, bins, max_lag, cov != 0);
}

int ctpvae_hmc_run_diagnostics_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                                   const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                                   const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps,
                                   unsigned n_keep_from, unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev,
                                   float *lar_out_dev, float *accepted_out_dev, float *target_out_dev, unsigned n_half_from, float lo,
                                   float width, int bins, long long *hist_dev, double *mom_dev, long long *accepted_dev, int max_lag,
                                   double *lag_dev, float *ring_dev, float *head_dev, double *xx_dev, ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    if (int rc = hmc_check_model("hmc_run_diagnostics", state_dev, C, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm,
                                 M, logw_dev, alpha_dev, lbeta_dev))
        return rc;
    const int n_out = (samples_out_dev != nullptr) + (lar_out_dev != nullptr) + (accepted_out_dev != nullptr) + (target_out_dev != nullptr);
    CTPVAE_REQUIRE(n_out == 0 || n_out == 4, "hmc_run_diagnostics: the four per-step outputs are given together or not at all (got %d)",
                   n_out);
    CTPVAE_REQUIRE(L >= 1 && L <= CTPVAE_HMC_MAX_LEAPFROGS, "hmc_run_diagnostics: 1 .. %d leapfrog steps (got %d)", CTPVAE_HMC_MAX_LEAPFROGS,
                   L);
    CTPVAE_REQUIRE(n_steps >= 1 && n_steps <= CTPVAE_HMC_MAX_STEPS, "hmc_run_diagnostics: 1 .. %d transitions per launch (got %d)",
                   CTPVAE_HMC_MAX_STEPS, n_steps);
    if (int rc = marg_grid_check("hmc_run_diagnostics", lo, width, bins)) return rc;
    CTPVAE_REQUIRE(hist_dev && mom_dev && accepted_dev, "hmc_run_diagnostics: null state pointer (hist, moments, accepted)");
    CTPVAE_REQUIRE(((size_t)hist_dev & 7) == 0 && ((size_t)mom_dev & 7) == 0 && ((size_t)accepted_dev & 7) == 0,
                   "hmc_run_diagnostics: hist, moments and accepted must be 8-byte aligned");
    if (int rc = hmc_diag_check_sizes("hmc_run_diagnostics", N, A, bins, max_lag)) return rc;
    if (max_lag > 0) {
        CTPVAE_REQUIRE(lag_dev && ring_dev && head_dev, "hmc_run_diagnostics: max_lag=%d needs the lag, ring and head arrays (null pointer)",
                       max_lag);
        CTPVAE_REQUIRE(((size_t)lag_dev & 7) == 0 && ((size_t)ring_dev & 3) == 0 && ((size_t)head_dev & 3) == 0,
                       "hmc_run_diagnostics: lag must be 8-byte aligned, ring and head 4-byte aligned");
    } else {
        CTPVAE_REQUIRE(!lag_dev && !ring_dev && !head_dev, "hmc_run_diagnostics: lag, ring and head arrays given with max_lag=0");
    }
    CTPVAE_REQUIRE(((size_t)xx_dev & 7) == 0, "hmc_run_diagnostics: xx must be 8-byte aligned");
    const size_t bytes = hmc_diag_lds_bytes(N, A, bins, max_lag, xx_dev != nullptr);
    CTPVAE_REQUIRE(bytes <= (size_t)kMaxLdsBytes,
                   "hmc_run_diagnostics: N=%d, A=%d, bins=%d, max_lag=%d%s need %zu bytes of LDS, a workgroup has %d: lower bins, max_lag "
                   "or turn cov off",
                   N, A, bins, max_lag, xx_dev ? ", cov" : "", bytes, kMaxLdsBytes);
    const HmcParams p = hmc_run_params(state_dev, C, first_chain, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M,
                                       logw_dev, alpha_dev, lbeta_dev, L, n_steps, n_keep_from, num_adaptation_steps, seed,
                                       samples_out_dev, lar_out_dev, accepted_out_dev, target_out_dev);
    HmcDiag h{};
    h.half_from = n_half_from, h.lo = lo, h.width = width, h.bins = bins;
    h.hist = reinterpret_cast<unsigned long long *>(hist_dev), h.mom = mom_dev;
    h.accepted = reinterpret_cast<unsigned long long *>(accepted_dev);
    h.Lm = max_lag, h.lag = lag_dev, h.ring = ring_dev, h.head = head_dev, h.xx = xx_dev;
    CTPVAE_SET_MAX_LDS_ONCE(hmc_diag_kernel, attr_set);
    hipLaunchKernelGGL(hmc_diag_kernel, dim3(C), dim3(64), bytes, (hipStream_t)stream, p, h);
    CTPVAE_LAUNCH_CHECK("hmc_diag_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
