// hmc_marginals.hip -- the HMC sampler's transitions (hmc.hip states them; hmc.h holds their code) with the chains' per-pixel marginals
// accumulated inside the persistent launch: a histogram over all chains of an object, two float64 moments per chain, pixel and half of
// the kept steps (what split R-hat needs), and the number of accepted kept steps per chain.  The four per-step outputs of
// ctpvae_hmc_run_f32 are optional here: all four or none.  With none, a launch writes nothing that grows with the number of steps.
//
// The transition, the random numbers, the adaptation and the carried state are hmc_kernel<false>'s, by the same functions of hmc.h;
// this file is compiled with the same flags.  After the accept test of every KEPT step t (t >= n_keep_from), with O the simplex point
// the run kernel stores as the sample, lane k < K adds, in this order:
//   counts    cnt[k][marginals_bin(O_k, lo, width, bins)] += 1, the bin rule of marginals.h (a NaN goes to column 0).  cnt is the
//             chain's own [K][bins + 2] table of 32-bit counts in LDS (a launch has at most CTPVAE_HMC_MAX_STEPS steps), zeroed when
//             the launch starts; lane k alone touches row k, so the adds are plain.  When the launch ends the wave adds the table into
//             hist [B][K][bins + 2] of object c / chains_per_object, one 64-bit integer atomic per non-zero cell.  Integer addition
//             commutes: the chains of an object, and the launches of a run, may arrive in any order.
//   moments   s1 += (double)O_k, s2 += (double)O_k * (double)O_k (exact: the square of a float fits a double) into the pair of the
//             step's half: half 0 while t < half_from, half 1 from there on.  The pairs live in mom [2 halves][2 moments][C][K]; a
//             launch loads the pair of its first kept step, swaps pairs at the boundary (stores one, loads the other) and stores what
//             it holds when it ends.  So sum (h, c, k) is ((s + O_t1) + O_t2) + ... over the kept steps of half h ascending, whatever
//             the cut into launches; no other chain's value enters it, and there are no floating-point atomics.
//   accepted  lane 0 counts the accepted kept steps; accepted[c] += that count when the launch ends (the chain owns the cell).
//
// LDS: the sampler's hmc_lds_bytes(N, A) (at most 57 KiB: 8 x 8, 256 angles) followed by the count table, K * (bins + 2) * 4 bytes (at
// most 64 KiB: 64 pixels, 254 bins): up to 121 KiB, above the 64 KiB a kernel gets by default, so the entry point raises the limit
// (CTPVAE_SET_MAX_LDS_ONCE).  One wave per workgroup as in hmc.hip: no wave waits on another.
#include "hmc.h"
#include "marginals.h"

namespace ctpvae {

struct HmcStats {
    unsigned half_from;              // index of the first step of half 1
    float lo, width;
    int bins;
    unsigned long long *hist;        // [B][K][bins + 2]
    double *mom;                     // [2][2][C][K]
    unsigned long long *accepted;    // [C]
};

__global__ __launch_bounds__(64) void hmc_stats_kernel(HmcParams p, HmcStats h)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x, c = blockIdx.x;
    const int K = p.K, cols = h.bins + 2;
    HmcLds m;
    HmcLane q;
    hmc_setup(p, lds, m, q);
    unsigned *cnt = reinterpret_cast<unsigned *>(m.btap + (size_t)p.A * 64);   // [K][cols], at byte hmc_lds_bytes(N, A): a multiple of 16
    for (int i = lane; i < K * cols; i += 64) cnt[i] = 0u;
    __syncthreads();
    unsigned *row = cnt + lane * cols;    // read by lanes < K only

    float *st = p.state + (size_t)c * (2 * K + 1);
    unsigned t0;
    HmcChain s = hmc_load_chain(st, K, q, t0);
    const unsigned chain = p.first_chain + (unsigned)c;
    const unsigned skip = p.keep_from > t0 ? p.keep_from - t0 : 0u;
    const bool per_step = p.samples != nullptr;

    // pair (half hf) of this lane's pixel: s1 at mom[2 hf][c][lane], s2 at mom[2 hf + 1][c][lane]
    const size_t CK = (size_t)p.C * K;
    double *pair = h.mom + (size_t)c * K + lane;
    int cur = t0 + skip >= h.half_from ? 1 : 0;
    double s1 = 0.0, s2 = 0.0;
    if (q.pix) s1 = pair[(size_t)(2 * cur) * CK], s2 = pair[(size_t)(2 * cur + 1) * CK];
    unsigned n_acc = 0u;

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
            if (q.pix) {
                row[marginals_bin(s.O, h.lo, h.width, h.bins)] += 1u;
                const double xd = (double)s.O;
                s1 += xd;
                s2 += xd * xd;
            }
            n_acc += accept ? 1u : 0u;
        }
    }
    hmc_store_chain(st, K, q, s, t0 + (unsigned)p.n_steps);
    if (q.pix) pair[(size_t)(2 * cur) * CK] = s1, pair[(size_t)(2 * cur + 1) * CK] = s2;
    if (lane == 0 && n_acc != 0u) h.accepted[c] += n_acc;
    __syncthreads();
    unsigned long long *hist = h.hist + (size_t)(c / p.cpo) * K * cols;
    for (int i = lane; i < K * cols; i += 64) {
        const unsigned v = cnt[i];
        if (v != 0u) atomicAdd(hist + i, (unsigned long long)v);
    }
}

static size_t hmc_stats_lds_bytes(int N, int A, int bins) { return hmc_lds_bytes(N, A) + (size_t)N * N * (bins + 2) * sizeof(unsigned); }

}  // namespace ctpvae

using namespace ctpvae;

extern "C" {

long long ctpvae_hmc_marginals_lds_bytes(int N, int A, int bins)
{
    CTPVAE_REQUIRE(N >= 2 && N <= 8, "hmc_marginals_lds_bytes: objects of 2 x 2 .. 8 x 8 pixels only (got N=%d)", N);
    CTPVAE_REQUIRE(A >= 1 && A <= CTPVAE_HMC_MAX_ANGLES, "hmc_marginals_lds_bytes: 1 .. %d angles (got A=%d)", CTPVAE_HMC_MAX_ANGLES, A);
    CTPVAE_REQUIRE(bins >= 1 && bins <= CTPVAE_MARGINALS_MAX_BINS, "hmc_marginals_lds_bytes: bins must be 1 .. %d (got %d)",
                   CTPVAE_MARGINALS_MAX_BINS, bins);
    return (long long)hmc_stats_lds_bytes(N, A, bins);
}

int ctpvae_hmc_run_marginals_f32(float *state_dev, int C, unsigned first_chain, int chains_per_object, int N, const float *T8_dev,
                                 const float *Tinv8_dev, int A, const float *mask_dev, const float *meas_dev, float pnm, int M,
                                 const float *logw_dev, const float *alpha_dev, const float *lbeta_dev, int L, int n_steps,
                                 unsigned n_keep_from, unsigned num_adaptation_steps, unsigned long long seed, float *samples_out_dev,
                                 float *lar_out_dev, float *accepted_out_dev, float *target_out_dev, unsigned n_half_from, float lo,
                                 float width, int bins, long long *hist_dev, double *mom_dev, long long *accepted_dev,
                                 ctpvae_stream_t stream)
{
    static std::atomic<unsigned long long> attr_set{0};
    if (int rc = hmc_check_model("hmc_run_marginals", state_dev, C, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M,
                                 logw_dev, alpha_dev, lbeta_dev))
        return rc;
    const int n_out = (samples_out_dev != nullptr) + (lar_out_dev != nullptr) + (accepted_out_dev != nullptr) + (target_out_dev != nullptr);
    CTPVAE_REQUIRE(n_out == 0 || n_out == 4, "hmc_run_marginals: the four per-step outputs are given together or not at all (got %d)", n_out);
    CTPVAE_REQUIRE(L >= 1 && L <= CTPVAE_HMC_MAX_LEAPFROGS, "hmc_run_marginals: 1 .. %d leapfrog steps (got %d)", CTPVAE_HMC_MAX_LEAPFROGS, L);
    CTPVAE_REQUIRE(n_steps >= 1 && n_steps <= CTPVAE_HMC_MAX_STEPS, "hmc_run_marginals: 1 .. %d transitions per launch (got %d)",
                   CTPVAE_HMC_MAX_STEPS, n_steps);
    if (int rc = marg_grid_check("hmc_run_marginals", lo, width, bins)) return rc;
    CTPVAE_REQUIRE(hist_dev && mom_dev && accepted_dev, "hmc_run_marginals: null state pointer (hist, moments, accepted)");
    CTPVAE_REQUIRE(((size_t)hist_dev & 7) == 0 && ((size_t)mom_dev & 7) == 0 && ((size_t)accepted_dev & 7) == 0,
                   "hmc_run_marginals: hist, moments and accepted must be 8-byte aligned");
    const HmcParams p = hmc_run_params(state_dev, C, first_chain, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M,
                                       logw_dev, alpha_dev, lbeta_dev, L, n_steps, n_keep_from, num_adaptation_steps, seed,
                                       samples_out_dev, lar_out_dev, accepted_out_dev, target_out_dev);
    HmcStats h{};
    h.half_from = n_half_from, h.lo = lo, h.width = width, h.bins = bins;
    h.hist = reinterpret_cast<unsigned long long *>(hist_dev), h.mom = mom_dev;
    h.accepted = reinterpret_cast<unsigned long long *>(accepted_dev);
    CTPVAE_SET_MAX_LDS_ONCE(hmc_stats_kernel, attr_set);
    hipLaunchKernelGGL(hmc_stats_kernel, dim3(C), dim3(64), hmc_stats_lds_bytes(N, A, bins), (hipStream_t)stream, p, h);
    CTPVAE_LAUNCH_CHECK("hmc_stats_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
