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
#include "hmc.h"

namespace ctpvae {

template <bool INIT>
__global__ __launch_bounds__(64) void hmc_kernel(HmcParams p)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x, c = blockIdx.x;
    const int K = p.K;
    HmcLds m;
    HmcLane q;
    hmc_setup(p, lds, m, q);

    float *st = p.state + (size_t)c * (2 * K + 1);
    if constexpr (INIT) {
        float x = 0.0f;
        if (p.start != nullptr) {
            // the inverse bijector: z_k = O_k / sum_{j>=k} O_j, x_k = (log O_k - log sum_{j>k} O_j) + log(K-1-k)
            const float v = q.pix ? p.start[(size_t)c * K + lane] : 0.0f;
            const float above = wave_suffix_excl(v, lane);
            x = q.act ? (logf(v) - logf(above)) + q.c : 0.0f;
        }
        HmcSimplex sp;
        float T = 0.0f, g = 0.0f;
        hmc_eval(x, true, q, m, sp, T, g);
        if (q.act) st[lane] = x, st[K - 1 + lane] = g;
        if (lane == 0) st[2 * K - 2] = T, st[2 * K - 1] = p.step_size, st[2 * K] = __uint_as_float(0u);
        return;
    }

    unsigned t0;
    HmcChain s = hmc_load_chain(st, K, q, t0);
    const unsigned chain = p.first_chain + (unsigned)c;
    // rows of the outputs: the first kept step of this launch is row 0
    const unsigned skip = p.keep_from > t0 ? p.keep_from - t0 : 0u;

    for (int i = 0; i < p.n_steps; ++i) {
        float lar;
        const bool accept = hmc_transition(p, q, m, t0 + (unsigned)i, chain, s, lar);
        if ((unsigned)i >= skip) hmc_store_step(p, q, (unsigned)i - skip, c, s, lar, accept);
    }
    hmc_store_chain(st, K, q, s, t0 + (unsigned)p.n_steps);
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
    const HmcParams p = hmc_run_params(state_dev, C, first_chain, chains_per_object, N, T8_dev, Tinv8_dev, A, mask_dev, meas_dev, pnm, M,
                                       logw_dev, alpha_dev, lbeta_dev, L, n_steps, n_keep_from, num_adaptation_steps, seed,
                                       samples_out_dev, lar_out_dev, accepted_out_dev, target_out_dev);
    hipLaunchKernelGGL(hmc_kernel<false>, dim3(C), dim3(64), hmc_lds_bytes(N, A), (hipStream_t)stream, p);
    CTPVAE_LAUNCH_CHECK("hmc_kernel");
    return CTPVAE_OK;
}

}  // extern "C"
