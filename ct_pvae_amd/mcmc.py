"""HMC ground-truth posterior for small objects (bin/toy_mcmc_v2.py, ctvae/toy_mcmc_v2_functions.py of vganapati/CT_PVAE).

    hmc_sample(meas, mask, theta, pnm, *, prior=None, num_results, ...)   tfp.mcmc.sample_chain over SimpleStepSizeAdaptation(
                                                                          TransformedTransitionKernel(HamiltonianMonteCarlo,
                                                                          IteratedSigmoidCentered)) on joint_log_prob
    python -m ct_pvae_amd.mcmc --save_path D -s STEPS -b BURNIN            bin/toy_mcmc_v2.py without its plots

One 64-lane wave runs a whole chain inside one persistent kernel (csrc/hmc.hip states the density, the transition, the orders of
the sums and the layout of the random numbers); this module validates, uploads the tables and loops over launches.  There is no
CPU path.
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _lib, forward_functions
from .forward_functions import _stream_ptr, rotate_tables
from .helper_functions import toy_dist

__all__ = ["hmc_sample", "toy_dist", "MAX_STEPS_PER_LAUNCH"]

# CTPVAE_HMC_MAX_STEPS of include/ctpvae_radon.h: the largest power of two that keeps one launch of the slowest shape measured with 5
# leapfrog steps (8 x 8, 180 angles, 149 us per transition on the MI355X) under 100 ms (tools/time_hmc.py -> profiles/hmc_timing.txt).
# The default steps_per_launch is this for up to 5 leapfrog steps and shrinks in proportion above, so that a default launch stays
# near that time (the entry point's worst case, 32 leapfrog steps at 256 angles, costs 1.26 ms per transition).
MAX_STEPS_PER_LAUNCH = 512
_MAX_ANGLES, _MAX_COMPONENTS, _MAX_LEAPFROGS = 256, 4, 32


def _lgamma64(a):
    return np.vectorize(math.lgamma, otypes=[np.float64])(a)


def _prior_tables(prior, K):
    """(logw [M], alpha [M][K], lbeta [M]) as float32: the concentrations rounded to float32 once, the rest from them in float64."""
    weights, alpha = toy_dist() if prior is None else prior
    weights = np.asarray(weights, np.float64).reshape(-1)
    alpha = np.asarray(alpha, np.float64)
    alpha = alpha[None] if alpha.ndim == 1 else alpha
    M = weights.size
    if not 1 <= M <= _MAX_COMPONENTS:
        raise ValueError(f"hmc_sample: the prior is a mixture of 1 .. {_MAX_COMPONENTS} Dirichlets (got {M} weights)")
    if alpha.shape != (M, K):
        raise ValueError(f"hmc_sample: concentrations must be [{M}][{K}] for {M} components and {K} pixels (got {alpha.shape})")
    alpha = alpha.astype(np.float32).astype(np.float64)
    if not (np.all(np.isfinite(alpha)) and np.all(alpha > 0)):
        raise ValueError("hmc_sample: concentrations must be positive and finite")
    if not (np.all(np.isfinite(weights)) and np.all(weights > 0)):
        raise ValueError("hmc_sample: mixture weights must be positive and finite")
    lbeta = _lgamma64(alpha).sum(-1) - _lgamma64(alpha.sum(-1))
    return np.log(weights).astype(np.float32), alpha.astype(np.float32), lbeta.astype(np.float32)


def hmc_sample(meas, mask, theta, pnm, *, prior=None, num_results, num_burnin_steps=0, num_leapfrog_steps=5, step_size=6.5e-2,
               num_adaptation_steps=400, chains_per_object=1, initial_state=None, seed=0, first_chain=0, steps_per_launch=None):
    """Posterior samples of N x N objects (N * N <= 64) on the simplex given sparse noisy sinograms, by HMC on the GPU.

    meas [A][N] or [B][A][N] and mask [A] or [B][A]: CUDA float tensors (create_all_masks' outputs); theta [A] radians; pnm: the
    Poisson noise multiplier.  prior: (weights [M], concentrations [M][K]) of a mixture of M <= 4 Dirichlets, default toy_dist().
    C = B * chains_per_object chains run side by side, chain c on object c // chains_per_object; its random numbers depend on
    (seed, first_chain + c, step index) alone, so a run does not change with steps_per_launch or with how chains are spread over
    calls.  initial_state [C][K]: starting points inside the simplex, every entry positive and finite (default: the bijector's
    image of 0).  The step size adapts during the first num_adaptation_steps steps (burn-in included), per chain.  steps_per_launch
    (1 .. MAX_STEPS_PER_LAUNCH) defaults to that cap, divided by num_leapfrog_steps / 5 above 5 leapfrog steps.

    Returns (samples [num_results][C][K], trace) with trace = {"log_accept_ratio", "is_accepted", "target_log_prob":
    [num_results][C], "step_size": [C] after the last step}."""
    lib = _lib.load()
    if not (isinstance(meas, torch.Tensor) and isinstance(mask, torch.Tensor)):
        raise TypeError("hmc_sample: meas and mask must be torch tensors")
    if meas.dim() == 2:
        meas, mask = meas[None], (mask[None] if mask.dim() == 1 else mask)
    if meas.dim() != 3 or mask.dim() != 2:
        raise ValueError(f"hmc_sample: meas must be [A][N] or [B][A][N] and mask [A] or [B][A] (got {tuple(meas.shape)}, {tuple(mask.shape)})")
    B, A, N = meas.shape
    K = N * N
    th = np.asarray(theta.detach().cpu() if isinstance(theta, torch.Tensor) else theta, dtype=np.float32).reshape(-1)
    if K > 64:
        raise ValueError(f"hmc_sample: objects of at most 64 pixels, one per lane (got N={N}: {K} pixels)")
    if N < 2:
        raise ValueError("hmc_sample: the object needs at least 2 x 2 pixels")
    if th.size != A or tuple(mask.shape) != (B, A):
        raise ValueError(f"hmc_sample: the object is square with one detector bin per pixel column: meas [B][A][N], mask [B][A], theta [A] "
                         f"(got meas {tuple(meas.shape)}, mask {tuple(mask.shape)}, {th.size} angles)")
    if A > _MAX_ANGLES:
        raise ValueError(f"hmc_sample: at most {_MAX_ANGLES} angles (got {A})")
    logw, alpha, lbeta = _prior_tables(prior, K)
    num_results, num_burnin_steps, L = int(num_results), int(num_burnin_steps), int(num_leapfrog_steps)
    cpo = int(chains_per_object)
    if num_results < 1 or num_burnin_steps < 0 or cpo < 1 or int(num_adaptation_steps) < 0 or int(first_chain) < 0:
        raise ValueError("hmc_sample: num_results and chains_per_object must be >= 1; burn-in, adaptation steps and first_chain >= 0")
    if not 1 <= L <= _MAX_LEAPFROGS:
        raise ValueError(f"hmc_sample: 1 .. {_MAX_LEAPFROGS} leapfrog steps (got {L})")
    if not float(step_size) > 0 or not float(pnm) > 0:
        raise ValueError("hmc_sample: step_size and pnm must be positive")
    spl = max(1, MAX_STEPS_PER_LAUNCH * 5 // max(L, 5)) if steps_per_launch is None else int(steps_per_launch)
    if not 1 <= spl <= MAX_STEPS_PER_LAUNCH:
        raise ValueError(f"hmc_sample: steps_per_launch must be 1 .. {MAX_STEPS_PER_LAUNCH} (got {spl})")
    total = num_burnin_steps + num_results
    if total >= 2 ** 32:
        raise ValueError("hmc_sample: the step index is 32 bits wide")
    C = B * cpo
    if int(first_chain) + C > 2 ** 32:
        raise ValueError(f"hmc_sample: the chain id is 32 bits wide (got first_chain={int(first_chain)} and {C} chains)")
    start_h = None
    if initial_state is not None:
        # checked on the host: the kernel takes logf of every entry, and a chain started at -inf or NaN would reject for ever, silently
        start_h = (initial_state.detach().cpu() if isinstance(initial_state, torch.Tensor) else torch.as_tensor(np.asarray(initial_state)))
        start_h = start_h.to(torch.float32).contiguous()
        if tuple(start_h.shape) != (C, K):
            raise ValueError(f"hmc_sample: initial_state must be [{C}][{K}] (got {tuple(start_h.shape)})")
        if not bool((torch.isfinite(start_h) & (start_h > 0)).all()):
            raise ValueError("hmc_sample: initial_state must be positive and finite in every entry (points inside the simplex)")
    if meas.device.type != "cuda" or mask.device != meas.device:
        raise _lib.RadonLibraryError("hmc_sample: meas and mask must be CUDA tensors on one device; there is no CPU path")
    dev = meas.device
    meas_d = meas.detach().to(torch.float32).contiguous()
    mask_d = mask.detach().to(torch.float32).contiguous()
    start = start_h.to(dev) if start_h is not None else None
    T8, Tinv8 = rotate_tables(th, N, N, dev)
    prior_d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (logw, alpha, lbeta)]
    state = forward_functions._new_output((C, 2 * K + 1), torch.float32, dev)
    samples = forward_functions._new_output((num_results, C, K), torch.float32, dev)
    lar, acc, tgt = (forward_functions._new_output((num_results, C), torch.float32, dev) for _ in range(3))
    model = (N, T8.data_ptr(), Tinv8.data_ptr(), A, mask_d.data_ptr(), meas_d.data_ptr(), float(pnm), logw.size, prior_d[0].data_ptr(),
             prior_d[1].data_ptr(), prior_d[2].data_ptr())
    with torch.cuda.device(dev):
        stream = _stream_ptr()
        _lib.check(lib.ctpvae_hmc_init_f32(state.data_ptr(), C, cpo, *model, start.data_ptr() if start is not None else None,
                                           float(step_size), stream), "hmc_init")
        for t0 in range(0, total, spl):
            n = min(spl, total - t0)
            row = max(t0, num_burnin_steps) - num_burnin_steps      # the launch's first kept step (== num_results: it keeps none)
            row = min(row, num_results - 1)
            _lib.check(lib.ctpvae_hmc_run_f32(state.data_ptr(), C, int(first_chain), cpo, *model, L, n, num_burnin_steps,
                                              int(num_adaptation_steps), int(seed) & (2 ** 64 - 1), samples[row].data_ptr(),
                                              lar[row].data_ptr(), acc[row].data_ptr(), tgt[row].data_ptr(), stream), "hmc_run")
    trace = {"log_accept_ratio": lar, "is_accepted": acc > 0.5, "target_log_prob": tgt, "step_size": state[:, 2 * K - 1].clone()}
    return samples, trace


def main(argv=None):
    """bin/toy_mcmc_v2.py: example 0 of the toy dataset under --save_path, theta = [0, pi / 2], the used angles only, pnm = 1e3,
    5 leapfrog steps of 6.5e-2, 400 adaptation steps; writes posterior_prob_trace.npy [STEPS][4] (no plots)."""
    ap = argparse.ArgumentParser(description="HMC posterior of the 2 x 2 toy object")
    ap.add_argument("--save_path", required=True, help="directory with all_masks.npy and all_proj_samples.npy; the output goes there")
    ap.add_argument("-s", type=int, dest="number_of_steps", default=200000, help="number of kept steps")
    ap.add_argument("-b", type=int, dest="burnin", default=50000, help="number of burn-in steps")
    ap.add_argument("--chains", type=int, default=1, help="independent chains (the output then is [STEPS][chains][4])")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    mask = np.load(os.path.join(args.save_path, "all_masks.npy"))[0].astype(np.float32)
    meas = np.load(os.path.join(args.save_path, "all_proj_samples.npy"))[0].astype(np.float32)
    theta = np.array([0, np.pi / 2], dtype=np.float32)
    used = mask > 0
    samples, _ = hmc_sample(torch.from_numpy(meas[used]).to(dev), torch.from_numpy(mask[used]).to(dev), theta[used], 1e3,
                            num_results=args.number_of_steps, num_burnin_steps=args.burnin, num_leapfrog_steps=5, step_size=6.5e-2,
                            num_adaptation_steps=400, chains_per_object=args.chains, seed=args.seed)
    out = samples.cpu().numpy()
    np.save(os.path.join(args.save_path, "posterior_prob_trace.npy"), out[:, 0] if args.chains == 1 else out)


if __name__ == "__main__":
    main()
