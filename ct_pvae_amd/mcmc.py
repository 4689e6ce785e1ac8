"""HMC ground-truth posterior for small objects (bin/toy_mcmc_v2.py, ctvae/toy_mcmc_v2_functions.py of vganapati/CT_PVAE).

    hmc_sample(meas, mask, theta, pnm, *, prior=None, num_results, ...)   tfp.mcmc.sample_chain over SimpleStepSizeAdaptation(
                                                                          TransformedTransitionKernel(HamiltonianMonteCarlo,
                                                                          IteratedSigmoidCentered)) on joint_log_prob
    hmc_marginals(meas, mask, theta, pnm, *, bins, lo, width, ...)        the same run with the histograms, moments, acceptance and
                                                                          split R-hat of all chains accumulated inside the launches
                                                                          (csrc/hmc_marginals.hip); keeps no sample unless asked to
    hmc_marginals(..., max_lag=L, cov=True)                               + the raw sums of the chains' autocovariance and of the
                                                                          covariance between pixels (csrc/hmc_diagnostics.hip):
                                                                          HmcMarginals.autocov / autocorr / ess / cov / corr
    python -m ct_pvae_amd.mcmc --save_path D -s STEPS -b BURNIN            bin/toy_mcmc_v2.py without its plots
                               [--marginals [--no_trace] [--compare F]     + hmc_marginals.npz; against a trainer's pixel_dist_K.npz
                                [--ess_lags L] [--cov]]                    + effective sample size per pixel, covariance

One 64-lane wave runs a whole chain inside one persistent kernel (csrc/hmc.hip states the density, the transition, the orders of
the sums and the layout of the random numbers); this module validates, uploads the tables and loops over launches.  With
hmc_sample(form="workgroup") a workgroup of up to 16 waves runs the chain, one pixel per thread, for objects of up to 32 x 32 pixels
(csrc/hmc_wg.hip).  There is no CPU path.
"""
import argparse
import ctypes
import math
import os
import types

import numpy as np
import torch

from . import _lib, forward_functions
from .forward_functions import _stream_ptr, rotate_tables
from .helper_functions import toy_dist
from .marginals import _grid_args, hist_distance

__all__ = ["hmc_sample", "hmc_marginals", "HmcMarginals", "split_rhat", "autocov_from_sums", "toy_dist", "MAX_STEPS_PER_LAUNCH", "MAX_STEPS_PER_LAUNCH_WG",
           "MAX_LAG"]

# CTPVAE_HMC_MAX_STEPS of include/ctpvae_radon.h: the largest power of two that keeps one launch of the slowest shape measured with 5
# leapfrog steps (8 x 8, 180 angles, 149 us per transition on the MI355X) under 100 ms (tools/time_hmc.py -> profiles/hmc_timing.txt).
# The default steps_per_launch is this for up to 5 leapfrog steps and shrinks in proportion above, so that a default launch stays
# near that time (the entry point's worst case, 32 leapfrog steps at 256 angles, costs 1.26 ms per transition).
# hmc_marginals shares the cap: the longest launch of its kernel at that shape, with 254 bins, takes 78.9 ms (154 us per transition;
# tools/time_hmc_marginals.py -> profiles/hmc_marginals_timing.txt).  So does its max_lag / cov path: 80.05 ms with 64 lags and cov
# (tools/time_hmc_diagnostics.py -> profiles/hmc_diagnostics_timing.txt).
MAX_STEPS_PER_LAUNCH = 512
# CTPVAE_HMC_MAX_LAG, and the LDS one workgroup can have on gfx950 (csrc/hmc_diagnostics.hip): what hmc_marginals(max_lag=, cov=) may ask
MAX_LAG = 64
LDS_BYTES_PER_WORKGROUP = 160 * 1024
_MAX_ANGLES, _MAX_COMPONENTS, _MAX_LEAPFROGS = 256, 4, 32
# The cap of hmc_sample(form="workgroup") (csrc/hmc_wg.hip), by the same rule: the largest power of two, at most 512, that keeps one
# launch of a full residency of chains of the slowest shape measured with 5 leapfrog steps under 100 ms on the MI355X.  Measured
# (tools/time_hmc_wg.py -> profiles/hmc_wg_timing.txt; it starts at 8 transitions per launch and doubles only while the projection
# stays under 100 ms), per transition inside a launch, 1 chain / one full residency of chains: 9 x 9 at 20 angles 23.9 / 33.6 us
# (2,560 chains), 16 x 16 at 20 angles 30.5 / 38.7 us (1,280), 16 x 16 at 90 angles 82.3 / 82.4 us (256), 32 x 32 at 20 angles 51.1 /
# 51.3 us (256).  The slowest, 82.4 us, makes a launch of 512 transitions 42.2 ms: the cap is 512, and the default shrinks with the
# leapfrog count above 5 as the wave form's does.  (Shapes beyond the table are not measured: a transition's time grows with the
# angle count, so a run with many more angles than these should pass a smaller steps_per_launch.)
MAX_STEPS_PER_LAUNCH_WG = 512
_MAX_N_WG = 32


def _lgamma64(a):
    return np.vectorize(math.lgamma, otypes=[np.float64])(a)


def _prior_tables(prior, K, who="hmc_sample"):
    """(logw [M], alpha [M][K], lbeta [M]) as float32: the concentrations rounded to float32 once, the rest from them in float64."""
    weights, alpha = toy_dist() if prior is None else prior
    weights = np.asarray(weights, np.float64).reshape(-1)
    alpha = np.asarray(alpha, np.float64)
    alpha = alpha[None] if alpha.ndim == 1 else alpha
    M = weights.size
    if not 1 <= M <= _MAX_COMPONENTS:
        raise ValueError(f"{who}: the prior is a mixture of 1 .. {_MAX_COMPONENTS} Dirichlets (got {M} weights)")
    if alpha.shape != (M, K):
        raise ValueError(f"{who}: concentrations must be [{M}][{K}] for {M} components and {K} pixels (got {alpha.shape})")
    alpha = alpha.astype(np.float32).astype(np.float64)
    if not (np.all(np.isfinite(alpha)) and np.all(alpha > 0)):
        raise ValueError(f"{who}: concentrations must be positive and finite")
    if not (np.all(np.isfinite(weights)) and np.all(weights > 0)):
        raise ValueError(f"{who}: mixture weights must be positive and finite")
    lbeta = _lgamma64(alpha).sum(-1) - _lgamma64(alpha.sum(-1))
    return np.log(weights).astype(np.float32), alpha.astype(np.float32), lbeta.astype(np.float32)


def _wg_pieces(C, cpo, cap):
    """The workgroup form's launches over C chains, at most cap chains each: (first chain, chains, chains per object of the launch,
    its first object).  A launch holds whole objects, or chains of one object alone (then all its chains share that object)."""
    c = 0
    while c < C:
        obj, within = divmod(c, cpo)
        if within == 0 and cap >= cpo:
            n, per = min(cap, C - c) // cpo * cpo, cpo
        else:
            n = per = min(cap, cpo - within)
        yield c, n, per, obj
        c += n


def _start_run(who, meas, mask, theta, pnm, *, prior, num_results, num_burnin_steps, num_leapfrog_steps, step_size,
               num_adaptation_steps, chains_per_object, initial_state, seed, first_chain, steps_per_launch, grid=None,
               diag=None, form="wave", chains_per_launch=None):
    """What hmc_sample and hmc_marginals share: every check on the values (grid = (bins, lo, width): the histogram's, checked last),
    then the device check, the uploads and the init launch.  Returns the run: sizes, the state and the model arguments of the run
    entry points (with the tensors they point into)."""
    lib = _lib.load()
    if form not in ("wave", "workgroup"):
        raise ValueError(f"{who}: form must be 'wave' or 'workgroup' (got {form!r})")
    wg = form == "workgroup"
    if not (isinstance(meas, torch.Tensor) and isinstance(mask, torch.Tensor)):
        raise TypeError(f"{who}: meas and mask must be torch tensors")
    if meas.dim() == 2:
        meas, mask = meas[None], (mask[None] if mask.dim() == 1 else mask)
    if meas.dim() != 3 or mask.dim() != 2:
        raise ValueError(f"{who}: meas must be [A][N] or [B][A][N] and mask [A] or [B][A] (got {tuple(meas.shape)}, {tuple(mask.shape)})")
    B, A, N = meas.shape
    K = N * N
    th = np.asarray(theta.detach().cpu() if isinstance(theta, torch.Tensor) else theta, dtype=np.float32).reshape(-1)
    if K > 64 and not wg:
        raise ValueError(f"{who}: objects of at most 64 pixels, one per lane (got N={N}: {K} pixels)"
                         + ("; form='workgroup' takes up to 32 x 32" if who == "hmc_sample" else ""))
    if N > _MAX_N_WG:
        raise ValueError(f"{who}: form='workgroup' takes objects of at most {_MAX_N_WG} x {_MAX_N_WG} pixels, one per thread (got N={N})")
    if N < 2:
        raise ValueError(f"{who}: the object needs at least 2 x 2 pixels")
    if th.size != A or tuple(mask.shape) != (B, A):
        raise ValueError(f"{who}: the object is square with one detector bin per pixel column: meas [B][A][N], mask [B][A], theta [A] "
                         f"(got meas {tuple(meas.shape)}, mask {tuple(mask.shape)}, {th.size} angles)")
    if A > _MAX_ANGLES:
        raise ValueError(f"{who}: at most {_MAX_ANGLES} angles (got {A})")
    logw, alpha, lbeta = _prior_tables(prior, K, who)
    num_results, num_burnin_steps, L = int(num_results), int(num_burnin_steps), int(num_leapfrog_steps)
    cpo = int(chains_per_object)
    if num_results < 1 or num_burnin_steps < 0 or cpo < 1 or int(num_adaptation_steps) < 0 or int(first_chain) < 0:
        raise ValueError(f"{who}: num_results and chains_per_object must be >= 1; burn-in, adaptation steps and first_chain >= 0")
    if not 1 <= L <= _MAX_LEAPFROGS:
        raise ValueError(f"{who}: 1 .. {_MAX_LEAPFROGS} leapfrog steps (got {L})")
    if not float(step_size) > 0 or not float(pnm) > 0:
        raise ValueError(f"{who}: step_size and pnm must be positive")
    spl_cap = MAX_STEPS_PER_LAUNCH_WG if wg else MAX_STEPS_PER_LAUNCH
    spl = max(1, spl_cap * 5 // max(L, 5)) if steps_per_launch is None else int(steps_per_launch)
    if not 1 <= spl <= spl_cap:
        raise ValueError(f"{who}: steps_per_launch must be 1 .. {spl_cap} (got {spl})")
    if chains_per_launch is not None and (not wg or int(chains_per_launch) < 1):
        raise ValueError(f"{who}: chains_per_launch is a positive number of chains, for form='workgroup' alone (got {chains_per_launch!r})")
    if wg:
        # the tap tables of a launch sit in LDS: refused here, before anything touches the device
        need = lib.ctpvae_hmc_wg_lds_bytes(N, A)
        if need > LDS_BYTES_PER_WORKGROUP:
            raise ValueError(f"{who}: {N} x {N} pixels at {A} angles need {need} bytes of LDS per chain, a workgroup has "
                             f"{LDS_BYTES_PER_WORKGROUP}: fewer angles")
    total = num_burnin_steps + num_results
    if total >= 2 ** 32:
        raise ValueError(f"{who}: the step index is 32 bits wide")
    C = B * cpo
    if int(first_chain) + C > 2 ** 32:
        raise ValueError(f"{who}: the chain id is 32 bits wide (got first_chain={int(first_chain)} and {C} chains)")
    start_h = None
    if initial_state is not None:
        # checked on the host: the kernel takes logf of every entry, and a chain started at -inf or NaN would reject for ever, silently
        start_h = (initial_state.detach().cpu() if isinstance(initial_state, torch.Tensor) else torch.as_tensor(np.asarray(initial_state)))
        start_h = start_h.to(torch.float32).contiguous()
        if tuple(start_h.shape) != (C, K):
            raise ValueError(f"{who}: initial_state must be [{C}][{K}] (got {tuple(start_h.shape)})")
        if not bool((torch.isfinite(start_h) & (start_h > 0)).all()):
            raise ValueError(f"{who}: initial_state must be positive and finite in every entry (points inside the simplex)")
    if grid is not None:
        grid = _grid_args(*grid)
    if diag is not None:
        # hmc_marginals' max_lag and cov: the range, then the LDS of one workgroup, both before anything touches the device
        max_lag, cov = diag
        if isinstance(max_lag, bool) or int(max_lag) != max_lag or not 0 <= int(max_lag) <= MAX_LAG:
            raise ValueError(f"{who}: max_lag must be an integer 0 .. {MAX_LAG} (got {max_lag!r})")
        diag = (int(max_lag), bool(cov))
        need = lib.ctpvae_hmc_diagnostics_lds_bytes(N, A, grid[0], *diag)
        if need > LDS_BYTES_PER_WORKGROUP:
            raise ValueError(f"{who}: {N} x {N} pixels, {A} angles, bins={grid[0]}, max_lag={diag[0]}, cov={diag[1]} need {need} bytes of "
                             f"LDS per chain, a workgroup has {LDS_BYTES_PER_WORKGROUP}: lower bins or max_lag, or turn cov off")
    if meas.device.type != "cuda" or mask.device != meas.device:
        raise _lib.RadonLibraryError(f"{who}: meas and mask must be CUDA tensors on one device; there is no CPU path")
    dev = meas.device
    meas_d = meas.detach().to(torch.float32).contiguous()
    mask_d = mask.detach().to(torch.float32).contiguous()
    start = start_h.to(dev) if start_h is not None else None
    T8, Tinv8 = rotate_tables(th, N, N, dev)
    prior_d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (logw, alpha, lbeta)]
    state = forward_functions._new_output((C, 2 * K + 1), torch.float32, dev)
    model = (N, T8.data_ptr(), Tinv8.data_ptr(), A, mask_d.data_ptr(), meas_d.data_ptr(), float(pnm), logw.size, prior_d[0].data_ptr(),
             prior_d[1].data_ptr(), prior_d[2].data_ptr())
    pieces = None
    with torch.cuda.device(dev):
        if wg:
            # at most as many workgroups in a launch as the device keeps resident at once
            cap = ctypes.c_int(0)
            _lib.check(lib.ctpvae_hmc_wg_resident_chains(N, A, ctypes.byref(cap)), "hmc_wg_resident_chains")
            cap = cap.value if chains_per_launch is None else min(cap.value, int(chains_per_launch))
            pieces = list(_wg_pieces(C, cpo, cap))
            for c0, n, per, obj in pieces:
                m = list(model)
                m[4], m[5] = mask_d[obj].data_ptr(), meas_d[obj].data_ptr()
                _lib.check(lib.ctpvae_hmc_wg_init_f32(state[c0].data_ptr(), n, per, *m, start[c0].data_ptr() if start is not None else None,
                                                      float(step_size), _stream_ptr()), "hmc_wg_init")
        else:
            _lib.check(lib.ctpvae_hmc_init_f32(state.data_ptr(), C, cpo, *model, start.data_ptr() if start is not None else None,
                                               float(step_size), _stream_ptr()), "hmc_init")
    return types.SimpleNamespace(lib=lib, dev=dev, B=B, N=N, K=K, C=C, cpo=cpo, L=L, spl=spl, total=total, num_results=num_results,
                                 pieces=pieces, mask_d=mask_d, meas_d=meas_d,
                                 num_burnin_steps=num_burnin_steps, state=state, model=model, grid=grid, diag=diag,
                                 run_args=(L, num_burnin_steps, int(num_adaptation_steps), int(seed) & (2 ** 64 - 1)),
                                 first_chain=int(first_chain), keep=(meas_d, mask_d, start, T8, Tinv8, prior_d))


def _launches(r):
    """(steps, first kept row) of the run's launches in order.  A launch that keeps no step gets a valid row all the same."""
    for t0 in range(0, r.total, r.spl):
        row = max(t0, r.num_burnin_steps) - r.num_burnin_steps      # the launch's first kept step (== num_results: it keeps none)
        yield min(r.spl, r.total - t0), min(row, r.num_results - 1)


def _per_step_outputs(r):
    samples = forward_functions._new_output((r.num_results, r.C, r.K), torch.float32, r.dev)
    lar, acc, tgt = (forward_functions._new_output((r.num_results, r.C), torch.float32, r.dev) for _ in range(3))
    return samples, lar, acc, tgt


def _trace(r, lar, acc, tgt):
    return {"log_accept_ratio": lar, "is_accepted": acc > 0.5, "target_log_prob": tgt, "step_size": r.state[:, 2 * r.K - 1].clone()}


def hmc_sample(meas, mask, theta, pnm, *, prior=None, num_results, num_burnin_steps=0, num_leapfrog_steps=5, step_size=6.5e-2,
               num_adaptation_steps=400, chains_per_object=1, initial_state=None, seed=0, first_chain=0, steps_per_launch=None,
               form="wave", chains_per_launch=None):
    """Posterior samples of N x N objects (N * N <= 64; up to 32 x 32 with form="workgroup") on the simplex given sparse noisy
    sinograms, by HMC on the GPU.

    meas [A][N] or [B][A][N] and mask [A] or [B][A]: CUDA float tensors (create_all_masks' outputs); theta [A] radians; pnm: the
    Poisson noise multiplier.  prior: (weights [M], concentrations [M][K]) of a mixture of M <= 4 Dirichlets, default toy_dist().
    C = B * chains_per_object chains run side by side, chain c on object c // chains_per_object; its random numbers depend on
    (seed, first_chain + c, step index) alone, so a run does not change with steps_per_launch or with how chains are spread over
    calls.  initial_state [C][K]: starting points inside the simplex, every entry positive and finite (default: the bijector's
    image of 0).  The step size adapts during the first num_adaptation_steps steps (burn-in included), per chain.  steps_per_launch
    (1 .. MAX_STEPS_PER_LAUNCH) defaults to that cap, divided by num_leapfrog_steps / 5 above 5 leapfrog steps.

    form="wave" (the default): one 64-lane wave per chain, csrc/hmc.hip.  form="workgroup": one workgroup of ceil(K / 64) waves per
    chain, one pixel per thread, 2 <= N <= 32 (csrc/hmc_wg.hip): the same target, transition, random numbers and outputs, and for
    N <= 8 the same bits.  Its tap tables sit in LDS, so an (N, A) above LDS_BYTES_PER_WORKGROUP (32 x 32 beyond 46 angles) raises
    ValueError before any launch; steps_per_launch is 1 .. MAX_STEPS_PER_LAUNCH_WG there.  A launch of that form holds at most as
    many chains as the device keeps resident at once (multiprocessors x the occupancy query); further launches take the rest, which
    changes no bit.  chains_per_launch (developers) lowers that number.

    Returns (samples [num_results][C][K], trace) with trace = {"log_accept_ratio", "is_accepted", "target_log_prob":
    [num_results][C], "step_size": [C] after the last step}."""
    r = _start_run("hmc_sample", meas, mask, theta, pnm, prior=prior, num_results=num_results, num_burnin_steps=num_burnin_steps,
                   num_leapfrog_steps=num_leapfrog_steps, step_size=step_size, num_adaptation_steps=num_adaptation_steps,
                   chains_per_object=chains_per_object, initial_state=initial_state, seed=seed, first_chain=first_chain,
                   steps_per_launch=steps_per_launch, form=form, chains_per_launch=chains_per_launch)
    samples, lar, acc, tgt = out = _per_step_outputs(r)
    L, keep_from, n_adapt, seed64 = r.run_args
    with torch.cuda.device(r.dev):
        stream = _stream_ptr()
        for i, (n, row) in enumerate(_launches(r)):
            if r.pieces is None:
                _lib.check(r.lib.ctpvae_hmc_run_f32(r.state.data_ptr(), r.C, r.first_chain, r.cpo, *r.model, L, n, keep_from, n_adapt,
                                                    seed64, samples[row].data_ptr(), lar[row].data_ptr(), acc[row].data_ptr(),
                                                    tgt[row].data_ptr(), stream), "hmc_run")
                continue
            kept = max(0, i * r.spl + n - max(i * r.spl, r.num_burnin_steps))      # the rows this launch stores
            for c0, nc, per, obj in r.pieces:
                # the entry point stores rows of ITS chains: straight into the outputs when the launch holds all of them
                dst = [a[row:] for a in out] if nc == r.C else [
                    forward_functions._new_output((max(kept, 1), nc) + a.shape[2:], torch.float32, r.dev) for a in out]
                m = list(r.model)
                m[4], m[5] = r.mask_d[obj].data_ptr(), r.meas_d[obj].data_ptr()
                _lib.check(r.lib.ctpvae_hmc_wg_run_f32(r.state[c0].data_ptr(), nc, r.first_chain + c0, per, *m, L, n, keep_from, n_adapt,
                                                       seed64, *(a.data_ptr() for a in dst), stream), "hmc_wg_run")
                if nc != r.C and kept:
                    for a, d in zip(out, dst):
                        a[row:row + kept, c0:c0 + nc] = d[:kept]
    return samples, _trace(r, lar, acc, tgt)


def split_rhat(s1, s2, n, chains_per_object):
    """Split R-hat from the sums alone.  s1, s2: float64 [2][C][K], the sum and the sum of squares of the n samples of (half, chain,
    pixel); an object's m = 2 * chains_per_object sequences are its chains' halves.  With mu_j = s1_j / n and v_j = (s2_j - s1_j^2 / n)
    / (n - 1): W = mean_j v_j, Bn = var_j(mu_j) (ddof = 1), rhat = sqrt(((n - 1) / n * W + Bn) / W), float64 [B][K].  W = 0 gives inf
    or NaN, as numpy evaluates it."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    n, cpo = int(n), int(chains_per_object)
    if s1.ndim != 3 or s1.shape[0] != 2 or s2.shape != s1.shape or cpo < 1 or s1.shape[1] % cpo != 0:
        raise ValueError(f"split_rhat: s1 and s2 must be [2][C][K] with C a multiple of chains_per_object (got {s1.shape}, {s2.shape}, {cpo})")
    if n < 2:
        raise ValueError(f"split_rhat: every half needs at least 2 samples (got n={n})")
    K = s1.shape[2]
    seq = lambda a: a.reshape(2, -1, cpo, K).transpose(1, 0, 2, 3).reshape(-1, 2 * cpo, K)   # noqa: E731  [B][m][K]
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = seq(s1 / n)
        v = seq((s2 - s1 * s1 / n) / (n - 1))
        W = v.mean(axis=1)
        Bn = mu.var(axis=1, ddof=1)
        return np.sqrt(((n - 1) / n * W + Bn) / W)


def autocov_from_sums(lag, head, ring, S, n):
    """The centred biased autocovariance from the raw sums alone, float64 [C][Lm + 1][K].  lag [C][Lm + 1][K]: r_l = sum over j = l ..
    n - 1 of x_j x_(j-l); head [C][Lm][K]: x_0 .. x_(Lm-1) (rows >= n unwritten); ring [C][Lm + 1][K]: x_j in slot j mod (Lm + 1) for
    the last Lm + 1 steps; S [C][K]: the sum of all n values.  With m = S / n, H_l = S - (x_0 + .. + x_(l-1)) and T_l = S - (x_(n-1) +
    .. + x_(n-l)):  c_l = (r_l - m (H_l + T_l) + (n - l) m^2) / n = sum_j (x_j - m)(x_(j-l) - m) / n exactly; c_l = 0 for l >= n."""
    lag, S, n = np.asarray(lag, np.float64), np.asarray(S, np.float64), int(n)
    head, ring = np.asarray(head, np.float64), np.asarray(ring, np.float64)
    C, slots, K = lag.shape
    m = S / n
    out = np.zeros_like(lag)
    first, last = np.zeros((C, K)), np.zeros((C, K))       # x_0 + .. + x_(l-1) and x_(n-1) + .. + x_(n-l)
    for l in range(min(slots, n)):
        if l:
            first = first + head[:, l - 1]
            last = last + ring[:, (n - l) % slots]
        out[:, l] = (lag[:, l] - m * ((S - first) + (S - last)) + (n - l) * (m * m)) / n
    return out


def _geyer_ess(rho, n, M):
    """Geyer's initial positive sequence over axis -2 of rho [..][Lm + 1][K] -> (ESS [..][K], truncated [..][K]); lags >= n count as 0."""
    slots = rho.shape[-2]
    rho = np.where((np.arange(slots) < n)[:, None], rho, 0.0)
    pairs = slots // 2
    P = rho[..., 0:2 * pairs:2, :] + rho[..., 1:2 * pairs:2, :]
    keep = np.cumprod(P > 0, axis=-2).astype(bool)             # (a NaN pair is not positive)
    total = np.where(keep, P, 0.0).sum(axis=-2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(keep[..., 0, :], M * n / (-1.0 + 2.0 * total), np.nan)
    return ess, keep[..., -1, :]


class HmcMarginals:
    """What hmc_marginals returns: the per-pixel marginals of C = B * chains_per_object chains on B objects of shape (N, N).
    On the device: hist int64 [B][K][bins + 2] (the rows of PixelMarginals.hist: below lo | the bins | at or above lo + bins * width,
    pooled over an object's chains), s1 and s2 float64 [2][C][K] (sum and sum of squares of the samples of each half of the kept steps,
    per chain), accepted int64 [C], step_size float32 [C] after the last step.  count = num_results * chains_per_object samples per
    pixel and object.  samples and trace are hmc_sample's, or None.

    With hmc_marginals(max_lag=Lm >= 1): lag float64 [C][Lm + 1][K] (sum over the kept steps j >= l of x_j * x_(j-l), per chain and
    pixel), ring float32 [C][Lm + 1][K] (the chain's last Lm + 1 kept values, step j in slot j mod (Lm + 1)) and head float32
    [C][Lm][K] (its first Lm kept values); with cov=True: xx float64 [C][K][K] (sum over the kept steps of O_k * O_i).  None otherwise.
    autocov(), autocorr(), ess(), ess_truncated(), cov() and corr() finish them on the host in float64."""

    def __init__(self, shape, bins, lo, width, num_results, chains_per_object, hist, s1, s2, accepted, step_size, samples=None, trace=None,
                 lag=None, ring=None, head=None, xx=None):
        self.shape = tuple(int(v) for v in shape)
        self.bins, self.lo, self.width = _grid_args(bins, lo, width)
        self.num_results, self.chains_per_object = int(num_results), int(chains_per_object)
        self.count = self.num_results * self.chains_per_object
        K, C = self.shape[0] * self.shape[1], accepted.shape[0]
        if (self.shape[0] != self.shape[1] or self.num_results < 1 or self.chains_per_object < 1 or C % self.chains_per_object != 0
                or tuple(hist.shape) != (C // self.chains_per_object, K, self.bins + 2) or tuple(s1.shape) != (2, C, K)
                or tuple(s2.shape) != (2, C, K) or tuple(step_size.shape) != (C,)):
            raise ValueError(f"HmcMarginals: hist [B][K][bins + 2], s1 and s2 [2][C][K], accepted and step_size [C] do not fit shape "
                             f"{self.shape}, {self.bins} bins and {self.chains_per_object} chains per object")
        self.hist, self.s1, self.s2, self.accepted, self.step_size = hist, s1, s2, accepted, step_size
        self.samples, self.trace = samples, trace
        self.device = hist.device
        self.max_lag = 0
        if lag is not None or ring is not None or head is not None:
            if lag is None or ring is None or head is None or lag.dim() != 3 or not 1 <= lag.shape[1] - 1 <= MAX_LAG:
                raise ValueError("HmcMarginals: lag, ring and head come together, with 1 .. 64 lags")
            self.max_lag = int(lag.shape[1]) - 1
            if (tuple(lag.shape) != (C, self.max_lag + 1, K) or tuple(ring.shape) != (C, self.max_lag + 1, K)
                    or tuple(head.shape) != (C, self.max_lag, K)):
                raise ValueError(f"HmcMarginals: lag and ring [C][max_lag + 1][K] and head [C][max_lag][K] do not fit {C} chains, {K} pixels "
                                 f"and {self.max_lag} lags")
        if xx is not None and tuple(xx.shape) != (C, K, K):
            raise ValueError(f"HmcMarginals: xx must be [{C}][{K}][{K}] (got {tuple(xx.shape)})")
        self.lag, self.ring, self.head, self.xx = lag, ring, head, xx

    @property
    def edges(self):
        """float64 [bins + 1], nominal: membership is the float32 rule of the kernel, not a comparison with these."""
        return self.lo + self.width * np.arange(self.bins + 1, dtype=np.float64)

    def _chain_sums(self):
        """float64 [C][K] twice: half 0 + half 1 of s1 and of s2, on the host."""
        s1, s2 = self.s1.cpu().numpy(), self.s2.cpu().numpy()
        return s1[0] + s1[1], s2[0] + s2[1]

    def _object_sums(self):
        """float64 [B][K] twice: an object's chains added in ascending order."""
        K = self.shape[0] * self.shape[1]
        return tuple(np.cumsum(a.reshape(-1, self.chains_per_object, K), axis=1)[:, -1] for a in self._chain_sums())

    def mean(self):
        """float64 [B][N][N]: the mean of every pixel over the count samples of its object."""
        return (self._object_sums()[0] / self.count).reshape(-1, *self.shape)

    def std(self):
        """float64 [B][N][N], the sample standard deviation (count - 1), as PixelMarginals.std; NaN while count < 2."""
        t1, t2 = self._object_sums()
        if self.count < 2:
            return np.full((t1.shape[0],) + self.shape, np.nan)
        var = (t2 - t1 * t1 / self.count) / (self.count - 1)
        return np.sqrt(np.maximum(var, 0.0)).reshape(-1, *self.shape)       # (np.maximum passes a NaN on)

    def chain_mean(self):
        """float64 [C][K]: every chain's own mean."""
        return self._chain_sums()[0] / self.num_results

    def accept_rate(self):
        """float64 [C]: accepted kept steps / kept steps."""
        return self.accepted.cpu().numpy().astype(np.float64) / self.num_results

    def rhat(self):
        """float64 [B][K]: split_rhat of the chains' halves (n = num_results / 2 samples each).  Needs an even num_results >= 4."""
        if self.num_results < 4 or self.num_results % 2 != 0:
            raise ValueError(f"HmcMarginals.rhat: split R-hat needs an even num_results >= 4 (got {self.num_results})")
        return split_rhat(self.s1.cpu().numpy(), self.s2.cpu().numpy(), self.num_results // 2, self.chains_per_object)

    def _need_lags(self, what):
        if self.max_lag < 1:
            raise ValueError(f"HmcMarginals.{what}: the run kept no lagged products; call hmc_marginals with max_lag >= 1")

    def autocov(self):
        """float64 [C][max_lag + 1][K]: autocov_from_sums of every chain and pixel, the centred biased autocovariance of the chain's
        num_results kept steps at lags 0 .. max_lag."""
        self._need_lags("autocov")
        return autocov_from_sums(self.lag.cpu().numpy(), self.head.cpu().numpy(), self.ring.cpu().numpy(), self._chain_sums()[0],
                                 self.num_results)

    def autocorr(self):
        """float64 [C][max_lag + 1][K]: autocov() / its lag 0.  A chain whose pixel never moved has lag 0 equal to 0 and gets NaN, as
        numpy evaluates it."""
        c = self.autocov()
        with np.errstate(divide="ignore", invalid="ignore"):
            return c / c[:, :1]

    def _ess(self, cross_chain):
        """(ess, truncated) of ess() and ess_truncated()."""
        self._need_lags("ess")
        c, n, M = self.autocov(), self.num_results, self.chains_per_object
        K = c.shape[2]
        with np.errstate(divide="ignore", invalid="ignore"):
            if not cross_chain:
                return _geyer_ess(c / c[:, :1], n, 1)
            # W and var+ over whole chains: the within-chain variance (n - 1) and the variance of the chains' means
            c = c.reshape(-1, M, self.max_lag + 1, K)
            W = c[:, :, 0].mean(axis=1) * (n / (n - 1.0)) if n > 1 else np.full((c.shape[0], K), np.nan)
            mu = self.chain_mean().reshape(-1, M, K)
            Bn = mu.var(axis=1, ddof=1) if M > 1 else np.zeros_like(W)
            var_plus = (n - 1.0) / n * W + Bn
            rho = 1.0 - (W[:, None] - c.mean(axis=1)) / var_plus[:, None]
            return _geyer_ess(rho, n, M)

    def ess(self, cross_chain=True):
        """Effective sample size by Geyer's initial positive sequence: with the pair sums P_m = rho_2m + rho_(2m+1), m = 0, 1, ..., over
        the lags the run kept, truncated at the first pair that is not positive, ESS = M * n / (-1 + 2 * sum of the pairs kept); n =
        num_results, lags >= n contribute nothing.  cross_chain=True: float64 [B][K], M = chains_per_object and rho_l = 1 - (W - mean_c
        autocov_l,c) / var+, where W = mean_c autocov_0,c * n / (n - 1) and var+ = (n - 1) / n * W + var_c(chain means, ddof = 1) are
        taken over WHOLE chains -- rhat() splits every chain in two halves, this does not, so the two do not share W or var+.  With one
        chain per object var+ = (n - 1) / n * W.  cross_chain=False: float64 [C][K], every chain on its own with M = 1 and rho =
        autocorr().  Where ess_truncated() is true the sum stopped at max_lag, not at a non-positive pair: the value is an upper
        bound.  NaN where lag 0 carries no information (a pixel that never moved)."""
        return self._ess(cross_chain)[0]

    def ess_truncated(self, cross_chain=True):
        """bool, the shape of ess(cross_chain): True where every pair sum up to max_lag was still positive, so that the sum was cut by
        the lag window and ess() there is an upper bound."""
        return self._ess(cross_chain)[1]

    def cov(self):
        """float64 [B][K][K]: the sample covariance (count - 1) between the pixels of an object over the count samples of all its
        chains, from xx and the sums; the chains are added in ascending order.  NaN while count < 2."""
        if self.xx is None:
            raise ValueError("HmcMarginals.cov: the run kept no cross products; call hmc_marginals with cov=True")
        K = self.shape[0] * self.shape[1]
        X = np.cumsum(self.xx.cpu().numpy().reshape(-1, self.chains_per_object, K, K), axis=1)[:, -1]
        t1 = self._object_sums()[0]
        if self.count < 2:
            return np.full(X.shape, np.nan)
        return (X - t1[:, :, None] * t1[:, None, :] / self.count) / (self.count - 1)

    def corr(self):
        """float64 [B][K][K]: cov() / sqrt(its diagonal, outer); NaN in the rows and columns of a pixel that never moved."""
        v = self.cov()
        d = np.sqrt(np.maximum(np.einsum("bkk->bk", v), 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            return v / (d[:, :, None] * d[:, None, :])

    def save(self, path):
        """One .npz: hist, s1, s2, accepted, step_size, edges, shape, bins, lo, width, num_results, chains_per_object, count and
        head = "hmc"; with kept samples also samples and the trace's log_accept_ratio, is_accepted and target_log_prob; with lags lag,
        ring and lag_head (the first values: "head" names the file's kind); with cross products xx."""
        extra = {}
        if self.samples is not None:
            extra = dict(samples=self.samples.cpu().numpy(), **{k: v.cpu().numpy() for k, v in self.trace.items() if k != "step_size"})
        if self.max_lag:
            extra.update(lag=self.lag.cpu().numpy(), ring=self.ring.cpu().numpy(), lag_head=self.head.cpu().numpy())
        if self.xx is not None:
            extra["xx"] = self.xx.cpu().numpy()
        np.savez(path, hist=self.hist.cpu().numpy(), s1=self.s1.cpu().numpy(), s2=self.s2.cpu().numpy(),
                 accepted=self.accepted.cpu().numpy(), step_size=self.step_size.cpu().numpy(), edges=self.edges,
                 shape=np.asarray(self.shape, np.int64), bins=np.int64(self.bins), lo=np.float64(self.lo), width=np.float64(self.width),
                 num_results=np.int64(self.num_results), chains_per_object=np.int64(self.chains_per_object), count=np.int64(self.count),
                 head=np.str_("hmc"), **extra)

    @classmethod
    def load(cls, path, device="cuda"):
        """The state save() wrote, on `device`."""
        dev = torch.device(device)
        with np.load(path) as f:
            if "head" not in f.files or str(f["head"]) != "hmc":
                raise ValueError(f"{path}: not a file of HmcMarginals.save (head must be 'hmc')")
            t = {k: torch.from_numpy(f[k]).to(dev) for k in f.files if k not in ("head", "edges") and f[k].ndim > 0}
            samples, trace = None, None
            if "samples" in t:
                samples = t["samples"]
                trace = {k: t[k] for k in ("log_accept_ratio", "is_accepted", "target_log_prob")}
                trace["step_size"] = t["step_size"].clone()
            m = cls(tuple(int(v) for v in f["shape"]), int(f["bins"]), float(f["lo"]), float(f["width"]), int(f["num_results"]),
                    int(f["chains_per_object"]), t["hist"], t["s1"], t["s2"], t["accepted"], t["step_size"], samples, trace, t.get("lag"),
                    t.get("ring"), t.get("lag_head"), t.get("xx"))
            if int(f["count"]) != m.count:
                raise ValueError(f"{path}: count {int(f['count'])} is not num_results * chains_per_object = {m.count}")
        return m


def hmc_marginals(meas, mask, theta, pnm, *, bins=50, lo=0.005, width=0.01, keep_samples=False, prior=None, num_results,
                  num_burnin_steps=0, num_leapfrog_steps=5, step_size=6.5e-2, num_adaptation_steps=400, chains_per_object=1,
                  initial_state=None, seed=0, first_chain=0, steps_per_launch=None, max_lag=0, cov=False):
    """hmc_sample's run (every argument of it with its meaning and default; the same chains bit for bit) with the per-pixel marginals
    of ALL chains accumulated inside the sampler's launches (csrc/hmc_marginals.hip): per object a histogram on PixelMarginals' grid
    (bins, lo, width: the reference's np.arange(0.005, 0.51, 0.01) by default), per chain the float64 sum and sum of squares of each
    half of the kept steps, and the accepted steps.  Returns an HmcMarginals: mean(), std(), chain_mean(), accept_rate(), rhat().
    keep_samples=False stores nothing per step: samples and trace are None, and no allocation of the call grows with num_results.
    keep_samples=True returns hmc_sample's samples and trace beside the statistics.  A NaN sample counts in column 0 and makes its
    chain's sums NaN.

    max_lag=Lm (1 .. MAX_LAG) and cov=True add, in the same launches (csrc/hmc_diagnostics.hip), per chain the float64 sums of the
    products of every kept value with the chain's Lm values before it, and of every pair of pixels of a kept step: what
    HmcMarginals.autocov(), autocorr(), ess(), ess_truncated() and cov(), corr() are finished from.  They cost (Lm + 1) * K * 12 + Lm * K * 4
    and K * K * 8 bytes per chain, whatever num_results, and everything else of the result keeps its bits.  The sums sit in LDS during
    a launch: a request above LDS_BYTES_PER_WORKGROUP (8 x 8 pixels with many angles, bins, lags and cov at once) raises ValueError
    before any launch.  With the defaults (0, False) the call is the one it was.

    This call runs the wave form only (N * N <= 64): hmc_sample's form="workgroup" has no marginals or diagnostics yet."""
    r = _start_run("hmc_marginals", meas, mask, theta, pnm, prior=prior, num_results=num_results, num_burnin_steps=num_burnin_steps,
                   num_leapfrog_steps=num_leapfrog_steps, step_size=step_size, num_adaptation_steps=num_adaptation_steps,
                   chains_per_object=chains_per_object, initial_state=initial_state, seed=seed, first_chain=first_chain,
                   steps_per_launch=steps_per_launch, grid=(bins, lo, width), diag=(max_lag, cov))
    bins, lo, width = r.grid
    Lm, cov = r.diag
    hist = torch.zeros((r.B, r.K, bins + 2), dtype=torch.int64, device=r.dev)
    mom = torch.zeros((2, 2, r.C, r.K), dtype=torch.float64, device=r.dev)           # [half][moment][chain][pixel]
    accepted = torch.zeros(r.C, dtype=torch.int64, device=r.dev)
    lag = ring = head = xx = None
    if Lm:
        lag = torch.zeros((r.C, Lm + 1, r.K), dtype=torch.float64, device=r.dev)
        ring = torch.zeros((r.C, Lm + 1, r.K), dtype=torch.float32, device=r.dev)
        head = torch.zeros((r.C, Lm, r.K), dtype=torch.float32, device=r.dev)
    if cov:
        xx = torch.zeros((r.C, r.K, r.K), dtype=torch.float64, device=r.dev)
    out = _per_step_outputs(r) if keep_samples else None
    L, keep_from, n_adapt, seed64 = r.run_args
    half_from = keep_from + r.num_results // 2
    with torch.cuda.device(r.dev):
        stream = _stream_ptr()
        for n, row in _launches(r):
            ptrs = [a[row].data_ptr() for a in out] if keep_samples else [None] * 4
            args = (r.state.data_ptr(), r.C, r.first_chain, r.cpo, *r.model, L, n, keep_from, n_adapt, seed64, *ptrs, half_from, lo, width,
                    bins, hist.data_ptr(), mom.data_ptr(), accepted.data_ptr())
            if Lm or cov:
                more = [a.data_ptr() if a is not None else None for a in (lag, ring, head, xx)]
                _lib.check(r.lib.ctpvae_hmc_run_diagnostics_f32(*args, Lm, *more, stream), "hmc_run_diagnostics")
            else:
                _lib.check(r.lib.ctpvae_hmc_run_marginals_f32(*args, stream), "hmc_run_marginals")
    samples, trace = (out[0], _trace(r, *out[1:])) if keep_samples else (None, None)
    return HmcMarginals((r.N, r.N), bins, lo, width, r.num_results, r.cpo, hist, mom[:, 0], mom[:, 1], accepted,
                        r.state[:, 2 * r.K - 1].clone(), samples, trace, lag, ring, head, xx)


def _load_pvae_hist(ap, path, m):
    """hist [K][bins + 2] of a PixelMarginals.save file on m's grid, or the parser's error."""
    with np.load(path) as f:
        hist, lo, width = f["hist"], float(f["lo"]), float(f["width"])
    K = m["N"] * m["N"]
    if hist.ndim != 2 or hist.shape[1] - 2 != m["bins"] or lo != m["lo"] or width != m["width"]:
        ap.error(f"--compare: {path} is binned on another grid (bins={hist.shape[-1] - 2}, lo={lo}, width={width}; this run: "
                 f"bins={m['bins']}, lo={m['lo']}, width={m['width']})")
    if hist.shape[0] != K:
        ap.error(f"--compare: {path} has {hist.shape[0]} pixels, the object has {K}")
    return hist


def main(argv=None):
    """bin/toy_mcmc_v2.py: example 0 of the toy dataset under --save_path, theta = [0, pi / 2], the used angles only, pnm = 1e3,
    5 leapfrog steps of 6.5e-2, 400 adaptation steps; writes posterior_prob_trace.npy [STEPS][4] (no plots).  --marginals: the run
    goes through hmc_marginals and hmc_marginals.npz is written too (--no_trace: and no sample is kept); --compare FILE: the
    total-variation distance per pixel between FILE's histogram (a trainer's pixel_dist_K.npz) and this posterior's; --ess_lags L:
    prints the minimum and the median over the pixels of the cross-chain effective sample size (and says where it is only an upper
    bound) and writes lag, ring and lag_head into the file; --cov: writes xx, the cross products of the pixels."""
    ap = argparse.ArgumentParser(description="HMC posterior of the 2 x 2 toy object")
    ap.add_argument("--save_path", required=True, help="directory with all_masks.npy and all_proj_samples.npy; the output goes there")
    ap.add_argument("-s", type=int, dest="number_of_steps", default=200000, help="number of kept steps")
    ap.add_argument("-b", type=int, dest="burnin", default=50000, help="number of burn-in steps")
    ap.add_argument("--chains", type=int, default=1, help="independent chains (the output then is [STEPS][chains][4])")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--marginals", action="store_true", help="accumulate histograms, moments and split R-hat of all chains on the device; "
                    "writes hmc_marginals.npz")
    ap.add_argument("--bins", type=int, default=50, help="with --marginals: number of bins")
    ap.add_argument("--lo", type=float, default=0.005, help="with --marginals: lower edge of the first bin")
    ap.add_argument("--width", type=float, default=0.01, help="with --marginals: width of a bin")
    ap.add_argument("--no_trace", action="store_true", help="with --marginals: keep no samples, write no posterior_prob_trace.npy")
    ap.add_argument("--compare", metavar="FILE", help="with --marginals: a pixel_dist_K.npz of the trainer on the same grid; prints the "
                    "total-variation distance per pixel and writes hmc_vs_pvae.npy")
    ap.add_argument("--ess_lags", type=int, default=0, metavar="L", help="with --marginals: accumulate the autocovariance up to lag L "
                    f"(1 .. {MAX_LAG}) and print the effective sample size per pixel")
    ap.add_argument("--cov", action="store_true", help="with --marginals: accumulate the covariance between the pixels")
    args = ap.parse_args(argv)
    if (args.no_trace or args.compare or args.ess_lags or args.cov) and not args.marginals:
        ap.error("--no_trace, --compare, --ess_lags and --cov need --marginals")
    if not 0 <= args.ess_lags <= MAX_LAG:
        ap.error(f"--ess_lags must be 0 .. {MAX_LAG}")
    mask = np.load(os.path.join(args.save_path, "all_masks.npy"))[0].astype(np.float32)
    meas = np.load(os.path.join(args.save_path, "all_proj_samples.npy"))[0].astype(np.float32)
    if args.marginals:
        bins, lo, width = _grid_args(args.bins, args.lo, args.width)
        pvae = _load_pvae_hist(ap, args.compare, dict(N=meas.shape[-1], bins=bins, lo=lo, width=width)) if args.compare else None
    dev = torch.device("cuda", 0)
    theta = np.array([0, np.pi / 2], dtype=np.float32)
    used = mask > 0
    run = dict(num_results=args.number_of_steps, num_burnin_steps=args.burnin, num_leapfrog_steps=5, step_size=6.5e-2,
               num_adaptation_steps=400, chains_per_object=args.chains, seed=args.seed)
    problem = (torch.from_numpy(meas[used]).to(dev), torch.from_numpy(mask[used]).to(dev), theta[used], 1e3)
    if args.marginals:
        m = hmc_marginals(*problem, bins=bins, lo=lo, width=width, keep_samples=not args.no_trace, max_lag=args.ess_lags, cov=args.cov,
                          **run)
        m.save(os.path.join(args.save_path, "hmc_marginals.npz"))
        samples = m.samples
        rate = m.accept_rate()
        print(f"{m.count} samples per pixel; acceptance {rate.min():.3f} .. {rate.max():.3f}; mean {m.mean()[0].ravel()}")
        if m.num_results >= 4 and m.num_results % 2 == 0:
            print(f"split R-hat per pixel {m.rhat()[0]}")
        if m.max_lag:
            ess, cut = m.ess()[0], m.ess_truncated()[0]
            print(f"ESS per pixel {ess}: minimum {np.nanmin(ess):.1f}, median {np.nanmedian(ess):.1f} of {m.count} samples"
                  + (f"; still positive at lag {m.max_lag} in {int(cut.sum())} pixels: upper bounds there" if cut.any() else ""))
        if pvae is not None:
            d = hist_distance(pvae, m.hist[0].cpu().numpy())
            print(f"total-variation distance to {args.compare} per pixel {d}")
            np.save(os.path.join(args.save_path, "hmc_vs_pvae.npy"), d)
    else:
        samples, _ = hmc_sample(*problem, **run)
    if samples is not None:
        out = samples.cpu().numpy()
        np.save(os.path.join(args.save_path, "posterior_prob_trace.npy"), out[:, 0] if args.chains == 1 else out)


if __name__ == "__main__":
    main()
