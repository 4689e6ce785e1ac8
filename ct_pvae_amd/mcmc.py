"""HMC ground-truth posterior for small objects (bin/toy_mcmc_v2.py, ctvae/toy_mcmc_v2_functions.py of vganapati/CT_PVAE).

    hmc_sample(meas, mask, theta, pnm, *, prior=None, num_results, ...)   tfp.mcmc.sample_chain over SimpleStepSizeAdaptation(
                                                                          TransformedTransitionKernel(HamiltonianMonteCarlo,
                                                                          IteratedSigmoidCentered)) on joint_log_prob
    hmc_marginals(meas, mask, theta, pnm, *, bins, lo, width, ...)        the same run with the histograms, moments, acceptance and
                                                                          split R-hat of all chains accumulated inside the launches
                                                                          (csrc/hmc_marginals.hip); keeps no sample unless asked to
    python -m ct_pvae_amd.mcmc --save_path D -s STEPS -b BURNIN            bin/toy_mcmc_v2.py without its plots
                               [--marginals [--no_trace] [--compare F]]    + hmc_marginals.npz; against a trainer's pixel_dist_K.npz

One 64-lane wave runs a whole chain inside one persistent kernel (csrc/hmc.hip states the density, the transition, the orders of
the sums and the layout of the random numbers); this module validates, uploads the tables and loops over launches.  There is no
CPU path.
"""
import argparse
import math
import os
import types

import numpy as np
import torch

from . import _lib, forward_functions
from .forward_functions import _stream_ptr, rotate_tables
from .helper_functions import toy_dist
from .marginals import _grid_args, hist_distance

__all__ = ["hmc_sample", "hmc_marginals", "HmcMarginals", "split_rhat", "toy_dist", "MAX_STEPS_PER_LAUNCH"]

# CTPVAE_HMC_MAX_STEPS of include/ctpvae_radon.h: the largest power of two that keeps one launch of the slowest shape measured with 5
# leapfrog steps (8 x 8, 180 angles, 149 us per transition on the MI355X) under 100 ms (tools/time_hmc.py -> profiles/hmc_timing.txt).
# The default steps_per_launch is this for up to 5 leapfrog steps and shrinks in proportion above, so that a default launch stays
# near that time (the entry point's worst case, 32 leapfrog steps at 256 angles, costs 1.26 ms per transition).
# hmc_marginals shares the cap: the longest launch of its kernel at that shape, with 254 bins, takes 78.9 ms (154 us per transition;
# tools/time_hmc_marginals.py -> profiles/hmc_marginals_timing.txt).
MAX_STEPS_PER_LAUNCH = 512
_MAX_ANGLES, _MAX_COMPONENTS, _MAX_LEAPFROGS = 256, 4, 32


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


def _start_run(who, meas, mask, theta, pnm, *, prior, num_results, num_burnin_steps, num_leapfrog_steps, step_size,
               num_adaptation_steps, chains_per_object, initial_state, seed, first_chain, steps_per_launch, grid=None):
    """What hmc_sample and hmc_marginals share: every check on the values (grid = (bins, lo, width): the histogram's, checked last),
    then the device check, the uploads and the init launch.  Returns the run: sizes, the state and the model arguments of the run
    entry points (with the tensors they point into)."""
    lib = _lib.load()
    if not (isinstance(meas, torch.Tensor) and isinstance(mask, torch.Tensor)):
        raise TypeError(f"{who}: meas and mask must be torch tensors")
    if meas.dim() == 2:
        meas, mask = meas[None], (mask[None] if mask.dim() == 1 else mask)
    if meas.dim() != 3 or mask.dim() != 2:
        raise ValueError(f"{who}: meas must be [A][N] or [B][A][N] and mask [A] or [B][A] (got {tuple(meas.shape)}, {tuple(mask.shape)})")
    B, A, N = meas.shape
    K = N * N
    th = np.asarray(theta.detach().cpu() if isinstance(theta, torch.Tensor) else theta, dtype=np.float32).reshape(-1)
    if K > 64:
        raise ValueError(f"{who}: objects of at most 64 pixels, one per lane (got N={N}: {K} pixels)")
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
    spl = max(1, MAX_STEPS_PER_LAUNCH * 5 // max(L, 5)) if steps_per_launch is None else int(steps_per_launch)
    if not 1 <= spl <= MAX_STEPS_PER_LAUNCH:
        raise ValueError(f"{who}: steps_per_launch must be 1 .. {MAX_STEPS_PER_LAUNCH} (got {spl})")
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
    with torch.cuda.device(dev):
        _lib.check(lib.ctpvae_hmc_init_f32(state.data_ptr(), C, cpo, *model, start.data_ptr() if start is not None else None,
                                           float(step_size), _stream_ptr()), "hmc_init")
    return types.SimpleNamespace(lib=lib, dev=dev, B=B, N=N, K=K, C=C, cpo=cpo, L=L, spl=spl, total=total, num_results=num_results,
                                 num_burnin_steps=num_burnin_steps, state=state, model=model, grid=grid,
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
    r = _start_run("hmc_sample", meas, mask, theta, pnm, prior=prior, num_results=num_results, num_burnin_steps=num_burnin_steps,
                   num_leapfrog_steps=num_leapfrog_steps, step_size=step_size, num_adaptation_steps=num_adaptation_steps,
                   chains_per_object=chains_per_object, initial_state=initial_state, seed=seed, first_chain=first_chain,
                   steps_per_launch=steps_per_launch)
    samples, lar, acc, tgt = _per_step_outputs(r)
    L, keep_from, n_adapt, seed64 = r.run_args
    with torch.cuda.device(r.dev):
        stream = _stream_ptr()
        for n, row in _launches(r):
            _lib.check(r.lib.ctpvae_hmc_run_f32(r.state.data_ptr(), r.C, r.first_chain, r.cpo, *r.model, L, n, keep_from, n_adapt, seed64,
                                                samples[row].data_ptr(), lar[row].data_ptr(), acc[row].data_ptr(), tgt[row].data_ptr(),
                                                stream), "hmc_run")
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


class HmcMarginals:
    """What hmc_marginals returns: the per-pixel marginals of C = B * chains_per_object chains on B objects of shape (N, N).
    On the device: hist int64 [B][K][bins + 2] (the rows of PixelMarginals.hist: below lo | the bins | at or above lo + bins * width,
    pooled over an object's chains), s1 and s2 float64 [2][C][K] (sum and sum of squares of the samples of each half of the kept steps,
    per chain), accepted int64 [C], step_size float32 [C] after the last step.  count = num_results * chains_per_object samples per
    pixel and object.  samples and trace are hmc_sample's, or None."""

    def __init__(self, shape, bins, lo, width, num_results, chains_per_object, hist, s1, s2, accepted, step_size, samples=None, trace=None):
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

    def save(self, path):
        """One .npz: hist, s1, s2, accepted, step_size, edges, shape, bins, lo, width, num_results, chains_per_object, count and
        head = "hmc"; with kept samples also samples and the trace's log_accept_ratio, is_accepted and target_log_prob."""
        extra = {}
        if self.samples is not None:
            extra = dict(samples=self.samples.cpu().numpy(), **{k: v.cpu().numpy() for k, v in self.trace.items() if k != "step_size"})
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
                    int(f["chains_per_object"]), t["hist"], t["s1"], t["s2"], t["accepted"], t["step_size"], samples, trace)
            if int(f["count"]) != m.count:
                raise ValueError(f"{path}: count {int(f['count'])} is not num_results * chains_per_object = {m.count}")
        return m


def hmc_marginals(meas, mask, theta, pnm, *, bins=50, lo=0.005, width=0.01, keep_samples=False, prior=None, num_results,
                  num_burnin_steps=0, num_leapfrog_steps=5, step_size=6.5e-2, num_adaptation_steps=400, chains_per_object=1,
                  initial_state=None, seed=0, first_chain=0, steps_per_launch=None):
    """hmc_sample's run (every argument of it with its meaning and default; the same chains bit for bit) with the per-pixel marginals
    of ALL chains accumulated inside the sampler's launches (csrc/hmc_marginals.hip): per object a histogram on PixelMarginals' grid
    (bins, lo, width: the reference's np.arange(0.005, 0.51, 0.01) by default), per chain the float64 sum and sum of squares of each
    half of the kept steps, and the accepted steps.  Returns an HmcMarginals: mean(), std(), chain_mean(), accept_rate(), rhat().
    keep_samples=False stores nothing per step: samples and trace are None, and no allocation of the call grows with num_results.
    keep_samples=True returns hmc_sample's samples and trace beside the statistics.  A NaN sample counts in column 0 and makes its
    chain's sums NaN."""
    r = _start_run("hmc_marginals", meas, mask, theta, pnm, prior=prior, num_results=num_results, num_burnin_steps=num_burnin_steps,
                   num_leapfrog_steps=num_leapfrog_steps, step_size=step_size, num_adaptation_steps=num_adaptation_steps,
                   chains_per_object=chains_per_object, initial_state=initial_state, seed=seed, first_chain=first_chain,
                   steps_per_launch=steps_per_launch, grid=(bins, lo, width))
    bins, lo, width = r.grid
    hist = torch.zeros((r.B, r.K, bins + 2), dtype=torch.int64, device=r.dev)
    mom = torch.zeros((2, 2, r.C, r.K), dtype=torch.float64, device=r.dev)           # [half][moment][chain][pixel]
    accepted = torch.zeros(r.C, dtype=torch.int64, device=r.dev)
    out = _per_step_outputs(r) if keep_samples else None
    L, keep_from, n_adapt, seed64 = r.run_args
    half_from = keep_from + r.num_results // 2
    with torch.cuda.device(r.dev):
        stream = _stream_ptr()
        for n, row in _launches(r):
            ptrs = [a[row].data_ptr() for a in out] if keep_samples else [None] * 4
            _lib.check(r.lib.ctpvae_hmc_run_marginals_f32(r.state.data_ptr(), r.C, r.first_chain, r.cpo, *r.model, L, n, keep_from, n_adapt,
                                                          seed64, *ptrs, half_from, lo, width, bins, hist.data_ptr(), mom.data_ptr(),
                                                          accepted.data_ptr(), stream), "hmc_run_marginals")
    samples, trace = (out[0], _trace(r, *out[1:])) if keep_samples else (None, None)
    return HmcMarginals((r.N, r.N), bins, lo, width, r.num_results, r.cpo, hist, mom[:, 0], mom[:, 1], accepted,
                        r.state[:, 2 * r.K - 1].clone(), samples, trace)


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
    total-variation distance per pixel between FILE's histogram (a trainer's pixel_dist_K.npz) and this posterior's."""
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
    args = ap.parse_args(argv)
    if (args.no_trace or args.compare) and not args.marginals:
        ap.error("--no_trace and --compare need --marginals")
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
        m = hmc_marginals(*problem, bins=bins, lo=lo, width=width, keep_samples=not args.no_trace, **run)
        m.save(os.path.join(args.save_path, "hmc_marginals.npz"))
        samples = m.samples
        rate = m.accept_rate()
        print(f"{m.count} samples per pixel; acceptance {rate.min():.3f} .. {rate.max():.3f}; mean {m.mean()[0].ravel()}")
        if m.num_results >= 4 and m.num_results % 2 == 0:
            print(f"split R-hat per pixel {m.rhat()[0]}")
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
