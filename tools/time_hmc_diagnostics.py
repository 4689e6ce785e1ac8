"""Transitions per second and peak device memory of hmc_marginals(max_lag=, cov=, keep_samples=False) (ct_pvae_amd.mcmc,
csrc/hmc_diagnostics.hip: the raw sums of the autocovariance and of the covariance between pixels accumulated inside the sampler's
launches) against hmc_marginals without them (csrc/hmc_marginals.hip, unchanged) and against hmc_sample followed by the same sums from
its stored samples, and the time of the longest single launch of the new kernel, which decides whether it may share
CTPVAE_HMC_MAX_STEPS (a launch stays under 100 ms).

    python tools/time_hmc_diagnostics.py [--out profiles/hmc_diagnostics_timing.txt] [--windows 3]

Shapes: those of tools/time_hmc_marginals.py -- the 2 x 2 toy with 1 chain and with 1,024 chains, 2,000 steps; 8 x 8 at 180 angles,
256 chains, 512 steps; 5 leapfrog steps, 50 bins.  Paths, each timed from the call to the end of a device synchronisation (so the
host's share counts), in alternating windows after one warm-up round:
    marginals       hmc_marginals(keep_samples=False), the baseline
    lag16, lag64    the same call with max_lag=16 / 64
    lag16+cov, lag64+cov   and with cov=True
    sample+torch    hmc_sample, then the lagged products of 64 lags and the cross products of ALL chains in float64 with torch
                    operations on the device
Reported: the median over the windows with min and max, as transitions per second of one chain (steps / time), the time relative to
the baseline's median, and the peak of torch.cuda.max_memory_allocated() above what was allocated before the call.  Last lines: the
longest ctpvae_hmc_run_diagnostics_f32 launch alone (HIP events around the entry point) at 8 x 8, 180 angles, 256 chains, 512 steps:
with 64 lags, cov and 50 bins, and with 254 bins, 16 lags and cov (254 bins with 64 lags and cov exceed a workgroup's LDS)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ct_pvae_amd as cp  # noqa: E402
from time_hmc import problem  # noqa: E402

LO, WIDTH, BINS = 0.005, 0.01, 50


def torch_sums(samples, max_lag=64):
    """lag float64 [max_lag + 1][C][K] and xx float64 [C][K][K] of stored samples [n][C][K], with torch operations."""
    x = samples.double()
    n = x.shape[0]
    lag = torch.stack([(x[l:] * x[:n - l]).sum(0) for l in range(min(max_lag + 1, n))])
    return lag, torch.einsum("nck,nci->cki", x, x)


def window(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t)
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return ms, peak


class LaunchTimer:
    """HIP events around every ctpvae_hmc_run_diagnostics_f32 launch."""

    def __init__(self):
        self.lib = cp._lib.load()
        self.real = self.lib.ctpvae_hmc_run_diagnostics_f32
        self.events = []

    def __enter__(self):
        def run(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = self.real(*args)
            b.record()
            self.events.append((a, b, args[16]))          # args[16]: n_steps
            return rc
        self.lib.ctpvae_hmc_run_diagnostics_f32 = run
        return self

    def __exit__(self, *exc):
        self.lib.ctpvae_hmc_run_diagnostics_f32 = self.real

    def longest(self):
        torch.cuda.synchronize()
        return max((a.elapsed_time(b), n) for a, b, n in self.events)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "hmc_diagnostics_timing.txt"))
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_hmc_diagnostics.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {args.windows} alternating windows "
             "per path, each from the call to the end of a device synchronisation;",
             "# transitions/s of one chain = steps / time; x base: median time / the marginals path's median; peak MB: device memory above "
             f"what was allocated before the call; {BINS} bins",
             "# shape              chains  steps  path          ms                        transitions/s (min .. max)     x base  peak MB"]
    rows = (("toy 2x2, 2 angles", 2, 2, 1, 2000), ("toy 2x2, 2 angles", 2, 2, 1024, 2000), ("8x8, 180 angles", 8, 180, 256, 512))
    for name, N, A, C, steps in rows:
        theta, mask, meas, prior = problem(N, A, dev)
        kw = dict(prior=prior, num_results=steps, chains_per_object=C, num_leapfrog_steps=5, step_size=6.5e-2 if N == 2 else 1e-2,
                  steps_per_launch=min(steps, cp.mcmc.MAX_STEPS_PER_LAUNCH))

        def marg(kw=kw, theta=theta, mask=mask, meas=meas, **more):
            return cp.hmc_marginals(meas, mask, theta, 1e3, bins=BINS, lo=LO, width=WIDTH, **more, **kw)
        paths = {
            "marginals": marg,
            "lag16": lambda: marg(max_lag=16),
            "lag64": lambda: marg(max_lag=64),
            "lag16+cov": lambda: marg(max_lag=16, cov=True),
            "lag64+cov": lambda: marg(max_lag=64, cov=True),
            "sample+torch": lambda: torch_sums(cp.hmc_sample(meas, mask, theta, 1e3, **kw)[0]),
        }
        got = {k: [] for k in paths}
        for w in range(args.windows + 1):                      # round 0 warms up
            for k, fn in paths.items():
                r = window(fn)
                if w:
                    got[k].append(r)
        base = float(np.median([r[0] for r in got["marginals"]]))
        for k, rs in got.items():
            ms = sorted(r[0] for r in rs)
            med, lo, hi = float(np.median(ms)), ms[0], ms[-1]
            lines.append(f"{name:19s}{C:7d}{steps:7d}  {k:12s}  {med:8.2f} ({lo:.2f} .. {hi:.2f})  "
                         f"{1e3 * steps / med:10.0f} ({1e3 * steps / hi:.0f} .. {1e3 * steps / lo:.0f})  {med / base:6.3f}  "
                         f"{max(r[1] for r in rs) / 1e6:7.2f}")
    # the longest launches the shared cap allows
    theta, mask, meas, prior = problem(8, 180, dev)
    for what, grid, more in (("50 bins, 64 lags, cov", dict(bins=BINS, lo=LO, width=WIDTH), dict(max_lag=64, cov=True)),
                             ("254 bins, 16 lags, cov", dict(bins=254, lo=0.0, width=2e-4), dict(max_lag=16, cov=True))):
        with LaunchTimer() as lt:
            for _ in range(4):
                cp.hmc_marginals(meas, mask, theta, 1e3, prior=prior, num_results=512, chains_per_object=256, num_leapfrog_steps=5,
                                 step_size=1e-2, steps_per_launch=512, **grid, **more)
            one_ms, one_n = lt.longest()
        cap = 1
        while 2 * cap * one_ms / one_n <= 100.0:
            cap *= 2
        lines.append(f"# longest ctpvae_hmc_run_diagnostics_f32 launch at 8x8, 180 angles, 256 chains, {what}: {one_ms:.2f} ms for {one_n} "
                     f"transitions ({1e3 * one_ms / one_n:.1f} us each) -> largest power of two of transitions under 100 ms per launch: {cap} "
                     f"(CTPVAE_HMC_MAX_STEPS is {cp.mcmc.MAX_STEPS_PER_LAUNCH})")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
