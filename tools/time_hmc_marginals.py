"""Transitions per second and peak device memory of hmc_marginals(keep_samples=False) (ct_pvae_amd.mcmc, csrc/hmc_marginals.hip: the
statistics accumulated inside the sampler's launches) against hmc_sample followed by binning its stored samples, and the time of the
longest single launch of the new kernel, which decides whether it may share CTPVAE_HMC_MAX_STEPS (a launch stays under 100 ms).

    python tools/time_hmc_marginals.py [--out profiles/hmc_marginals_timing.txt] [--windows 3]

Shapes: those of tools/time_hmc.py that size the cap -- the 2 x 2 toy with 1 chain and with 1,024 chains, 2,000 steps; 8 x 8 at 180
angles, 256 chains, 512 steps; 5 leapfrog steps, 50 bins.  Paths, each timed from the call to the end of a device synchronisation (so
the host's share counts), in alternating windows after one warm-up round:
    marginals     hmc_marginals(keep_samples=False)
    sample+torch  hmc_sample, then histogram and float64 moments of ALL chains with torch operations on the device
    sample+host   hmc_sample, then the README's bin_samples(samples[:, 0].cpu().numpy(), ...) of chain 0 alone
Reported: the median over the windows with min and max, as transitions per second of one chain (steps / time), and for the first two
paths the peak of torch.cuda.max_memory_allocated() above what was allocated before the call.  Last line: the longest
ctpvae_hmc_run_marginals_f32 launch alone (HIP events around the entry point) at 8 x 8, 180 angles, 256 chains, 512 steps, 254 bins."""
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


def torch_stats(samples):
    """hist int64 [K][BINS + 2] over all chains under the library's bin rule, and the float64 sums, with torch operations."""
    K = samples.shape[-1]
    t = (samples - LO) / WIDTH
    col = torch.where(t >= BINS, BINS + 1, 1 + t.clamp(0, BINS).to(torch.int64))
    col = torch.where(t >= 0, col, torch.zeros_like(col))
    flat = (torch.arange(K, device=samples.device) * (BINS + 2) + col).reshape(-1)
    x = samples.double()
    return torch.bincount(flat, minlength=K * (BINS + 2)).view(K, BINS + 2), x.sum(0), (x * x).sum(0)


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
    """HIP events around every ctpvae_hmc_run_marginals_f32 launch."""

    def __init__(self):
        self.lib = cp._lib.load()
        self.real = self.lib.ctpvae_hmc_run_marginals_f32
        self.events = []

    def __enter__(self):
        def run(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = self.real(*args)
            b.record()
            self.events.append((a, b, args[16]))          # args[16]: n_steps
            return rc
        self.lib.ctpvae_hmc_run_marginals_f32 = run
        return self

    def __exit__(self, *exc):
        self.lib.ctpvae_hmc_run_marginals_f32 = self.real

    def longest(self):
        torch.cuda.synchronize()
        return max((a.elapsed_time(b), n) for a, b, n in self.events)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "hmc_marginals_timing.txt"))
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_hmc_marginals.py on {torch.cuda.get_device_name(0)}; median (min .. max) of {args.windows} alternating windows "
             "per path, each from the call to the end of a device synchronisation;",
             f"# transitions/s of one chain = steps / time; peak MB: device memory above what was allocated before the call; {BINS} bins",
             "# shape              chains  steps  path          ms                        transitions/s (min .. max)      peak MB"]
    rows = (("toy 2x2, 2 angles", 2, 2, 1, 2000), ("toy 2x2, 2 angles", 2, 2, 1024, 2000), ("8x8, 180 angles", 8, 180, 256, 512))
    for name, N, A, C, steps in rows:
        theta, mask, meas, prior = problem(N, A, dev)
        kw = dict(prior=prior, num_results=steps, chains_per_object=C, num_leapfrog_steps=5, step_size=6.5e-2 if N == 2 else 1e-2,
                  steps_per_launch=min(steps, cp.mcmc.MAX_STEPS_PER_LAUNCH))
        paths = {
            "marginals": lambda: cp.hmc_marginals(meas, mask, theta, 1e3, bins=BINS, lo=LO, width=WIDTH, **kw),
            "sample+torch": lambda: torch_stats(cp.hmc_sample(meas, mask, theta, 1e3, **kw)[0].view(-1, N * N)),
            "sample+host": lambda: cp.bin_samples(cp.hmc_sample(meas, mask, theta, 1e3, **kw)[0][:, 0].cpu().numpy(), LO, WIDTH, BINS),
        }
        got = {k: [] for k in paths}
        for w in range(args.windows + 1):                      # round 0 warms up
            for k, fn in paths.items():
                r = window(fn)
                if w:
                    got[k].append(r)
        for k, rs in got.items():
            ms = sorted(r[0] for r in rs)
            med, lo, hi = float(np.median(ms)), ms[0], ms[-1]
            peak = "      -" if k == "sample+host" else f"{max(r[1] for r in rs) / 1e6:7.2f}"
            lines.append(f"{name:19s}{C:7d}{steps:7d}  {k:12s}  {med:8.2f} ({lo:.2f} .. {hi:.2f})  "
                         f"{1e3 * steps / med:10.0f} ({1e3 * steps / hi:.0f} .. {1e3 * steps / lo:.0f})  {peak}")
    # the longest launch the shared cap allows, with the largest count table
    theta, mask, meas, prior = problem(8, 180, dev)
    with LaunchTimer() as lt:
        for _ in range(4):
            cp.hmc_marginals(meas, mask, theta, 1e3, prior=prior, bins=254, lo=0.0, width=2e-4, num_results=512, chains_per_object=256,
                             num_leapfrog_steps=5, step_size=1e-2, steps_per_launch=512)
        one_ms, one_n = lt.longest()
    cap = 1
    while 2 * cap * one_ms / one_n <= 100.0:
        cap *= 2
    lines.append(f"# longest ctpvae_hmc_run_marginals_f32 launch at 8x8, 180 angles, 256 chains, 254 bins: {one_ms:.2f} ms for {one_n} transitions "
                 f"({1e3 * one_ms / one_n:.1f} us each) -> largest power of two of transitions under 100 ms per launch: {cap} "
                 f"(CTPVAE_HMC_MAX_STEPS is {cp.mcmc.MAX_STEPS_PER_LAUNCH})")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
