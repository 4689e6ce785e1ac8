"""Steps per second of the HMC sampler (ct_pvae_amd.mcmc.hmc_sample: one persistent launch per steps_per_launch transitions) against
the same transitions driven from the host through the public calls -- project_tf_fast -> poisson_log_prob -> backward() inside
set_multithreading_enabled(False), with the bijector, the prior and the leapfrog in torch ops -- and the time of the longest single
launch, which is what CTPVAE_HMC_MAX_STEPS / the default steps_per_launch are sized by (largest power of two that keeps the slowest
shape's launch under 100 ms).

    python tools/time_hmc.py [--out profiles/hmc_timing.txt] [--host-steps 100]

Shapes: the 2 x 2 toy (2 angles) with 1 chain and with 1,024 chains, 2,000 steps; 8 x 8 at 180 angles, 256 chains, 512 steps; all with
5 leapfrog steps, and these size the cap.  A last row runs the entry point's worst case (8 x 8, 256 angles, 4 mixture components, 32
leapfrog steps, 256 chains) so that the longest launch the cap allows is a measured figure too.  "hmc_sample ms" is the median of 5
timed calls after one warm-up call, from HIP events around the whole call (init launch, uploads, run launches).  "launch ms" is
the longest ctpvae_hmc_run_f32 launch ALONE over those calls, from HIP events recorded right before and after the entry point."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402


def problem(N, A, dev, seed=0):
    rng = np.random.default_rng(seed)
    theta = np.linspace(0, np.pi, A, endpoint=False).astype(np.float32)
    obj = torch.from_numpy(rng.dirichlet(np.full(N * N, 2.0)).astype(np.float32).reshape(N, N)).to(dev)
    sino = cp.project_tf_fast(obj, theta, pad=False, dim=2)[..., 0][None]                       # [1][A][N]
    mask = torch.full((1, A), 1.0, device=dev)
    meas = torch.poisson(sino * 1e3) / 1e3
    alpha = rng.uniform(0.5, 2.0, (2, N * N))
    return theta, mask, meas, (np.array([0.4, 0.6]), alpha)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


class LaunchTimer:
    """HIP events around every ctpvae_hmc_run_f32 launch, on the stream hmc_sample launches into."""

    def __init__(self):
        self.lib = cp._lib.load()
        self.real = self.lib.ctpvae_hmc_run_f32
        self.events = []

    def __enter__(self):
        def run(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = self.real(*args)
            b.record()
            self.events.append((a, b, args[16]))          # args[16]: n_steps
            return rc
        self.lib.ctpvae_hmc_run_f32 = run
        return self

    def __exit__(self, *exc):
        self.lib.ctpvae_hmc_run_f32 = self.real

    def longest(self):
        """(ms, n_steps) of the longest launch seen."""
        torch.cuda.synchronize()
        return max((a.elapsed_time(b), n) for a, b, n in self.events)


def host_driven(theta, mask, meas, prior, C, steps, L=5, eps=6.5e-2):
    """The sampler composed from the public calls (what a user had before hmc_sample); decisions stay on the device."""
    dev = meas.device
    N = meas.shape[-1]
    K = N * N
    logw = torch.log(torch.tensor(prior[0], dtype=torch.float32, device=dev))
    am1 = torch.tensor(prior[1], dtype=torch.float32, device=dev) - 1
    lbeta = (torch.lgamma(am1 + 1).sum(-1) - torch.lgamma((am1 + 1).sum(-1)))
    off = torch.log(torch.arange(K - 1, 0, -1, dtype=torch.float32, device=dev))
    maskc, measc = mask.expand(C, -1).contiguous(), meas.expand(C, -1, -1).contiguous()
    tiny = float(np.finfo(np.float32).tiny)

    def target(x):
        x = x.detach().requires_grad_(True)
        t = x - off
        lz, l1mz = -torch.nn.functional.softplus(-t), -torch.nn.functional.softplus(t)
        logr = torch.nn.functional.pad(torch.cumsum(l1mz, 1), (1, 0))
        O = torch.exp(torch.nn.functional.pad(lz, (0, 1)) + logr).clamp_min(tiny)
        prior_lp = torch.logsumexp(logw + torch.log(O) @ am1.T - lbeta, dim=1)
        proj = cp.project_tf_fast(O.reshape(C, N, N, 1), theta, pad=False, dim=2, integrate_vae=True)[..., 0]
        T = prior_lp + cp.poisson_log_prob(proj, maskc, measc, 1e3).sum((1, 2)) + (lz + l1mz + logr[:, :-1]).sum(1)
        T.sum().backward()
        return T.detach(), x.grad

    with torch.autograd.set_multithreading_enabled(False):
        x = torch.zeros(C, K - 1, device=dev)
        T, g = target(x)

        def run():
            nonlocal x, T, g
            for _ in range(steps):
                p = torch.randn_like(x)
                k0 = 0.5 * (p * p).sum(1)
                p = p + 0.5 * eps * g
                xn = x
                for l in range(L):
                    xn = xn + eps * p
                    Tn, gn = target(xn)
                    p = p + (0.5 * eps if l == L - 1 else eps) * gn
                lar = (Tn - 0.5 * (p * p).sum(1)) - (T - k0)
                acc = (torch.log(torch.rand(C, device=dev)) < lar)
                x, g, T = torch.where(acc[:, None], xn, x), torch.where(acc[:, None], gn, g), torch.where(acc, Tn, T)
        return timed(run, reps=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hmc_timing.txt"))
    ap.add_argument("--host-steps", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"# tools/time_hmc.py on {torch.cuda.get_device_name(0)}; median (min .. max) of 5 timed calls of hmc_sample; launch ms: the longest",
             "# ctpvae_hmc_run_f32 launch alone (HIP events around the entry point), with its number of transitions",
             "# shape                        L  chains  steps  hmc_sample ms            steps/s  host-driven steps/s    launch ms (steps)"]
    worst_us = 0.0
    rows = (("toy 2x2, 2 angles", 2, 2, 5, 1, 2000, True), ("toy 2x2, 2 angles", 2, 2, 5, 1024, 2000, True),
            ("8x8, 180 angles", 8, 180, 5, 256, 512, True), ("8x8, 256 angles, M=4 (worst)", 8, 256, 32, 256, 64, False))
    for name, N, A, L, C, steps, sizes_cap in rows:
        theta, mask, meas, prior = problem(N, A, dev)
        if not sizes_cap:
            prior = (np.full(4, 0.25), np.random.default_rng(1).uniform(0.5, 2.0, (4, N * N)))
        eps = 6.5e-2 if N == 2 else 1e-2
        spl = min(steps, cp.mcmc.MAX_STEPS_PER_LAUNCH)
        call = lambda: cp.hmc_sample(meas, mask, theta, 1e3, prior=prior, num_results=steps, chains_per_object=C,   # noqa: E731
                                     num_leapfrog_steps=L, step_size=eps, steps_per_launch=spl)
        with LaunchTimer() as lt:
            med, lo, hi = timed(call)
            one_ms, one_n = lt.longest()
        if sizes_cap:
            worst_us = max(worst_us, 1e3 * one_ms / one_n)
            hmed, _, _ = host_driven(theta, mask, meas, prior, C, args.host_steps, L=L, eps=eps)
            host = f"{1e3 * args.host_steps / hmed:10.1f} ({args.host_steps} steps)"
        else:
            worst_case_us = 1e3 * one_ms / one_n
            host = "         - (not run)"
        lines.append(f"{name:29s}{L:3d}{C:8d}{steps:7d}  {med:8.2f} ({lo:.2f} .. {hi:.2f})  {1e3 * steps / med:10.0f}  {host}  {one_ms:9.2f} ({one_n})")
    cap = 1
    while 2 * cap * worst_us <= 100e3:
        cap *= 2
    lines.append(f"# slowest of the shapes that size the cap: {worst_us:.1f} us per transition in a launch -> largest power of two of "
                 f"transitions under 100 ms per launch: {cap}")
    lines.append(f"# worst case the entry point admits: {worst_case_us:.1f} us per transition -> {cap} transitions take "
                 f"{1e-3 * cap * worst_case_us:.0f} ms in one launch")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
