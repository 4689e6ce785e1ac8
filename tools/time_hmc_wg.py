"""Transitions per second of the workgroup form of the HMC sampler (hmc_sample(form="workgroup"), csrc/hmc_wg.hip: one workgroup of
ceil(N * N / 64) waves per chain) against the same transitions driven from the host through the public calls (tools/time_hmc.py's
loop: project_tf_fast -> poisson_log_prob -> backward(), the only way to sample these sizes without it), and the time of the longest
single launch, which is what ct_pvae_amd.mcmc.MAX_STEPS_PER_LAUNCH_WG is sized by.

    python tools/time_hmc_wg.py [--out profiles/hmc_wg_timing.txt] [--host-steps 10]

Shapes (N, A) = (9, 20), (16, 20), (16, 90), (32, 20), each with 1 chain and with one full residency of chains (what
ctpvae_hmc_wg_resident_chains reports: the most one launch holds), 5 leapfrog steps.  Nobody had measured a transition at these
sizes, so every (shape, chains) starts at 8 transitions per launch and doubles, up to 512, only while the time PROJECTED from the
launch just measured stays under 100 ms; the launch times are HIP events around ctpvae_hmc_wg_run_f32 alone.  Throughput: 3
alternating windows (workgroup form, host loop, workgroup form, ...) on the host clock, each a whole call with the device drained
before and after; median (min .. max).  A last pair of rows runs 8 x 8 at 20 angles in both forms, where they give the same bits."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ct_pvae_amd as cp  # noqa: E402
from time_hmc import problem  # noqa: E402

LIMIT_MS = 100.0
EPS = 1e-2


class LaunchTimer:
    """HIP events around every launch of one run entry point, on the stream hmc_sample launches into."""

    def __init__(self, name):
        self.lib, self.name = cp._lib.load(), name
        self.real = getattr(self.lib, name)
        self.events = []

    def __enter__(self):
        def run(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = self.real(*args)
            b.record()
            self.events.append((a, b, args[16]))          # args[16]: n_steps
            return rc
        setattr(self.lib, self.name, run)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.real)

    def longest(self):
        """(ms, n_steps) of the longest launch seen."""
        torch.cuda.synchronize()
        return max((a.elapsed_time(b), n) for a, b, n in self.events)


def host_loop(theta, mask, meas, prior, C, steps, L=5, eps=EPS):
    """tools/time_hmc.py's host-driven sampler as a callable that runs `steps` transitions of C chains."""
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

    state = {}

    def run():
        with torch.autograd.set_multithreading_enabled(False):
            if not state:
                x = torch.zeros(C, K - 1, device=dev)
                state["x"], (state["T"], state["g"]) = x, target(x)
            x, T, g = state["x"], state["T"], state["g"]
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
            state["x"], state["T"], state["g"] = x, T, g
    return run


def window(fn):
    """One call on the host clock, the device drained before and after: ms."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def alternating(fns, windows=3):
    """windows rounds over fns in turn after one untimed call of each: per fn (median, min, max) ms."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            ms[i].append(window(fn))
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def climb(call):
    """Start at 8 transitions per launch; double (to 512 at most) only while the projection from the launch just measured stays under
    100 ms.  Returns (transitions per launch reached, ms of that launch, us per transition)."""
    spl = 8
    while True:
        with LaunchTimer("ctpvae_hmc_wg_run_f32") as lt:
            call(spl, spl)
            ms, n = lt.longest()
        assert n == spl
        if spl >= 512 or 2.0 * ms >= LIMIT_MS:
            return spl, ms, 1e3 * ms / spl
        spl *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hmc_wg_timing.txt"))
    ap.add_argument("--host-steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = cp._lib.load()
    cp.mcmc.MAX_STEPS_PER_LAUNCH_WG = 512      # this tool is what sizes the shipped value: it climbs to its own limit, launch by launch
    lines = [f"# tools/time_hmc_wg.py on {torch.cuda.get_device_name(0)}; hmc_sample(form='workgroup'), 5 leapfrog steps, step size {EPS}",
             "# steps: transitions per launch reached from 8 by doubling while the projected launch stays under 100 ms; launch ms: that launch",
             "# alone (HIP events around ctpvae_hmc_wg_run_f32); call ms and transitions/s: median (min .. max) of 3 alternating windows on the",
             f"# host clock, a call of `steps` transitions against {args.host_steps} transitions of the host-driven loop; chains: 1, and one full residency",
             "# shape            chains  steps  launch ms  us/transition  call ms                    transitions/s    host loop transitions/s      x"]
    slowest = 0.0
    for N, A in ((9, 20), (16, 20), (16, 90), (32, 20)):
        theta, mask, meas, prior = problem(N, A, dev)
        full = ctypes.c_int(0)
        cp._lib.check(lib.ctpvae_hmc_wg_resident_chains(N, A, ctypes.byref(full)), "hmc_wg_resident_chains")
        for C in (1, full.value):
            call = lambda steps, spl: cp.hmc_sample(meas, mask, theta, 1e3, prior=prior, num_results=steps, chains_per_object=C,   # noqa: E731
                                                    step_size=EPS, steps_per_launch=spl, form="workgroup")
            spl, ms, us = climb(call)
            if C > 1:
                slowest = max(slowest, us)
            (med, lo, hi), (hmed, hlo, hhi) = alternating([lambda: call(spl, spl),
                                                           host_loop(theta, mask, meas, prior, C, args.host_steps)])
            rate, hrate = 1e3 * spl / med, 1e3 * args.host_steps / hmed
            lines.append(f"{N:2d}x{N:<2d}, {A:3d} angles{C:8d}{spl:7d}{ms:11.2f}{us:15.1f}  {med:8.2f} ({lo:.2f} .. {hi:.2f})  {rate:12.0f}"
                         f"  {hrate:9.1f} ({1e3 * args.host_steps / hhi:.1f} .. {1e3 * args.host_steps / hlo:.1f})  {rate / hrate:7.1f}")
    cap = 8
    while cap < 512 and 2 * cap * slowest < 1e3 * LIMIT_MS:
        cap *= 2
    lines.append(f"# slowest full-residency shape: {slowest:.1f} us per transition in a launch -> largest power of two of transitions (at most "
                 f"512) under 100 ms per launch: MAX_STEPS_PER_LAUNCH_WG = {cap}")
    # one wave per workgroup: the two forms give the same bits
    theta, mask, meas, prior = problem(8, 20, dev)
    lines.append("# 8x8, 20 angles, one launch per call: the workgroup form (one wave per workgroup) against the wave form, which gives the same bits")
    for C in (1, 256):
        run = lambda steps, spl, f="workgroup": cp.hmc_sample(meas, mask, theta, 1e3, prior=prior, num_results=steps,   # noqa: E731
                                                              chains_per_object=C, step_size=EPS, steps_per_launch=spl, form=f)
        spl, _, us = climb(run)
        (med, lo, hi), (wmed, wlo, whi) = alternating([lambda: run(spl, spl), lambda: run(spl, spl, "wave")])
        lines.append(f" 8x8 ,  20 angles{C:8d}{spl:7d}  workgroup {med:8.2f} ({lo:.2f} .. {hi:.2f}) ms {1e3 * spl / med:9.0f}/s ({us:.1f} us/transition "
                     f"in the launch)   wave {wmed:8.2f} ({wlo:.2f} .. {whi:.2f}) ms {1e3 * spl / wmed:9.0f}/s   workgroup / wave time {med / wmed:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
