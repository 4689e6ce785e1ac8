"""Forward + backward of the P-VAE's default Beta output head: the chain of torch operations the trainer runs without
--fused_beta_head (two trainer.positive_range, torch.distributions.Beta.rsample, clamp, .log_prob and the per-object sum, under
autograd) against the fused pair of launches (ct_pvae_amd.beta_head, csrc/beta_head.hip), and the trainer's steps per second with and
without --fused_beta_head at the c3 recipe WITHOUT --normal (-b 5 --ns 2, 128 x 128).

    python tools/time_beta_head.py [--out profiles/beta_head_timing.txt] [--steps 100]

Head rows: n = 10 (the c3 recipe's ns * B) and n = 100 objects of 128 x 128; both versions get the same alpha / beta (requires_grad)
and the same cotangents, and run inside torch.autograd.set_multithreading_enabled(False) as the trainer's backward does.  "ms" is the
median (min .. max) of 3 windows of 30 calls each after a warm-up window, from a host clock around work that ends in a device
synchronise; "gpu ms" is the same windows from HIP events.  The two versions alternate window by window.  Trainer rows: 3 alternating
windows of --steps steps each after 20 warm-up steps, median steps per second.  The two versions do not compute the same numbers: the
fused pair draws from Philox and differentiates implicitly, in float64 (csrc/beta_head.hip's header); torch draws from its global
generator and differentiates with _dirichlet_grad in float32.  The header names the device as torch reports it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import trainer as tr  # noqa: E402


def torch_head(alpha, beta, gx, gl, sr):
    dist = torch.distributions.Beta(tr.positive_range(alpha), tr.positive_range(beta))
    x = dist.rsample()
    lp = dist.log_prob(x.clamp(sr, 1 - sr)).sum(dim=(1, 2, 3))
    ((x * gx).sum() + (lp * gl).sum()).backward()


def fused_head(alpha, beta, gx, gl, draw, sr):
    x, lp = cp.beta_head(alpha, beta, seed=1, draw=draw, sqrt_reg=sr)
    torch.autograd.backward((x, lp), (gx.permute(0, 2, 3, 1), gl))


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for i in range(calls):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls, a.elapsed_time(b) / calls


def head_rows(dev, calls=30, windows=3):
    rows = []
    sr = tr.EPS32
    for n in (10, 100):
        g = torch.Generator(device=dev).manual_seed(n)
        alpha = (torch.rand((n, 1, 128, 128), device=dev, generator=g) * 3 - 1).requires_grad_(True)     # the tests' "trainer" range
        beta = (torch.rand((n, 1, 128, 128), device=dev, generator=g) * 3 - 1).requires_grad_(True)
        gx, gl = torch.randn((n, 1, 128, 128), device=dev, generator=g), torch.randn((n,), device=dev, generator=g)

        def clear():
            alpha.grad = beta.grad = None
        fns = {"torch ops": lambda i: (clear(), torch_head(alpha, beta, gx, gl, sr)),
               "fused pair": lambda i: (clear(), fused_head(alpha, beta, gx, gl, i, sr))}
        res = {k: [] for k in fns}
        with torch.autograd.set_multithreading_enabled(False):
            for k, f in fns.items():
                window(f, calls)
            for _ in range(windows):
                for k, f in fns.items():
                    res[k].append(window(f, calls))
        for k, v in res.items():
            host, gpu = np.array(v).T
            rows.append(f"beta head fwd+bwd  n={n:<4d} {k:11s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                        f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})")
        t, f = np.array(res["torch ops"]), np.array(res["fused pair"])
        overlap = ["the windows overlap" if f[:, j].max() >= t[:, j].min() and t[:, j].max() >= f[:, j].min() else "the windows do not overlap"
                   for j in (0, 1)]
        rows.append(f"#   n={n}: torch ops / fused pair = {np.median(t[:, 0]) / np.median(f[:, 0]):.2f}x host clock ({overlap[0]}), "
                    f"{np.median(t[:, 1]) / np.median(f[:, 1]):.2f}x HIP events ({overlap[1]})")
    return rows


def trainer_rows(dev, steps, windows=3):
    """Two trainers at the c3 recipe without --normal (Beta latents, Beta(0.5, 0.5) prior, Beta output): with and without
    --fused_beta_head."""
    recipe = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random -i 1000 --train"
    flags = ["", " --fused_beta_head"]
    ts = {f: tr.PVAETrainer(tr.get_args((recipe + f).split()), dev) for f in flags}
    rate = {f: [] for f in flags}

    def run(f, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ts[f].train_step(sync=False)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    for f in flags:
        run(f, 20)
    for _ in range(windows):
        for f in flags:
            rate[f].append(run(f, steps))
    rows = [f"trainer c3 without --normal ({steps} steps / window)  {(f.strip() or 'unfused'):20s} {np.median(v):8.1f} steps/s "
            f"({min(v):.1f} .. {max(v):.1f})   {1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    u, f = rate[flags[0]], rate[flags[1]]
    overlap = "the windows overlap" if max(f) >= min(u) and max(u) >= min(f) else "the windows do not overlap"
    rows.append(f"#   --fused_beta_head / unfused = {np.median(f) / np.median(u):.3f}x steps/s ({overlap})")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beta_head_timing.txt"))
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_beta_head.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_beta_head.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over 3 alternating windows",
             "# what                                    ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += head_rows(dev)
    lines += trainer_rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
