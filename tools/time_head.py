"""Forward + backward of the P-VAE's TruncatedNormal output head: the chain of torch operations the trainer runs without
--fused_head (trainer.positive_range / TruncatedNormal.rsample / .log_prob and the per-object sum, under autograd) against the fused
pair of launches (ct_pvae_amd.truncated_normal_head, csrc/head.hip), and the trainer's steps per second with and without --fused_head
at the c3 recipe (README: -b 5 --ns 2, 128 x 128).

    python tools/time_head.py [--out profiles/head_timing.txt] [--steps 200]

Head rows: n objects of 128 x 128; both versions get the same alpha / beta (requires_grad) and the same cotangents, and run inside
torch.autograd.set_multithreading_enabled(False) as the trainer's backward does.  "ms" is the median (min .. max) of 7 windows of 50
calls each after a warm-up window, from a host clock around work that ends in a device synchronise -- what a host-bound training step
pays; "gpu ms" is the same windows from HIP events.  The two versions alternate window by window.  Trainer rows: 3 alternating windows
of --steps steps each after 30 warm-up steps, median steps per second, with and without --fused_head, each under torch's default
convolution algorithms and under --reproducible.  The header names the device as torch reports it, with its gfx architecture."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import trainer as tr  # noqa: E402


def torch_head(alpha, beta, gx, gl):
    dist = tr.TruncatedNormal(tr.positive_range(alpha), tr.positive_range(beta), low=0.0, high=1e10)
    x = dist.rsample()
    lp = dist.log_prob(x).sum(dim=(1, 2, 3))
    ((x * gx).sum() + (lp * gl).sum()).backward()


def fused_head(alpha, beta, gx, gl, draw):
    x, lp = cp.truncated_normal_head(alpha, beta, seed=1, draw=draw)
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


def head_rows(dev, calls=50, windows=7):
    rows = []
    for n in (10, 100):
        g = torch.Generator(device=dev).manual_seed(n)
        alpha = (torch.rand((n, 1, 128, 128), device=dev, generator=g) * 3 - 1).requires_grad_(True)
        beta = (torch.rand((n, 1, 128, 128), device=dev, generator=g) * 3.5 - 3).requires_grad_(True)
        gx, gl = torch.randn((n, 1, 128, 128), device=dev, generator=g), torch.randn((n,), device=dev, generator=g)

        def clear():
            alpha.grad = beta.grad = None
        fns = {"torch ops": lambda i: (clear(), torch_head(alpha, beta, gx, gl)),
               "fused pair": lambda i: (clear(), fused_head(alpha, beta, gx, gl, i))}
        res = {k: [] for k in fns}
        with torch.autograd.set_multithreading_enabled(False):
            for k, f in fns.items():
                window(f, calls)
            for _ in range(windows):
                for k, f in fns.items():
                    res[k].append(window(f, calls))
        for k, v in res.items():
            host, gpu = np.array(v).T
            rows.append(f"head fwd+bwd  n={n:<4d} {k:11s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                        f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})")
        rows.append(f"#   n={n}: torch ops / fused pair = {np.median(np.array(res['torch ops'])[:, 0]) / np.median(np.array(res['fused pair'])[:, 0]):.2f}x "
                    f"host clock, {np.median(np.array(res['torch ops'])[:, 1]) / np.median(np.array(res['fused pair'])[:, 1]):.2f}x HIP events")
    return rows


def trainer_rows(dev, steps, windows=3):
    """Four trainers at the c3 recipe: with and without --fused_head, each with torch's default convolution algorithms and with
    --reproducible.  torch.backends.cudnn.deterministic is process-wide, so every window sets it as its row's flags leave it."""
    recipe = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random --normal -i 1000 --train"
    default = torch.backends.cudnn.deterministic
    flags = ["", " --fused_head", " --reproducible", " --fused_head --reproducible"]
    ts = {}
    for f in flags:
        torch.backends.cudnn.deterministic = default
        ts[f] = tr.PVAETrainer(tr.get_args((recipe + f).split()), dev)
    rate = {f: [] for f in flags}

    def run(f, n):
        torch.backends.cudnn.deterministic = default or "--reproducible" in f
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ts[f].train_step(sync=False)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    for f in flags:
        run(f, 30)
    for _ in range(windows):
        for f in flags:
            rate[f].append(run(f, steps))
    torch.backends.cudnn.deterministic = default
    rows = [f"trainer c3 ({steps} steps / window)  {(f.strip() or 'unfused'):30s} {np.median(v):8.1f} steps/s ({min(v):.1f} .. {max(v):.1f})   "
            f"{1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    med = {f: np.median(v) for f, v in rate.items()}
    rows.append(f"#   --fused_head / unfused = {med[flags[1]] / med[flags[0]]:.3f}x steps/s with the default convolutions, "
                f"{med[flags[3]] / med[flags[2]]:.3f}x with --reproducible; --reproducible / default = {med[flags[2]] / med[flags[0]]:.3f}x")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "head_timing.txt"))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_head.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_head.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over alternating windows",
             "# what                               ms per call, host clock + synchronise     gpu ms per call, HIP events"]
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
