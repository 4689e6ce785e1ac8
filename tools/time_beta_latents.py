"""Forward + backward of the P-VAE's default Beta latent block: the chain of torch operations the trainer runs without
--fused_beta_latents (chunk / positive_range / Beta.rsample -- the Dirichlet sampler and _dirichlet_grad -- / kl_divergence against
Beta(0.5, 0.5) and its per-object sum, under autograd) against the fused pair of launches per level (ct_pvae_amd.beta_latents,
csrc/beta_latent.hip), the number of device launches of both, and the trainer's steps per second without --normal with neither, each
and both of --fused_beta_latents / --fused_beta_head at the c3 recipe (README: -b 5 --ns 2 --api 20, 128 x 128, --nb 3).

    python tools/time_beta_latents.py [--out profiles/beta_latents_timing.txt] [--steps 100]

Latent rows: the four skip levels of the c3 encoder (their shapes are read from an EncodeNet built as the trainer builds it), B = 5,
ns = 2; both versions get the same skip tensors (requires_grad from level 1 on) and the same cotangents for z and for the KL of levels
1 .. 3 (level 0's KL is not computed by either, as in the trainer), and run inside torch.autograd.set_multithreading_enabled(False)
as the trainer's backward does.  "ms" is the median (min .. max) of 3 windows of 50 calls each after a warm-up window, from a host
clock around work that ends in a device synchronise -- what a host-bound training step pays; "gpu ms" is the same windows from HIP
events.  The two versions alternate window by window.  Launch rows: device kernels per call of all four levels, forward + backward,
counted by torch.profiler.  Level rows: per level the forward launch without and with its KL workgroups, and the pair with the
backward (both cotangents), HIP events -- what the float64 work costs.  Trainer rows: 3 alternating windows of --steps steps each
after 30 warm-up steps, median steps per second.  No time is promised: the torch chain of the same run is the yardstick, and a loss is reported as one.  The header names the device as
torch reports it, with its gfx architecture."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import trainer as tr  # noqa: E402

RECIPE = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random -i 1000 --train"
NS = 2


def torch_latents(skips, gz, gk):
    """trainer.find_loss_vae_unsup's q / q_sample / kl lines of the default path."""
    q = []
    for sk in skips:
        loc, log_scale = sk.chunk(2, dim=1)
        q.append(torch.distributions.Beta(tr.positive_range(loc), tr.positive_range(log_scale)))
    B = skips[0].shape[0]
    z = [d.rsample((NS,)).reshape((NS * B,) + tuple(d.concentration1.shape[1:])) for d in q]
    kl = sum(torch.distributions.kl_divergence(d, torch.distributions.Beta(torch.full_like(d.concentration1, 0.5),
                                                                             torch.full_like(d.concentration1, 0.5)))
             .sum(dim=(1, 2, 3)) for d in q[1:])
    pairs = [(a, g) for a, g in zip(z, gz) if a.requires_grad] + [(kl, gk)]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])


def fused_latents(skips, gz, gk, draw):
    outs = [cp.beta_latents(sk, ns=NS, seed=1, draw=draw, level=level, want_kl=level > 0) for level, sk in enumerate(skips)]
    kl = sum((o[1] for o in outs[2:]), outs[1][1])
    pairs = [(o[0], g) for o, g in zip(outs, gz) if o[0].requires_grad] + [(kl, gk)]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])


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


def count_launches(fn):
    """Device kernels and copies of one call, from torch.profiler's device-side events."""
    from torch.profiler import ProfilerActivity, profile
    fn(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(1)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def latent_rows(dev, calls=50, windows=3):
    args = tr.get_args(RECIPE.split())
    fm = [int(args.nfm * args.nfmm ** i) for i in range(args.num_blocks)]
    enc = tr.EncodeNet(len(args.algorithms) + 1, fm, 2, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        shapes = [tuple(s.shape) for s in enc(torch.rand((args.batch_size, len(args.algorithms) + 1, 128, 128), device=dev, generator=g))]
    # level 0 is the (repeated) input: it needs no gradient in the trainer either, so its backward is not run by either version
    skips = [(torch.rand(s, device=dev, generator=g) * 3 - 1).requires_grad_(level > 0) for level, s in enumerate(shapes)]   # np_twin_beta's "trainer" range
    gz = [torch.randn((NS * s[0], s[1] // 2) + s[2:], device=dev, generator=g) for s in shapes]
    gk = torch.randn((shapes[0][0],), device=dev, generator=g)

    def clear():
        for sk in skips:
            sk.grad = None
    fns = {"torch ops": lambda i: (clear(), torch_latents(skips, gz, gk)),
           "fused pairs": lambda i: (clear(), fused_latents(skips, gz, gk, i))}
    res = {k: [] for k in fns}
    rows = ["# skip levels [B][2C][H][W]: " + ", ".join("x".join(map(str, s)) for s in shapes)]
    with torch.autograd.set_multithreading_enabled(False):
        for k, f in fns.items():
            window(f, calls)
        for _ in range(windows):
            for k, f in fns.items():
                res[k].append(window(f, calls))
        launches = {k: count_launches(f) for k, f in fns.items()}
    for k, v in res.items():
        host, gpu = np.array(v).T
        rows.append(f"Beta latents fwd+bwd, 4 levels  {k:11s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                    f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})   {launches[k]:4d} device launches per call")
    rows.append(f"#   torch ops / fused pairs = {np.median(np.array(res['torch ops'])[:, 0]) / np.median(np.array(res['fused pairs'])[:, 0]):.2f}x "
                f"host clock, {np.median(np.array(res['torch ops'])[:, 1]) / np.median(np.array(res['fused pairs'])[:, 1]):.2f}x HIP events, "
                f"{launches['torch ops'] - launches['fused pairs']} launches fewer")
    # where the fused time goes: per level the forward launch with and without its KL workgroups (the float64 part of the forward, B
    # workgroups) and the pair with the backward (float64 throughout), HIP events, median of the same number of windows
    def level_ms(fn):
        window(fn, calls)
        return float(np.median([window(fn, calls)[1] for _ in range(windows)]))
    for level, sk in enumerate(skips):
        leaf = sk.detach().clone().requires_grad_(True)

        def fwd(i, kl):
            with torch.no_grad():
                cp.beta_latents(leaf, ns=NS, seed=1, draw=i, level=level, want_kl=kl)

        def pair(i):
            leaf.grad = None
            z, kl = cp.beta_latents(leaf, ns=NS, seed=1, draw=i, level=level)
            torch.autograd.backward([z, kl], [gz[level], gk])
        with torch.autograd.set_multithreading_enabled(False):
            rows.append(f"#   level {level} ({'x'.join(map(str, shapes[level]))}): forward without KL {level_ms(lambda i: fwd(i, False)):.4f}, forward with KL "
                        f"{level_ms(lambda i: fwd(i, True)):.4f}, forward with KL + backward {level_ms(pair):.4f} gpu ms")
    return rows


def trainer_rows(dev, steps, windows=3):
    flags = ["", " --fused_beta_latents", " --fused_beta_head", " --fused_beta_head --fused_beta_latents"]
    ts = {f: tr.PVAETrainer(tr.get_args((RECIPE + f).split()), dev) for f in flags}
    rate = {f: [] for f in flags}

    def run(f, n):
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
    rows = [f"trainer c3 without --normal ({steps} steps / window)  {(f.strip() or 'neither flag'):40s} {np.median(v):8.1f} steps/s "
            f"({min(v):.1f} .. {max(v):.1f})   {1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    med = {f: np.median(v) for f, v in rate.items()}
    rows.append(f"#   steps/s against neither flag: --fused_beta_latents {med[flags[1]] / med[flags[0]]:.3f}x, --fused_beta_head "
                f"{med[flags[2]] / med[flags[0]]:.3f}x, both {med[flags[3]] / med[flags[0]]:.3f}x; both / --fused_beta_head alone "
                f"{med[flags[3]] / med[flags[2]]:.3f}x")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beta_latents_timing.txt"))
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_beta_latents.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_beta_latents.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over 3 alternating windows",
             "# what                                         ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += latent_rows(dev)
    lines += trainer_rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
