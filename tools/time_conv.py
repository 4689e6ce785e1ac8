"""Forward + backward of the 16 padded ConvBlocks of the c3 networks -- periodic pad, convolution, maxout -- as the fused operation
(ct_pvae_amd.periodic_conv_maxout, csrc/conv.hip) against the trainer's torch chain (trainer._PeriodicPad, torch's convolution,
trainer._Maxout) with the library's default algorithms and with torch.backends.cudnn.deterministic; the device launches of each; and
the trainer's steps per second with and without --fused_conv, with and without --reproducible, at the c3 recipe (README: -b 5 --ns 2
--api 20, 128 x 128, --nb 3) on top of --fused_head --fused_latents --fused_blocks --fused_update.

    python tools/time_conv.py [--out profiles/conv_timing.txt] [--steps 200]

Block rows: the shapes are read with forward hooks from an EncodeNet (B = 5) and a DecodeNet (ns * B = 10) built as the trainer builds
them; the three versions get the same inputs (requires_grad, but for the first encoder block's, which is data in the trainer too), the
same parameters and the same cotangents, inside torch.autograd.set_multithreading_enabled(False) as the trainer's backward is.  "ms"
is the median (min .. max) of 5 windows of 20 calls each after a warm-up window, from a host clock around work that ends in a device
synchronise; "gpu ms" is the same windows from HIP events.  The versions alternate window by window.  Launch rows: device kernels per
call, counted by torch.profiler.  Trainer rows: 3 alternating windows of --steps steps each after 30 warm-up steps, median steps per
second; the baseline is this commit with the flag off, in the same process and the same windows; torch's deterministic switch is set
per window to what the run's --reproducible asks.  The header names the device as torch reports it, with its gfx architecture."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import trainer as tr  # noqa: E402

RECIPE = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random --normal -i 1000 --train"
BASE = " --fused_head --fused_latents --fused_blocks --fused_update"
NS = 2
VERSIONS = ("fused", "torch default", "torch deterministic")


def padded_blocks(dev):
    """The 16 padded blocks in the order they run, encoder first: dict(x, w, b, g, stride, pads, first) on the device."""
    args = tr.get_args(RECIPE.split())
    fm = [int(args.nfm * args.nfmm ** i) for i in range(args.num_blocks)]
    enc = tr.EncodeNet(len(args.algorithms) + 1, fm, 2, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    dec = tr.DecodeNet(enc.channels, 2, 1, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    found, hooks = [], []
    for net in (enc, dec):
        for m in net.modules():
            if isinstance(m, tr.ConvBlock) and not m.transpose:
                rec = {"mod": m}
                found.append(rec)
                hooks.append(m.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("x", tuple(a[0].shape))))
                hooks.append(m.ab.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("conv_in", tuple(a[0].shape))))
                hooks.append(m.register_forward_hook(lambda mod, a, out, rec=rec: rec.__setitem__("out", tuple(out.shape))))
    with torch.no_grad():
        skips = enc(torch.rand((args.batch_size, len(args.algorithms) + 1, 128, 128), device=dev))
        dec([s.chunk(2, dim=1)[0].repeat(NS, 1, 1, 1) for s in skips])
    for h in hooks:
        h.remove()
    g = torch.Generator(device=dev).manual_seed(5)
    blocks = []
    for i, rec in enumerate(found):
        (H, W), (PH, PW) = rec["x"][2:], rec["conv_in"][2:]
        p = (PW - W, PH - H)
        m = rec["mod"]
        blocks.append(dict(x=torch.randn(rec["x"], device=dev, generator=g).requires_grad_(i > 0),
                           w=m.ab.weight.detach().clone().requires_grad_(True), b=m.ab.bias.detach().clone().requires_grad_(True),
                           g=torch.randn(rec["out"], device=dev, generator=g), stride=m.stride,
                           pads=(p[0] // 2 + p[0] % 2, p[0] // 2, p[1] // 2 + p[1] % 2, p[1] // 2)))      # ConvBlock.forward's split
    return blocks


def run_blocks(blocks, version):
    """Every block's forward, then all their backwards in one pass."""
    torch.backends.cudnn.deterministic = version == "torch deterministic"
    outs = []
    for b in blocks:
        b["x"].grad = b["w"].grad = b["b"].grad = None
        if version == "fused":
            outs.append(cp.periodic_conv_maxout(b["x"], b["w"], b["b"], b["stride"], b["pads"]))
        else:
            y = torch.nn.functional.conv2d(tr._PeriodicPad.apply(b["x"], b["pads"]), b["w"], b["b"], stride=b["stride"])
            outs.append(tr._Maxout.apply(y))
    torch.autograd.backward(outs, [b["g"] for b in blocks])


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls, a.elapsed_time(b) / calls


def count_launches(fn):
    """Device kernels and copies of one call, from torch.profiler's device-side events."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def measure(blocks, calls=20, windows=5):
    fns = {v: (lambda v=v: run_blocks(blocks, v)) for v in VERSIONS}
    res = {v: [] for v in VERSIONS}
    for f in fns.values():
        window(f, calls)
    for _ in range(windows):
        for v, f in fns.items():
            res[v].append(window(f, calls))
    return {v: np.array(r).T for v, r in res.items()}, fns


def block_rows(dev):
    blocks = padded_blocks(dev)
    rows = []
    was = torch.backends.cudnn.deterministic
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for i, b in enumerate(blocks):
                res, _ = measure([b])
                N, Cin, H, W = b["x"].shape
                what = f"block {i:2d} {N}x{Cin}x{H}x{W} -> {b['w'].shape[0] // 2} k{b['w'].shape[2]} s{b['stride']}"
                for v, (host, gpu) in res.items():
                    rows.append(f"{what:36s} {v:20s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                                f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})")
                med = {v: np.median(r[1]) for v, r in res.items()}
                rows.append(f"#   gpu ms, fused against torch default {med['torch default'] / med['fused']:.2f}x, against torch deterministic "
                            f"{med['torch deterministic'] / med['fused']:.2f}x (above 1: the fused operation is the faster)")
            res, fns = measure(blocks)
            launches = {v: count_launches(f) for v, f in fns.items()}
            for v, (host, gpu) in res.items():
                rows.append(f"{'all ' + str(len(blocks)) + ' padded blocks fwd+bwd':36s} {v:20s} {np.median(host):8.4f} ({host.min():.4f} .. "
                            f"{host.max():.4f})   {np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})   {launches[v]:4d} device "
                            f"launches per call")
    finally:
        torch.backends.cudnn.deterministic = was
    return rows


def trainer_rows(dev, steps, windows=3):
    flags = [BASE + " --reproducible", BASE + " --reproducible --fused_conv", BASE, BASE + " --fused_conv"]
    was = torch.backends.cudnn.deterministic
    try:
        ts = {f: tr.PVAETrainer(tr.get_args((RECIPE + f).split()), dev) for f in flags}
        rate = {f: [] for f in flags}

        def run(f, n):
            torch.backends.cudnn.deterministic = "--reproducible" in f          # (a trainer sets it once, for its process)
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
    finally:
        torch.backends.cudnn.deterministic = was
    rows = [f"# trainer c3, every row with{BASE}"]
    rows += [f"trainer c3 ({steps} steps / window)  {(f[len(BASE):].strip() or 'neither flag'):30s} {np.median(v):8.1f} steps/s ({min(v):.1f} .. "
             f"{max(v):.1f})   {1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    med = {f: np.median(v) for f, v in rate.items()}
    apart = min(rate[flags[1]]) > max(rate[flags[0]]) or max(rate[flags[1]]) < min(rate[flags[0]])
    rows.append(f"#   steps/s with --fused_conv against without: {med[flags[1]] / med[flags[0]]:.3f}x under --reproducible (the windows "
                f"{'do not overlap' if apart else 'overlap'}), {med[flags[3]] / med[flags[2]]:.3f}x against the non-deterministic default")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "conv_timing.txt"))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_conv.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_conv.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over alternating windows",
             "# what                                 version                ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += block_rows(dev)
    lines += trainer_rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
