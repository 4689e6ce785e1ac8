"""Forward + backward of the glue around the convolutions of the c3 networks' 19 ConvBlocks -- the periodic pad in front of 16 of
them and the maxout behind all 19 -- as the trainer's chains of torch operations (trainer._PeriodicPad, trainer._Maxout) against the
fused launches (ct_pvae_amd.periodic_pad / maxout, csrc/convblock.hip), the number of device launches of both, and the trainer's
steps per second with and without --fused_blocks at the c3 recipe (README: -b 5 --ns 2 --api 20, 128 x 128, --nb 3).

    python tools/time_convblock.py [--out profiles/convblock_timing.txt] [--steps 200]

Glue rows: the shapes are read with forward hooks from an EncodeNet (B = 5) and a DecodeNet (ns * B = 10) built as the trainer builds
them; both versions get the same inputs (requires_grad, but for the first encoder block's, which is data in the trainer too) and the
same cotangents, no convolution runs, and everything is inside torch.autograd.set_multithreading_enabled(False) as the trainer's
backward is.  "ms" is the median (min .. max) of 7 windows of 50 calls each after a warm-up window, from a host clock around work
that ends in a device synchronise -- what a host-bound training step pays; "gpu ms" is the same windows from HIP events.  The two
versions alternate window by window.  Launch rows: device kernels per call, counted by torch.profiler.  Trainer rows: 3 alternating
windows of --steps steps each after 30 warm-up steps, median steps per second; the baseline is this commit with the flag off, in
the same process and the same windows.  The header names the device as torch reports it, with its gfx architecture."""
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
NS = 2


def block_shapes(dev):
    """[(input shape, pads or None, convolution output shape)] of the 19 blocks, encoder first, in the order they run."""
    args = tr.get_args(RECIPE.split())
    fm = [int(args.nfm * args.nfmm ** i) for i in range(args.num_blocks)]
    enc = tr.EncodeNet(len(args.algorithms) + 1, fm, 2, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    dec = tr.DecodeNet(enc.channels, 2, 1, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    found, hooks = [], []
    for net in (enc, dec):
        for m in net.modules():
            if isinstance(m, tr.ConvBlock):
                rec = {"transpose": m.transpose}
                found.append(rec)
                hooks.append(m.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("x", tuple(a[0].shape))))
                hooks.append(m.ab.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("conv_in", tuple(a[0].shape))))
                hooks.append(m.ab.register_forward_hook(lambda mod, a, out, rec=rec: rec.__setitem__("y", tuple(out.shape))))
    with torch.no_grad():
        skips = enc(torch.rand((args.batch_size, len(args.algorithms) + 1, 128, 128), device=dev))
        dec([s.chunk(2, dim=1)[0].repeat(NS, 1, 1, 1) for s in skips])
    for h in hooks:
        h.remove()
    out = []
    for rec in found:
        (H, W), (PH, PW) = rec["x"][2:], rec["conv_in"][2:]
        p = (PW - W, PH - H)
        pads = None if rec["transpose"] else (p[0] // 2 + p[0] % 2, p[0] // 2, p[1] // 2 + p[1] % 2, p[1] // 2)     # ConvBlock.forward's split
        out.append((rec["x"], pads, rec["y"]))
    return out


def glue(blocks, fused):
    """Every block's pad and maxout, forward, then all their backwards in one pass."""
    pad = cp.periodic_pad if fused else tr._PeriodicPad.apply
    mo = cp.maxout if fused else tr._Maxout.apply
    outs, cots = [], []
    for b in blocks:
        if b["pads"] is not None:
            o = pad(b["x"], b["pads"])
            if o.requires_grad:
                outs.append(o), cots.append(b["g_pad"])
        outs.append(mo(b["y"])), cots.append(b["g_out"])
    torch.autograd.backward(outs, cots)


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


def glue_rows(dev, calls=50, windows=7):
    shapes = block_shapes(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    blocks = []
    for k, (xs, pads, ys) in enumerate(shapes):
        b = dict(pads=pads, x=torch.randn(xs, device=dev, generator=g).requires_grad_(k > 0),
                 y=torch.randn(ys, device=dev, generator=g).requires_grad_(True),
                 g_out=torch.randn((ys[0], ys[1] // 2) + ys[2:], device=dev, generator=g))
        if pads is not None:
            b["g_pad"] = torch.randn(xs[:2] + (xs[2] + pads[2] + pads[3], xs[3] + pads[0] + pads[1]), device=dev, generator=g)
        blocks.append(b)

    def clear():
        for b in blocks:
            b["x"].grad = b["y"].grad = None
    fns = {"torch ops": lambda i: (clear(), glue(blocks, False)), "fused pairs": lambda i: (clear(), glue(blocks, True))}
    res = {k: [] for k in fns}
    padded = sum(1 for s in shapes if s[1] is not None)
    rows = [f"# {len(shapes)} blocks, {padded} of them padded; inputs [N][C][H][W] from {'x'.join(map(str, shapes[0][0]))} to "
            f"{'x'.join(map(str, min((s[0] for s in shapes), key=lambda s: s[2] * s[3])))}, convolution outputs up to "
            f"{'x'.join(map(str, max((s[2] for s in shapes), key=lambda s: s[0] * s[1] * s[2] * s[3])))}"]
    with torch.autograd.set_multithreading_enabled(False):
        for k, f in fns.items():
            window(f, calls)
        for _ in range(windows):
            for k, f in fns.items():
                res[k].append(window(f, calls))
        launches = {k: count_launches(f) for k, f in fns.items()}
    for k, v in res.items():
        host, gpu = np.array(v).T
        rows.append(f"pad + maxout fwd+bwd, {len(shapes)} blocks  {k:11s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                    f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})   {launches[k]:4d} device launches per call")
    rows.append(f"#   torch ops / fused pairs = {np.median(np.array(res['torch ops'])[:, 0]) / np.median(np.array(res['fused pairs'])[:, 0]):.2f}x "
                f"host clock, {np.median(np.array(res['torch ops'])[:, 1]) / np.median(np.array(res['fused pairs'])[:, 1]):.2f}x HIP events, "
                f"{launches['torch ops'] - launches['fused pairs']} launches fewer")
    return rows


def trainer_rows(dev, steps, windows=3):
    flags = [" --fused_head --fused_latents", " --fused_head --fused_latents --fused_blocks", "", " --fused_blocks"]
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
    rows = [f"trainer c3 ({steps} steps / window)  {(f.strip() or 'neither flag'):45s} {np.median(v):8.1f} steps/s ({min(v):.1f} .. {max(v):.1f})   "
            f"{1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    med = {f: np.median(v) for f, v in rate.items()}
    rows.append(f"#   steps/s with --fused_blocks against without: {med[flags[1]] / med[flags[0]]:.3f}x on top of --fused_head --fused_latents, "
                f"{med[flags[3]] / med[flags[2]]:.3f}x alone")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "convblock_timing.txt"))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_convblock.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_convblock.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over alternating windows",
             "# what                                         ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += glue_rows(dev)
    lines += trainer_rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
