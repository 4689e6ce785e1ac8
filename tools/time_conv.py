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
import numpy as np
import torch

import _conv_timing as ct      # (first: it puts the repository on sys.path)
import ct_pvae_amd as cp
from _conv_timing import BASE, measure, tr


def padded_blocks(dev):
    """The 16 padded blocks in the order they run, encoder first: dict(x, w, b, g, stride, pads, first) on the device."""
    args, enc, dec = ct.c3_networks(dev)
    found, hooks = [], []
    for net in (enc, dec):
        for m in net.modules():
            if isinstance(m, tr.ConvBlock) and not m.transpose:
                rec = {"mod": m}
                found.append(rec)
                hooks.append(m.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("x", tuple(a[0].shape))))
                hooks.append(m.ab.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("conv_in", tuple(a[0].shape))))
                hooks.append(m.register_forward_hook(lambda mod, a, out, rec=rec: rec.__setitem__("out", tuple(out.shape))))
    ct.run_networks(args, enc, dec, dev)
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


def block_rows(dev):
    blocks = padded_blocks(dev)
    rows = []
    was = torch.backends.cudnn.deterministic
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for i, b in enumerate(blocks):
                res, _ = measure(run_blocks, [b])
                N, Cin, H, W = b["x"].shape
                what = f"block {i:2d} {N}x{Cin}x{H}x{W} -> {b['w'].shape[0] // 2} k{b['w'].shape[2]} s{b['stride']}"
                for v, (host, gpu) in res.items():
                    rows.append(ct.timing_row(what, v, host, gpu))
                med = {v: np.median(r[1]) for v, r in res.items()}
                rows.append(f"#   gpu ms, fused against torch default {med['torch default'] / med['fused']:.2f}x, against torch deterministic "
                            f"{med['torch deterministic'] / med['fused']:.2f}x (above 1: the fused operation is the faster)")
            res, fns = measure(run_blocks, blocks)
            launches = {v: ct.count_launches(f) for v, f in fns.items()}
            for v, (host, gpu) in res.items():
                rows.append(ct.timing_row(f"all {len(blocks)} padded blocks fwd+bwd", v, host, gpu) + f"   {launches[v]:4d} device launches per call")
    finally:
        torch.backends.cudnn.deterministic = was
    return rows


def trainer_rows(dev, steps):
    flags = [BASE + " --reproducible", BASE + " --reproducible --fused_conv", BASE, BASE + " --fused_conv"]
    rate, rows = ct.trainer_rates(dev, flags, steps)
    med = {f: np.median(v) for f, v in rate.items()}
    apart = not ct.overlap(rate[flags[1]], rate[flags[0]])
    rows.append(f"#   steps/s with --fused_conv against without: {med[flags[1]] / med[flags[0]]:.3f}x under --reproducible (the windows "
                f"{'do not overlap' if apart else 'overlap'}), {med[flags[3]] / med[flags[2]]:.3f}x against the non-deterministic default")
    return rows


if __name__ == "__main__":
    ct.main("time_conv.py", "conv_timing.txt", lambda dev, steps: block_rows(dev) + trainer_rows(dev, steps))
