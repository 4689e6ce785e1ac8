"""Forward + backward of the 3 transposed ConvBlocks of the c3 decoder -- transposed convolution, maxout -- as the fused operation
(ct_pvae_amd.conv_transpose_maxout, csrc/conv_transpose.hip) against the trainer's torch chain (torch's transposed convolution,
trainer._Maxout) with the library's default algorithms and with torch.backends.cudnn.deterministic; the device launches of each; the
trainer's steps per second at the c3 recipe (README: -b 5 --ns 2 --api 20, 128 x 128, --nb 3) on top of --fused_head --fused_latents
--fused_blocks --fused_update with --fused_conv --fused_convt, with --reproducible --fused_conv and with neither flag; and the
kernels' registers and occupancy as the compiler reports them.

    python tools/time_conv_transpose.py [--out profiles/conv_transpose_timing.txt] [--steps 200]

Block rows: the shapes are read with forward hooks from a DecodeNet (ns * B = 10) built as the trainer builds it; the three versions
get the same inputs (requires_grad), the same parameters and the same cotangents, inside
torch.autograd.set_multithreading_enabled(False) as the trainer's backward is.  "ms" is the median (min .. max) of 5 windows of 20
calls each after a warm-up window, from a host clock around work that ends in a device synchronise; "gpu ms" is the same windows
from HIP events.  The versions alternate window by window.  Launch rows: device kernels per call, counted by torch.profiler.  Trainer
rows: 3 alternating windows of --steps steps each after 30 warm-up steps, median steps per second, all in the same process and the
same windows; torch's deterministic switch is set per window to what the run's --reproducible asks.  Resource rows: hipcc's
-Rpass-analysis=kernel-resource-usage remarks for csrc/conv_transpose.hip with the Makefile's flags.  The header names the device as
torch reports it, with its gfx architecture."""
import numpy as np
import torch

import _conv_timing as ct      # (first: it puts the repository on sys.path)
import ct_pvae_amd as cp
from _conv_timing import BASE, VERSIONS, measure, overlap, tr


def transposed_blocks(dev):
    """The 3 transposed blocks in the order they run: dict(x, w, b, g, stride, pad, opad) on the device."""
    args, enc, dec = ct.c3_networks(dev)
    found, hooks = [], []
    for m in dec.modules():
        if isinstance(m, tr.ConvBlock) and m.transpose:
            rec = {"mod": m}
            found.append(rec)
            hooks.append(m.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("x", tuple(a[0].shape))))
            hooks.append(m.register_forward_hook(lambda mod, a, out, rec=rec: rec.__setitem__("out", tuple(out.shape))))
    ct.run_networks(args, enc, dec, dev)
    for h in hooks:
        h.remove()
    g = torch.Generator(device=dev).manual_seed(5)
    blocks = []
    for rec in found:
        m = rec["mod"]
        blocks.append(dict(x=torch.randn(rec["x"], device=dev, generator=g).requires_grad_(True),
                           w=m.ab.weight.detach().clone().requires_grad_(True), b=m.ab.bias.detach().clone().requires_grad_(True),
                           g=torch.randn(rec["out"], device=dev, generator=g), stride=m.ab.stride[0], pad=m.ab.padding[0],
                           opad=m.ab.output_padding[0]))
    return blocks


def run_blocks(blocks, version):
    """Every block's forward, then all their backwards in one pass."""
    torch.backends.cudnn.deterministic = version == "torch deterministic"
    outs = []
    for b in blocks:
        b["x"].grad = b["w"].grad = b["b"].grad = None
        if version == "fused":
            outs.append(cp.conv_transpose_maxout(b["x"], b["w"], b["b"], b["stride"], b["pad"], b["opad"]))
        else:
            y = torch.nn.functional.conv_transpose2d(b["x"], b["w"], b["b"], stride=b["stride"], padding=b["pad"], output_padding=b["opad"])
            outs.append(tr._Maxout.apply(y))
    torch.autograd.backward(outs, [b["g"] for b in blocks])


def block_rows(dev):
    blocks = transposed_blocks(dev)
    rows = []
    was = torch.backends.cudnn.deterministic
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for i, b in enumerate(blocks + [None]):
                res, fns = measure(run_blocks, [b] if b is not None else blocks)
                launches = {v: ct.count_launches(f) for v, f in fns.items()}
                if b is not None:
                    N, Cin, H, W = b["x"].shape
                    what = f"block {i} {N}x{Cin}x{H}x{W} -> {b['w'].shape[1] // 2} k{b['w'].shape[2]} s{b['stride']}"
                else:
                    what = f"all {len(blocks)} transposed blocks fwd+bwd"
                for v, (host, gpu) in res.items():
                    rows.append(ct.timing_row(what, v, host, gpu) + f"   {launches[v]:4d} device launches per call")
                med = {v: np.median(r[1]) for v, r in res.items()}
                notes = [f"{v} {med[v] / med['fused']:.2f}x ({'the windows overlap' if overlap(res[v][1], res['fused'][1]) else 'no overlap'})"
                         for v in VERSIONS[1:]]
                rows.append(f"#   gpu ms of the torch chain over the fused operation's: {', '.join(notes)} (above 1: the fused operation is "
                            f"the faster)")
    finally:
        torch.backends.cudnn.deterministic = was
    return rows


def trainer_rows(dev, steps):
    flags = [BASE + " --fused_conv --fused_convt", BASE + " --reproducible --fused_conv", BASE]
    rate, rows = ct.trainer_rates(dev, flags, steps)
    med = {f: np.median(v) for f, v in rate.items()}
    rows.append(f"#   steps/s with --fused_conv --fused_convt against --reproducible --fused_conv: {med[flags[0]] / med[flags[1]]:.3f}x (the "
                f"windows {'overlap: not measurable' if overlap(rate[flags[0]], rate[flags[1]]) else 'do not overlap'}), against neither "
                f"flag {med[flags[0]] / med[flags[2]]:.3f}x (the windows "
                f"{'overlap: not measurable' if overlap(rate[flags[0]], rate[flags[2]]) else 'do not overlap'})")
    return rows


if __name__ == "__main__":
    ct.main("time_conv_transpose.py", "conv_transpose_timing.txt",
            lambda dev, steps: block_rows(dev) + trainer_rows(dev, steps) + ct.resource_rows("conv_transpose.hip"))
