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
import argparse
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import trainer as tr  # noqa: E402

RECIPE = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random --normal -i 1000 --train"
BASE = " --fused_head --fused_latents --fused_blocks --fused_update"
NS = 2
VERSIONS = ("fused", "torch default", "torch deterministic")


def transposed_blocks(dev):
    """The 3 transposed blocks in the order they run: dict(x, w, b, g, stride, pad, opad) on the device."""
    args = tr.get_args(RECIPE.split())
    fm = [int(args.nfm * args.nfmm ** i) for i in range(args.num_blocks)]
    enc = tr.EncodeNet(len(args.algorithms) + 1, fm, 2, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    dec = tr.DecodeNet(enc.channels, 2, 1, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    found, hooks = [], []
    for m in dec.modules():
        if isinstance(m, tr.ConvBlock) and m.transpose:
            rec = {"mod": m}
            found.append(rec)
            hooks.append(m.register_forward_pre_hook(lambda mod, a, rec=rec: rec.__setitem__("x", tuple(a[0].shape))))
            hooks.append(m.register_forward_hook(lambda mod, a, out, rec=rec: rec.__setitem__("out", tuple(out.shape))))
    with torch.no_grad():
        skips = enc(torch.rand((args.batch_size, len(args.algorithms) + 1, 128, 128), device=dev))
        dec([s.chunk(2, dim=1)[0].repeat(NS, 1, 1, 1) for s in skips])
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


def overlap(a, b):
    return not (min(a) > max(b) or max(a) < min(b))


def block_rows(dev):
    blocks = transposed_blocks(dev)
    rows = []
    was = torch.backends.cudnn.deterministic
    try:
        with torch.autograd.set_multithreading_enabled(False):
            for i, b in enumerate(blocks + [None]):
                res, fns = measure([b] if b is not None else blocks)
                launches = {v: count_launches(f) for v, f in fns.items()}
                if b is not None:
                    N, Cin, H, W = b["x"].shape
                    what = f"block {i} {N}x{Cin}x{H}x{W} -> {b['w'].shape[1] // 2} k{b['w'].shape[2]} s{b['stride']}"
                else:
                    what = f"all {len(blocks)} transposed blocks fwd+bwd"
                for v, (host, gpu) in res.items():
                    rows.append(f"{what:36s} {v:20s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                                f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})   {launches[v]:4d} device launches per call")
                med = {v: np.median(r[1]) for v, r in res.items()}
                notes = [f"{v} {med[v] / med['fused']:.2f}x ({'the windows overlap' if overlap(res[v][1], res['fused'][1]) else 'no overlap'})"
                         for v in VERSIONS[1:]]
                rows.append(f"#   gpu ms of the torch chain over the fused operation's: {', '.join(notes)} (above 1: the fused operation is "
                            f"the faster)")
    finally:
        torch.backends.cudnn.deterministic = was
    return rows


def trainer_rows(dev, steps, windows=3):
    flags = [BASE + " --fused_conv --fused_convt", BASE + " --reproducible --fused_conv", BASE]
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
    rows.append(f"#   steps/s with --fused_conv --fused_convt against --reproducible --fused_conv: {med[flags[0]] / med[flags[1]]:.3f}x (the "
                f"windows {'overlap: not measurable' if overlap(rate[flags[0]], rate[flags[1]]) else 'do not overlap'}), against neither "
                f"flag {med[flags[0]] / med[flags[2]]:.3f}x (the windows "
                f"{'overlap: not measurable' if overlap(rate[flags[0]], rate[flags[2]]) else 'do not overlap'})")
    return rows


def resource_rows():
    """Registers, LDS, scratch and occupancy of each kernel of csrc/conv_transpose.hip from the compiler's remarks."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["# kernel resources: no hipcc here"]
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "conv_transpose.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    if out.returncode != 0:
        return ["# kernel resources: the compile failed"]
    rows, rec = ["# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)"], None
    keys = (("VGPRs", r"\bVGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRs", r"\bSGPRs: (\d+)"), ("scratch B/lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("occupancy waves/SIMD", r"Occupancy \[waves/SIMD\]: (\d+)"), ("LDS B/block", r"LDS Size \[bytes/block\]: (\d+)"))
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            rec = [re.sub(r"^_ZN6ctpvae\d+|E?P[KfhiS_0-9A-Za-z]*$", "", m.group(1))]
            rows.append(rec)
        for label, pat in keys:
            m = re.search(pat, line)
            if m and rec is not None:
                rec.append(f"{label} {m.group(1)}")
    return [r if isinstance(r, str) else f"{r[0]:28s} " + ", ".join(r[1:]) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_transpose_timing.txt"))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_conv_transpose.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_conv_transpose.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over alternating windows",
             "# what                                 version                ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += block_rows(dev)
    lines += trainer_rows(dev, args.steps)
    lines += resource_rows()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
