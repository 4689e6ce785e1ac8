"""What tools/time_conv.py and tools/time_conv_transpose.py share: the recipe, the timed window, the launch count, the alternating
measurement of the three versions of a list of blocks, the alternating trainer windows, the compiler's resource remarks of a kernel
file and the write-out.  The tools' docstrings say what the numbers mean."""
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
from ct_pvae_amd import trainer as tr  # noqa: E402

RECIPE = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random --normal -i 1000 --train"
BASE = " --fused_head --fused_latents --fused_blocks --fused_update"
NS = 2
VERSIONS = ("fused", "torch default", "torch deterministic")


def c3_networks(dev):
    """(args, EncodeNet, DecodeNet) of the recipe, built as the trainer builds them."""
    args = tr.get_args(RECIPE.split())
    fm = [int(args.nfm * args.nfmm ** i) for i in range(args.num_blocks)]
    enc = tr.EncodeNet(len(args.algorithms) + 1, fm, 2, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    dec = tr.DecodeNet(enc.channels, 2, 1, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    return args, enc, dec


def run_networks(args, enc, dec, dev):
    """One forward of both networks on random data (B objects into the encoder, ns * B into the decoder), for hooks to read shapes."""
    with torch.no_grad():
        skips = enc(torch.rand((args.batch_size, len(args.algorithms) + 1, 128, 128), device=dev))
        dec([s.chunk(2, dim=1)[0].repeat(NS, 1, 1, 1) for s in skips])


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


def overlap(a, b):
    return not (min(a) > max(b) or max(a) < min(b))


def measure(run_blocks, blocks, calls=20, windows=5):
    """{version: array [2][windows] of (host ms, gpu ms) per call} of run_blocks(blocks, version), the versions alternating window by
    window after a warm-up window each, and the {version: callable} that was timed."""
    fns = {v: (lambda v=v: run_blocks(blocks, v)) for v in VERSIONS}
    res = {v: [] for v in VERSIONS}
    for f in fns.values():
        window(f, calls)
    for _ in range(windows):
        for v, f in fns.items():
            res[v].append(window(f, calls))
    return {v: np.array(r).T for v, r in res.items()}, fns


def timing_row(what, version, host, gpu):
    return (f"{what:36s} {version:20s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
            f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})")


def trainer_rates(dev, flags, steps, windows=3):
    """({flags: [steps per second of each window]}, the rows that print them): one trainer per flag set, 30 warm-up steps each, then
    `windows` alternating windows of `steps` steps; torch's deterministic switch is set per window."""
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
    return rate, rows


def resource_rows(hip_file):
    """Registers, LDS, scratch and occupancy of each kernel of csrc/<hip_file> from the compiler's remarks."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return ["# kernel resources: no hipcc here"]
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", hip_file, "-o", os.devnull],
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


def main(tool, default_out, rows):
    """Parse --out and --steps, require the GPU, print the header and rows(dev, steps), and write them to --out."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", default_out))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"tools/{tool} measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/{tool} on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over alternating windows",
             "# what                                 version                ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
