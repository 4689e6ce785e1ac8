"""Forward + backward of the dropout in front of the c3 networks' 19 ConvBlocks -- with the periodic pad of the 16 blocks that have
one -- as torch.nn.functional.dropout followed by the existing fused pad (ct_pvae_amd.periodic_pad) against the Philox-keyed launches
(ct_pvae_amd.dropout_pad, and ct_pvae_amd.dropout for the three transposed blocks; csrc/convblock.hip), the number of device launches
of both, and the trainer's steps per second with --dp 0.1 against --dp 0 at the c3 recipe (README: -b 5 --ns 2 --api 20, 128 x 128,
--nb 3), both with --fused_head --fused_latents --fused_blocks.

    python tools/time_dropout.py [--out profiles/dropout_timing.txt] [--steps 200]

Dropout rows: the shapes are read with forward hooks from an EncodeNet (B = 5) and a DecodeNet (ns * B = 10) built as the trainer
builds them (tools/time_convblock.py's block_shapes); both versions get the same inputs (requires_grad, but for the first encoder
block's, which is data in the trainer too) and the same cotangents, no convolution runs, and everything is inside
torch.autograd.set_multithreading_enabled(False) as the trainer's backward is.  The torch chain keeps a mask tensor per block for its
backward and draws from the global generator; the keyed launches keep nothing.  "ms" is the median (min .. max) of 3 windows of 50
calls each after a warm-up window, from a host clock around work that ends in a device synchronise; "gpu ms" is the same windows from
HIP events.  The two versions alternate window by window.  Launch rows: device kernels per call, counted by torch.profiler.  Trainer
rows: 3 alternating windows of --steps steps each after 30 warm-up steps, median steps per second, in the same process and the same
windows.  The header names the device as torch reports it, with its gfx architecture."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import trainer as tr  # noqa: E402
from time_convblock import RECIPE, block_shapes, count_launches, window  # noqa: E402

RATE = 0.1
FUSED = " --fused_head --fused_latents --fused_blocks"


def drop(blocks, keyed, draw):
    """Every block's dropout (+ pad), forward, then all their backwards in one pass."""
    outs, cots = [], []
    for layer, b in enumerate(blocks):
        if keyed:
            key = dict(seed=1234, draw=draw, layer=layer, first_object=0)
            o = cp.dropout(b["x"], RATE, **key) if b["pads"] is None else cp.dropout_pad(b["x"], b["pads"], RATE, **key)
        else:
            o = F.dropout(b["x"], RATE, training=True)
            if b["pads"] is not None:
                o = cp.periodic_pad(o, b["pads"])
        if o.requires_grad:
            outs.append(o), cots.append(b["g"])
    torch.autograd.backward(outs, cots)


def dropout_rows(dev, calls=50, windows=3):
    shapes = block_shapes(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    blocks = []
    for k, (xs, pads, _) in enumerate(shapes):
        gs = xs if pads is None else xs[:2] + (xs[2] + pads[2] + pads[3], xs[3] + pads[0] + pads[1])
        blocks.append(dict(pads=pads, x=torch.randn(xs, device=dev, generator=g).requires_grad_(k > 0),
                           g=torch.randn(gs, device=dev, generator=g)))

    def clear():
        for b in blocks:
            b["x"].grad = None
    fns = {"F.dropout, pad": lambda i: (clear(), drop(blocks, False, i)), "keyed, fused": lambda i: (clear(), drop(blocks, True, i))}
    res = {k: [] for k in fns}
    padded = sum(1 for s in shapes if s[1] is not None)
    rows = [f"# {len(shapes)} blocks, {padded} of them padded, rate {RATE}; inputs [N][C][H][W] from {'x'.join(map(str, shapes[0][0]))} to "
            f"{'x'.join(map(str, min((s[0] for s in shapes), key=lambda s: s[2] * s[3])))}"]
    with torch.autograd.set_multithreading_enabled(False):
        for k, f in fns.items():
            window(f, calls)
        for _ in range(windows):
            for k, f in fns.items():
                res[k].append(window(f, calls))
        launches = {k: count_launches(f) for k, f in fns.items()}
    for k, v in res.items():
        host, gpu = np.array(v).T
        rows.append(f"dropout (+ pad) fwd+bwd, {len(shapes)} blocks  {k:15s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                    f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})   {launches[k]:4d} device launches per call")
    a, b = np.array(res["F.dropout, pad"]), np.array(res["keyed, fused"])
    rows.append(f"#   F.dropout, pad / keyed, fused = {np.median(a[:, 0]) / np.median(b[:, 0]):.2f}x host clock, "
                f"{np.median(a[:, 1]) / np.median(b[:, 1]):.2f}x HIP events, {launches['F.dropout, pad'] - launches['keyed, fused']} launches fewer")
    return rows


def trainer_rows(dev, steps, windows=3):
    flags = [FUSED + " --dp 0", FUSED + f" --dp {RATE}"]
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
    rows = [f"trainer c3 ({steps} steps / window)  {f.strip():55s} {np.median(v):8.1f} steps/s ({min(v):.1f} .. {max(v):.1f})   "
            f"{1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    med = {f: np.median(v) for f, v in rate.items()}
    rows.append(f"#   steps/s with --dp {RATE} against --dp 0: {med[flags[1]] / med[flags[0]]:.3f}x "
                f"({1e3 / med[flags[1]] - 1e3 / med[flags[0]]:+.3f} ms/step for 19 dropouts each way)")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dropout_timing.txt"))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_dropout.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_dropout.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over 3 alternating windows",
             "# what                                              ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += dropout_rows(dev)
    lines += trainer_rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
