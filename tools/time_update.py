"""The update stage of a training step: the trainer's chain of torch calls (nan_to_num_, _foreach_norm, stack / divide / clamp_, unbind,
_foreach_mul_, p.grad pointed at the bucket, torch.optim.Adam(fused=True).step()) against FusedUpdate.step (ct_pvae_amd/update.py,
csrc/update.hip: two launches), on the parameter list of the c3 recipe (README: -b 5 --ns 2 --api 20, 128 x 128, --nb 3), and the
trainer's steps per second with and without --fused_update.

    python tools/time_update.py [--out profiles/update_timing.txt] [--steps 200]

Update rows: both versions own a copy of the c3 networks' parameters (an EncodeNet and a DecodeNet built as the trainer builds them)
and a FlatGradBucket filled once with normal draws; a call is one update from that bucket (the chain scales its bucket in place, as in
the trainer).  "ms" is the median (min .. max) of 3 windows of 200 calls each after a warm-up window, from a host clock around work that
ends in a device synchronise -- what a host-bound training step pays; "gpu ms" is the same windows from HIP events.  The two versions
alternate window by window.  Launch rows: device kernels per call, counted by torch.profiler.  Trainer rows: 3 alternating windows of
--steps steps each after 30 warm-up steps, median steps per second, for the plain recipe and on top of --fused_head --fused_latents
--fused_blocks.  A line says so if two windows overlap or the pair does not beat the chain."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import sharding, trainer as tr  # noqa: E402

RECIPE = "--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --pnm_start 1e3 --random --normal -i 1000 --train"


def c3_parameters(dev):
    args = tr.get_args(RECIPE.split())
    fm = [int(args.nfm * args.nfmm ** i) for i in range(args.num_blocks)]
    enc = tr.EncodeNet(len(args.algorithms) + 1, fm, 2, args.kernel_size, args.stride_encode, args.il, args.ik).to(dev)
    dec = tr.DecodeNet(enc.channels, 2, 1, args.kernel_size, args.stride_encode, args.il, args.ik, first_layer=enc.num_layers).to(dev)
    return list(enc.parameters()) + list(dec.parameters()), args


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
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def overlap(a, b):
    return min(a) <= max(b) and min(b) <= max(a)


def update_rows(dev, calls=200, windows=3):
    params_a, args = c3_parameters(dev)
    params_b = [torch.nn.Parameter(p.detach().clone()) for p in params_a]
    g = torch.Generator(device=dev).manual_seed(5)
    grads = [torch.randn(p.shape, device=dev, generator=g) * 1e-2 for p in params_a]
    bucket_a, bucket_b = sharding.FlatGradBucket(grads).fill(grads), sharding.FlatGradBucket(grads).fill(grads)
    opt = torch.optim.Adam(params_a, lr=args.lr, eps=args.adam_epsilon, fused=True)
    fu = cp.FusedUpdate(params_b, lr=args.lr, eps=args.adam_epsilon, clip_norm=args.norm)

    def chain():                                   # trainer._loss_and_update, from nan_to_num_ to self.opt.step()
        torch.nan_to_num_(bucket_a.flat, nan=0.0)
        norms = torch.stack(torch._foreach_norm(bucket_a.views))
        scales = (args.norm / norms).clamp_(max=1.0)
        torch._foreach_mul_(bucket_a.views, list(scales.unbind()))
        bucket_a.attach(params_a)
        opt.step()

    def pair():
        fu.step(bucket_b.flat)
    fns = {"torch chain": chain, "fused pair": pair}
    res = {k: [] for k in fns}
    for f in fns.values():
        window(f, calls)
    for _ in range(windows):
        for k, f in fns.items():
            res[k].append(window(f, calls))
    launches = {k: count_launches(f) for k, f in fns.items()}
    rows = [f"# c3 parameter list: {len(params_a)} tensors, {bucket_a.flat.numel()} elements, {fu._partials.numel()} chunks of at most "
            f"{cp.update.chunk_len()}"]
    for k, v in res.items():
        host, gpu = np.array(v).T
        rows.append(f"one update, c3 parameters  {k:11s} {np.median(host):8.4f} ({host.min():.4f} .. {host.max():.4f})   "
                    f"{np.median(gpu):8.4f} ({gpu.min():.4f} .. {gpu.max():.4f})   {launches[k]:4d} device launches per call")
    ch, pr = np.array(res["torch chain"]), np.array(res["fused pair"])
    rows.append(f"#   torch chain / fused pair = {np.median(ch[:, 0]) / np.median(pr[:, 0]):.2f}x host clock, "
                f"{np.median(ch[:, 1]) / np.median(pr[:, 1]):.2f}x HIP events, {launches['torch chain'] - launches['fused pair']} launches fewer")
    if overlap(ch[:, 0], pr[:, 0]):
        rows.append("#   the host-clock windows of the two OVERLAP")
    if np.median(pr[:, 0]) >= np.median(ch[:, 0]):
        rows.append("#   the fused pair does NOT beat the torch chain here")
    return rows


def trainer_rows(dev, steps, windows=3):
    base = ["", " --fused_head --fused_latents --fused_blocks"]
    flags = [b + u for b in base for u in ("", " --fused_update")]
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
    rows = [f"trainer c3 ({steps} steps / window)  {(f.strip() or 'no flag'):60s} {np.median(v):8.1f} steps/s ({min(v):.1f} .. {max(v):.1f})   "
            f"{1e3 / np.median(v):.3f} ms/step" for f, v in rate.items()]
    for b in base:
        off, on = rate[b], rate[b + " --fused_update"]
        rows.append(f"#   --fused_update on top of [{b.strip() or 'no flag'}]: {np.median(on) / np.median(off):.3f}x steps/s"
                    + ("; the windows OVERLAP" if overlap(off, on) else "; no window overlaps")
                    + ("; NOT faster" if np.median(on) <= np.median(off) else ""))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "update_timing.txt"))
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_update.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_update.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over 3 alternating windows",
             "# what                                    ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    lines += update_rows(dev)
    lines += trainer_rows(dev, args.steps)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
