"""Developer tool: the bilinear forward, precision="exact" against precision="fast", one process on one box, alternating.

HIP-event pairs around graph-replayed launches (time_modes.graph_time: the median of five replays of one graph of n launches is ONE
run), at least five alternated runs per shape and leg, every run printed, then min / median / max per leg:
    (a) 50 x 128^2 x 20 angles   (b) 50 x 128^2 x 180   (c) 32 x 512^2 x 90 (tiles + the reduce pass)   (d) 5 x 128^2 x 20

    python tools/ab_bilin_fast.py [--runs 5] [BxNxA ...]
    CTPVAE_VARIANT_LIB=tools/libctpvae_radon_<tag>.bin python tools/ab_bilin_fast.py --exact-only
the second form times the exact leg alone on another build of the library (an older one, without the fast entry points: the same C
ABI otherwise) -- run it on the same box, next to the first, for "did the exact kernel move".  The fast and exact results of the
first form are compared (max |fast - exact| / max |exact|) and must differ."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ct_pvae_amd import _lib, phantoms  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--exact-only", action="store_true")
ap.add_argument("shapes", nargs="*")
args = ap.parse_args()
if os.environ.get("CTPVAE_VARIANT_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["CTPVAE_VARIANT_LIB"])
    _lib.torch_node = lambda: None
    if args.exact_only:      # a build from before the fast entry points binds without them
        for name in ("ctpvae_rotate_fwd_fast_f32", "ctpvae_rotate_fwd_tiled_fast_f32"):
            _lib.SIGNATURES.pop(name, None)
from ct_pvae_amd.forward_functions import RotatePlan  # noqa: E402
from time_modes import graph_time  # noqa: E402

d = torch.device("cuda", 0)
shapes = [tuple(int(v) for v in a.split("x")) for a in args.shapes] or [(50, 128, 20), (50, 128, 180), (32, 512, 90), (5, 128, 20)]
print(f"library {_lib.LIB_PATH} on {torch.cuda.get_device_name(0)}; {args.runs} alternated runs per leg, us per launch", flush=True)
for B, N, A in shapes:
    dense = phantoms.dense_theta(180)
    theta = dense[phantoms.sparse_angle_indices(180, A)] if A < 180 and 180 % A == 0 else np.pi * np.arange(A) / A
    legs = {"exact": RotatePlan(theta, N, N, True, d, interp="bilinear")}
    if not args.exact_only:
        legs["fast"] = RotatePlan(theta, N, N, True, d, interp="bilinear", precision="fast")
    x = torch.randn((B, N, N), device=d)
    outs = {k: torch.full((B, A, p.PW), float("nan"), device=d) for k, p in legs.items()}
    n = 20 if N >= 256 else 100
    for k, p in legs.items():                    # warm-up: first launches, workspaces, clocks
        graph_time(lambda: p.forward(x, out=outs[k]), n)
    times = {k: [] for k in legs}
    for run in range(args.runs):
        for k, p in legs.items():
            times[k].append(graph_time(lambda: p.forward(x, out=outs[k]), n) * 1e6)
        print(f"  B={B} N={N} A={A} run {run}: " + "  ".join(f"{k} {times[k][-1]:8.2f}" for k in legs), flush=True)
    line = f"B={B} N={N} A={A}: " + "  ".join(f"{k} min {min(t):.2f} median {np.median(t):.2f} max {max(t):.2f}" for k, t in times.items())
    if "fast" in legs:
        e, f = outs["exact"].double(), outs["fast"].double()
        rel = float((f - e).abs().max() / e.abs().max())
        line += f"  | every fast run below every exact run: {max(times['fast']) < min(times['exact'])}; rel diff {rel:.2e}, {'DIFFER' if rel > 0 else 'EQUAL BITS (flag not wired?)'}"
    print(line, flush=True)
