"""Developer tool: what the few-angle (SHORT) planned adjoint's gather phase costs, on ONE box, in the form of tools/ab_wt_stores.py.

    python tools/ab_bwd_short_gather.py                                                      (the in-tree library)
    CTPVAE_VARIANT_LIB=tools/libctpvae_radon_<tag>.bin python tools/ab_bwd_short_gather.py   (another build)
    python tools/ab_bwd_short_gather.py --summarise log [log ...]                            (the table of alternated runs)

Rows (128 x 128 padded): the adjoint alone at B = 1, 5, 50, 400 x 20 angles, B = 1 and 50 x 32 and x 16 angles; the forward + adjoint pair at
B = 50 x 20 (the benchmark's step); the no-change rows -- the forward alone at B = 50 x 20, the adjoint at B = 50 x 180 angles (the
general form), the training call's subset backward (S = 10, 20 of 180 angles: rotate_bwd_planned_sel_kernel).
Each figure: the median of five HIP-graph replays of N launches between two events, after three untimed replays; `spread` is the
largest minus the smallest of the five.  One process prints one `AB` line per row; run parent and change alternately, each process under
its own time limit, and give all the logs to --summarise: per row every process's figure, diff = median of the parent's figures - median
of the change's, P-spread = largest - smallest of the parent's, ratio = diff / P-spread, all-below = every figure of the change below
every figure of the parent."""
import os
import re
import sys

import numpy as np


def summarise(paths):
    rows, order = {}, []
    for path in paths:
        for line in open(path):
            m = re.match(r"AB tag=(\S+) row=(\S+) kernel=(\S+) median=(\S+) spread=(\S+)", line)
            if m:
                if m.group(2) not in rows:
                    order.append(m.group(2))
                rows.setdefault(m.group(2), {}).setdefault(m.group(1), []).append(float(m.group(4)))
                rows[m.group(2)]["kernel"] = m.group(3)
    print("%-24s | %-36s | %-36s | diff  P-spread ratio all-below | kernel" % ("row", "parent runs", "change runs"))
    for row in order:
        p, c = rows[row].get("parent", []), rows[row].get("change", [])
        if not p or not c:
            continue
        diff, spread = float(np.median(p) - np.median(c)), max(p) - min(p)
        print("%-24s | %-36s | %-36s | %+.2f %.2f %5.1f %-3s | %s" % (row, " ".join("%.2f" % v for v in p), " ".join("%.2f" % v for v in c), diff,
                                                                   spread, diff / max(spread, 1e-9), "yes" if max(c) < min(p) else "no", rows[row]["kernel"]))


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2:])
    sys.exit(0)

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ct_pvae_amd import _lib

TAG = os.environ.get("CTPVAE_AB_TAG") or ("parent" if os.environ.get("CTPVAE_VARIANT_LIB") else "change")
if os.environ.get("CTPVAE_VARIANT_LIB"):
    import ctypes
    _lib.LIB_PATH = os.path.abspath(os.environ["CTPVAE_VARIANT_LIB"])
    _lib.torch_node = lambda: None      # the C++ autograd node binds the in-tree library: not used here
    _old = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(_old, k)}
from ct_pvae_amd import phantoms
from ct_pvae_amd.forward_functions import RotatePlan

d = torch.device("cuda", 0)


def timed(body, n):
    """(median, spread, the five runs) in microseconds per call of body"""
    body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            body()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / n)
    return float(np.median(runs)), float(max(runs) - min(runs)), runs


def report(row, kernel, t):
    print("AB tag=%s row=%s kernel=%s median=%.3f spread=%.3f runs=%s" % (TAG, row, kernel, t[0], t[1], ",".join("%.3f" % r for r in t[2])), flush=True)


def main():
    print("library:", _lib.LIB_PATH, flush=True)
    for B, A, what in ((1, 20, "adj"), (1, 32, "adj"), (1, 16, "adj"), (5, 20, "adj"), (50, 20, "adj fwd pair"), (400, 20, "adj"), (50, 32, "adj"), (50, 16, "adj"), (50, 180, "adj")):
        theta = phantoms.dense_theta(180)[np.arange(A) * 180 // A]
        plan = RotatePlan(theta, 128, 128, True, d)
        x = torch.rand((B, 128, 128), device=d)
        gs = torch.randn((B, A, plan.PW), device=d)
        out, gx = torch.empty_like(gs), torch.empty_like(x)
        n = 200 if B * A < 8000 else 50

        def pair():
            plan.forward(x, out=out)
            plan.backward(out, out=gx)
        for w in what.split():
            body = {"adj": lambda: plan.backward(gs, out=gx), "fwd": lambda: plan.forward(x, out=out), "pair": pair}[w]
            kernel = {"adj": plan.backward_kernel_name(B), "fwd": plan.forward_kernel_name(B), "pair": "both"}[w]
            report("B=%d_A=%d_%s" % (B, A, w), kernel, timed(body, n))
    dense = RotatePlan(phantoms.dense_theta(180), 128, 128, True, d)
    S = 10
    sub = torch.from_numpy(np.random.default_rng(0).permutation(180)[:20].astype(np.int32))
    dlp = torch.randn((S, 20, dense.PW), device=d)
    gx, w = torch.empty((S, 128, 128), device=d), torch.ones(S, device=d)
    report("training_S=10_20of180_adj", "rotate_bwd_planned_sel_kernel", timed(lambda: dense.backward(dlp, out=gx, scale=w, angles_i=sub), 200))


if __name__ == "__main__":
    main()
