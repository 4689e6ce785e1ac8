"""Developer tool: what the compact tail section of the tf_compat backward plan is worth to the few-angle (SHORT) planned adjoint, on
ONE box, with the timing of tools/ab_bwd_short_gather.py (median of five HIP-graph replays of N launches between two events).

    python tools/ab_bwd_tail.py                                                      (the in-tree library: tag `change`)
    CTPVAE_TUNE_BWD_TAIL=0 CTPVAE_AB_TAG=knob0 python tools/ab_bwd_tail.py            (the in-tree library reading the whole uint4)
    CTPVAE_VARIANT_LIB=tools/libctpvae_radon_<tag>.bin python tools/ab_bwd_tail.py   (another build: tag `parent`)
    python tools/ab_bwd_tail.py --summarise log [log ...]                            (change against parent, then against knob0)

Rows (128 x 128 padded): the adjoint alone at B = 1, 5, 25, 50 x 20 angles (records of one dword behind a full vector), B = 40 and 80 x 20
and x 32 (the cells whose tile height changed with the section: eleven waves), B = 50 x 8 (records
alone), x 24 and x 28 (records of two and three dwords), x 16 and x 32 (no section: the parent's requests), x 180 (the general form); the
forward alone and the forward + adjoint pair at B = 50 x 20 (the benchmark's step).  Run the three kinds of process alternately, each
under its own time limit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "--summarise":
    import re

    rows, order = {}, []
    for path in sys.argv[2:]:
        for line in open(path):
            m = re.match(r"AB tag=(\S+) row=(\S+) kernel=(\S+) median=(\S+) spread=(\S+)", line)
            if m:
                if m.group(2) not in rows:
                    order.append(m.group(2))
                rows.setdefault(m.group(2), {}).setdefault(m.group(1), []).append(float(m.group(4)))
    for base in ("parent", "knob0"):
        print("%-18s | %-36s | %-36s | diff  spread ratio all-below" % ("row", base + " runs", "change runs"))
        for row in order:
            p, c = rows[row].get(base, []), rows[row].get("change", [])
            if p and c:
                diff, spread = float(np.median(p) - np.median(c)), max(p) - min(p)
                print("%-18s | %-36s | %-36s | %+.2f %.2f %5.1f %s" % (row, " ".join("%.2f" % v for v in p), " ".join("%.2f" % v for v in c), diff, spread,
                                                                      diff / max(spread, 1e-9), "yes" if max(c) < min(p) else "no"))
    sys.exit(0)

import ab_bwd_short_gather as ab     # (binds CTPVAE_VARIANT_LIB, sets the tag)
import torch
from ct_pvae_amd import phantoms
from ct_pvae_amd.forward_functions import RotatePlan


def main():
    print("library:", ab._lib.LIB_PATH, "tag:", ab.TAG, flush=True)
    for B, A, what in ((50, 20, "adj fwd pair"), (1, 20, "adj"), (5, 20, "adj"), (25, 20, "adj"), (40, 20, "adj"), (80, 20, "adj"), (40, 32, "adj"), (80, 32, "adj"), (50, 8, "adj"), (50, 24, "adj"), (50, 28, "adj"),
                       (50, 16, "adj"), (50, 32, "adj"), (50, 180, "adj")):
        theta = phantoms.dense_theta(180)[np.arange(A) * 180 // A]
        plan = RotatePlan(theta, 128, 128, True, ab.d)
        x = torch.rand((B, 128, 128), device=ab.d)
        gs = torch.randn((B, A, plan.PW), device=ab.d)
        out, gx = torch.empty_like(gs), torch.empty_like(x)
        n = 200 if B * A < 8000 else 50

        def pair():
            plan.forward(x, out=out)
            plan.backward(out, out=gx)
        for w in what.split():
            body = {"adj": lambda: plan.backward(gs, out=gx), "fwd": lambda: plan.forward(x, out=out), "pair": pair}[w]
            kernel = {"adj": plan.backward_kernel_name(B), "fwd": plan.forward_kernel_name(B), "pair": "both"}[w]
            ab.report("B=%d_A=%d_%s" % (B, A, w), kernel, ab.timed(body, n))


if __name__ == "__main__":
    main()
