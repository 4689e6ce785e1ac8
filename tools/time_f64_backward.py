"""Developer tool: the float64 backward (ctpvae_rotate_bwd_f64) next to the fp32 backward of the same call, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_f64_backward.py

Shapes: 50 x 128^2 x 20 angles (nearest and bilinear, tf_compat and exact) and 8 x 512^2 x 90 bilinear (both modes).  Each call
runs WARM + REPS times; the host times REPS back-to-back launches between two synchronisations (enqueue-bound for short kernels:
read the kernel trace for kernel time).  The launches of one shape share a kernel name and differ in grid size."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ct_pvae_amd import phantoms  # noqa: E402
from ct_pvae_amd.forward_functions import RotatePlan  # noqa: E402

WARM, REPS = 3, 20


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / REPS


def main():
    d = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    cases = [(50, 128, 20, interp, mode) for interp in ("nearest", "bilinear") for mode in ("tf_compat", "exact")]
    cases += [(8, 512, 90, "bilinear", mode) for mode in ("tf_compat", "exact")]
    for S, N, A, interp, mode in cases:
        theta = phantoms.dense_theta(180)[phantoms.sparse_angle_indices(180, A)] if A < 180 else phantoms.dense_theta(180)
        plan = RotatePlan(theta, N, N, True, d, interp=interp, backward=mode)
        g64 = torch.from_numpy(rng.standard_normal((S, A, plan.PW))).to(d)
        g32 = g64.float()
        o64 = torch.empty((S, N, N), dtype=torch.float64, device=d)
        o32 = torch.empty((S, N, N), dtype=torch.float32, device=d)
        t64 = timed(lambda: plan.backward_f64(g64, out=o64))
        t32 = timed(lambda: plan.backward(g32, out=o32))
        print(f"{S} x {N}^2 x {A} {interp:8s} {mode:9s}: f64 {t64:9.1f} us/call ({plan.PW} bins), "
              f"fp32 {t32:8.1f} us/call", flush=True)


if __name__ == "__main__":
    main()
