"""Times the likelihood training call on the ray-driven projector (calculate_log_prob_M_given_R(model="siddon"),
reduce="per_object", reconstruction gradient only) against what a user has to write without it: project_tf_fast(model="siddon")
on the gathered theta + gaussian_poisson_log_prob on gathered operands + a torch sum, and autograd's backward through both.

Method (as tools/ab_compare.py): each variant is captured into a HIP graph after a warm-up call, the graphs are replayed in
alternation (A B A B ...) on one box, HIP events bracket blocks of replays; per variant the median and the min / max of the
block means are printed, in microseconds per call.

    python tools/time_siddon_loglik.py [--blocks 15] [--reps 20] [--trainer]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import phantoms  # noqa: E402

PNM, EPS = 1e4, 1.2e-7


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def time_graphs(graphs, blocks, reps):
    res = {k: [] for k in graphs}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record()
            b.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / reps)
    return res


def shape_case(B, n_sub, A_all, blocks, reps, dev):
    rng = np.random.default_rng(B + n_sub)
    theta = np.ascontiguousarray(phantoms.dense_theta(A_all), dtype=np.float32)
    sub = None if n_sub == A_all else rng.permutation(A_all)[:n_sub]
    img = phantoms.foam_batch(B, 128, seed=1, supersample=2)
    x = torch.from_numpy(img[..., None]).to(dev).requires_grad_(True)
    mask = torch.from_numpy(rng.uniform(0.02, 0.08, (B, A_all)).astype(np.float32)).to(dev)
    meas = torch.rand((B, A_all, 184), device=dev) * 3.0
    pnm = torch.tensor(PNM, device=dev)
    w = torch.linspace(0.5, 2.0, B, device=dev)
    idx = None if sub is None else torch.from_numpy(sub).to(dev)
    th_sub = theta if sub is None else np.ascontiguousarray(theta[sub])

    def fused():
        with torch.autograd.set_multithreading_enabled(False):
            s = cp.calculate_log_prob_M_given_R(x, mask, meas, pnm, EPS, theta=theta, angles_i=sub, pad=True, model="siddon",
                                                reduce="per_object")
            return s, torch.autograd.grad(s, x, w)[0]

    def two_step():
        with torch.autograd.set_multithreading_enabled(False):
            m, y = (mask, meas) if idx is None else (mask.index_select(1, idx), meas.index_select(1, idx))
            proj = cp.project_tf_fast(x, th_sub, pad=True, dim=2, integrate_vae=True, model="siddon")
            lp = cp.gaussian_poisson_log_prob(proj[..., 0], m, y, pnm, EPS)
            s = lp.sum(dim=(1, 2))
            return s, torch.autograd.grad(s, x, w)[0]

    gf, of = capture(fused)
    gt, ot = capture(two_step)
    gf.replay(), gt.replay()
    torch.cuda.synchronize()
    gerr = float((of[1] - ot[1]).abs().max() / ot[1].abs().max())
    serr = float(((of[0] - ot[0]).abs() / ot[0].abs()).max())
    res = time_graphs({"fused": gf, "two_step": gt}, blocks, reps)
    line = f"B={B:3d} angles={n_sub:3d}/{A_all} 128x128:"
    for k, v in res.items():
        line += f"  {k} median {np.median(v):8.2f} us (min {min(v):8.2f}, max {max(v):8.2f})"
    line += f"  ratio two_step/fused {np.median(res['two_step']) / np.median(res['fused']):.3f}"
    line += f"  [sums rel diff {serr:.1e}, grad diff / max {gerr:.1e}]"
    print(line, flush=True)


def trainer_case(model, steps, dev):
    from ct_pvae_amd import trainer as tr
    args = tr.get_args(f"--nsa 20 --td 50 -b 5 --ns 2 --api 20 --pnm 1e4 --random --normal -i {steps} --train --model {model}".split())
    t = tr.PVAETrainer(args, dev)
    for _ in range(10):
        t.train_step(sync=False)
    torch.cuda.synchronize()
    rates = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(steps):
            t.train_step(sync=False)
        torch.cuda.synchronize()
        rates.append(steps / (time.perf_counter() - t0))
    print(f"trainer --model {model} -b 5 --ns 2 --api 20: median {np.median(rates):.2f} steps/s "
          f"(min {min(rates):.2f}, max {max(rates):.2f}; 5 blocks of {steps} steps)", flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--trainer", action="store_true")
    p.add_argument("--trainer_steps", type=int, default=40)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    print(f"device {torch.cuda.get_device_name(0)}; {a.blocks} alternated blocks of {a.reps} graph replays per variant", flush=True)
    for B, n, A in ((10, 20, 180), (50, 20, 180), (50, 180, 180)):
        shape_case(B, n, A, a.blocks, a.reps, dev)
    if a.trainer:
        for model in ("rotate", "siddon", "rotate", "siddon"):
            trainer_case(model, a.trainer_steps, dev)


if __name__ == "__main__":
    main()
