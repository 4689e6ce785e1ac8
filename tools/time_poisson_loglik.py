"""Times calculate_log_prob_M_given_R(noise="poisson", reduce="per_object") + the reconstruction gradient against the two-step
Poisson path on gathered operands (project_tf_fast on the gathered theta, poisson_log_prob, a torch sum, autograd's backward
through both), with the Gaussian call beside it, for both models: B slices of 128 x 128, 20 of 180 angles.

Method (tools/time_siddon_loglik.py's): each variant is captured into a HIP graph after a warm-up, the graphs are replayed in
alternation (A B C A B C ...) on one box, HIP events bracket blocks of replays; per variant the median and the min / max of the
block means are printed, in microseconds per call.

    python tools/time_poisson_loglik.py [--blocks 15] [--reps 20] [B ...]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import phantoms  # noqa: E402
from tools.time_siddon_loglik import capture, time_graphs  # noqa: E402

PNM, EPS = 1e4, 1.2e-7


def shape_case(model, B, blocks, reps, d):
    theta = np.ascontiguousarray(phantoms.dense_theta(180), dtype=np.float32)
    sub = np.random.default_rng(0).permutation(180)[:20].astype(np.int32)
    img = torch.from_numpy(phantoms.foam_batch(B, 128, seed=B, supersample=2)[..., None]).to(d)
    sino = cp.project_tf_fast(img, theta, pad=True, dim=2, integrate_vae=True, model=model)[..., 0]
    mask, meas = cp.create_all_masks(x_train_sinograms=sino, num_angles=180, poisson_noise_multiplier=PNM, num_sparse_angles=20,
                                     random=True, train=True, seed=1)
    x = (img * 0.9).requires_grad_(True)
    w = torch.linspace(0.5, 2.0, B, device=d)
    idx = torch.from_numpy(sub).to(d).long()
    m2, y2, th2 = mask[:, idx].contiguous(), meas[:, idx].contiguous(), np.ascontiguousarray(theta[sub])

    def fused(noise):
        def step():
            with torch.autograd.set_multithreading_enabled(False):
                s = cp.calculate_log_prob_M_given_R(x, mask, meas, PNM, EPS, theta=theta, angles_i=sub, pad=True, reduce="per_object",
                                                    model=model, noise=noise)
                return s, torch.autograd.grad(s, x, w)[0]
        return step

    def two_step():
        with torch.autograd.set_multithreading_enabled(False):
            proj = cp.project_tf_fast(x, th2, pad=True, dim=2, integrate_vae=True, model=model)
            s = cp.poisson_log_prob(proj[..., 0], m2, y2, PNM).sum(dim=(1, 2))
            return s, torch.autograd.grad(s, x, w)[0]

    graphs, outs = {}, {}
    for name, fn in (("fused_poisson", fused("poisson")), ("two_step_poisson", two_step), ("fused_gaussian", fused("gaussian"))):
        graphs[name], outs[name] = capture(fn)
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    f, t = outs["fused_poisson"], outs["two_step_poisson"]
    fin = torch.isfinite(t[0])
    serr = float(((f[0] - t[0]).abs() / t[0].abs())[fin].max()) if fin.any() else float("nan")
    gerr = float((f[1] - t[1]).abs().max() / t[1].abs().max())
    res = time_graphs(graphs, blocks, reps)
    line = f"model={model:6s} B={B:3d} angles=20/180 128x128:"
    for k, v in res.items():
        line += f"  {k} median {np.median(v):8.2f} us (min {min(v):8.2f}, max {max(v):8.2f})"
    line += f"  ratio two_step/fused poisson {np.median(res['two_step_poisson']) / np.median(res['fused_poisson']):.3f}"
    line += f"  [sums rel diff {serr:.1e}, grad diff / max {gerr:.1e}]"
    print(line, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("B", type=int, nargs="*", default=[10, 50])
    a = p.parse_args()
    d = torch.device("cuda", 0)
    print(f"device {torch.cuda.get_device_name(0)}; {a.blocks} alternated blocks of {a.reps} graph replays per variant", flush=True)
    for model in ("rotate", "siddon"):
        for B in a.B:
            shape_case(model, B, a.blocks, a.reps, d)


if __name__ == "__main__":
    main()
