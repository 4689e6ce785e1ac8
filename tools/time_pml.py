"""Times ONE iteration of recon(algorithm='pml_quad' | 'pml_hybrid') -- the forward launch with the ratio store + the back-projector
launch with the penalized update as its store (ctpvae_siddon_fwd_ratio_f32 / ctpvae_siddon_bwd_sel_pml_f32) -- against the
composition the library offered before: _project -> torch.where(sim != 0, data / sim, 0) -> _backproject -> the update written with
torch ops over 8 shifted copies of x, at 3 slices x 94^2 x 45 angles (the tests' fixture) and 50 slices x 184^2 x 180 angles (the
reconstruction grid of the 128^2 training set).

Method (tools/time_mlem.py's): each variant is captured into a HIP graph after a warm-up, the graphs are replayed in alternation on
one box, HIP events bracket blocks of replays; per variant the median and the 10th / 90th percentile of the block means are printed,
in microseconds per iteration, and appended to profiles/r12_pml.txt (--out).  Every replay runs ONE iteration from the same fixed
state (the second pml_quad iterate): the update reads x and writes another buffer, so nothing has to be restored.  The results of
the two paths are compared once per penalty.

    python tools/time_pml.py [--blocks 15] [--reps 10] [--out FILE]"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ct_pvae_amd import _lib, phantoms  # noqa: E402
from ct_pvae_amd.forward_functions import _stream_ptr  # noqa: E402
from ct_pvae_amd.helper_functions import _siddon_tables, create_sinograms  # noqa: E402
from tools.time_siddon_loglik import capture, time_graphs  # noqa: E402

rc = importlib.import_module("ct_pvae_amd.recon")

NEIGHBOURS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
BETA, DELTA = 1.0, 0.1


def penalty_weights(gx, gy, dev):
    """[8][gx][gy]: direct a, diagonal a / sqrt(2), a = 1 / (n_direct + n_diag / sqrt(2)) over the neighbours inside the grid, else 0."""
    i, j = torch.meshgrid(torch.arange(gx, device=dev), torch.arange(gy, device=dev), indexing="ij")
    inside = torch.stack([(i + di >= 0) & (i + di < gx) & (j + dj >= 0) & (j + dj < gy) for di, dj in NEIGHBOURS]).double()
    a = 1.0 / (inside[:4].sum(0) + inside[4:].sum(0) / np.sqrt(2.0))
    scale = torch.tensor([1.0] * 4 + [1.0 / np.sqrt(2.0)] * 4, dtype=torch.float64, device=dev)[:, None, None]
    return (inside * a * scale).float()


def torch_update(x, u, colsum, w, hybrid):
    """The store of ctpvae_siddon_bwd_sel_pml_f32 with torch ops (the order of include/ctpvae_radon.h)."""
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    gx, gy = x.shape[-2:]
    E = -(x * u)
    F, P = torch.zeros_like(x), torch.zeros_like(x)
    for q, (di, dj) in enumerate(NEIGHBOURS):
        xk = xp[:, 1 + di:1 + di + gx, 1 + dj:1 + dj + gy]
        t = (2.0 * BETA) * w[q]
        if hybrid:
            t = t * (1.0 / (1.0 + ((x - xk) / DELTA).abs()))
        F = F + t
        P = P - t * (x + xk)
    G = P + colsum
    S = torch.sqrt(G * G - (8.0 * E) * F)
    return torch.where(G > 0, (-2.0 * E) / (G + S), torch.where(F != 0, (-G + S) / (4.0 * F), x))


def shape_case(S, n, A, blocks, reps, dev):
    lib = _lib.load()
    theta = np.linspace(0.0, np.pi, A, endpoint=False).astype(np.float32)
    img = torch.from_numpy(phantoms.foam_batch(S, n, seed=S, supersample=1)).to(dev)
    data = create_sinograms(img, theta, pad=True)
    dx = data.shape[2]
    gx = gy = dx
    tables = _siddon_tables(theta, dev)
    sin_t, cos_t, quad = tables
    ws = rc._bp_workspace(tables, S, gx, gy, A, dx, dev)
    colsum = rc._backproject(torch.ones((1, A, dx), device=dev), tables, gx, gy, ws=ws)[0]
    need = lib.ctpvae_siddon_fwd_workspace_bytes(S, gx, gy)
    fws = torch.empty(int(need), dtype=torch.uint8, device=dev) if need else None
    start = rc.recon(data, theta, sinogram_order=True, algorithm="pml_quad", num_iter=2)       # a plausible iterate, not the flat start
    w = penalty_weights(gx, gy, dev)
    ratio = torch.empty_like(data)
    geo = (gx, gy, sin_t.data_ptr(), cos_t.data_ptr(), quad.data_ptr(), A, dx, ctypes.c_float(dx / 2.0))
    outs = {k: torch.empty_like(start) for k in ("fused quad", "fused hybrid", "composed quad", "composed hybrid")}

    def fused(hybrid):
        out = outs["fused hybrid" if hybrid else "fused quad"]

        def run():
            sp = _stream_ptr()
            _lib.check(lib.ctpvae_siddon_fwd_ratio_f32(start.data_ptr(), S, *geo, None, A, data.data_ptr(),
                                                       fws.data_ptr() if fws is not None else None, ratio.data_ptr(), sp), "fwd_ratio")
            _lib.check(lib.ctpvae_siddon_bwd_sel_pml_f32(ratio.data_ptr(), S, *geo, None, A, ws.data_ptr(), colsum.data_ptr(),
                                                         ctypes.c_float(BETA), ctypes.c_float(DELTA), int(hybrid), start.data_ptr(),
                                                         out.data_ptr(), sp), "bwd_sel_pml")
            return out
        return run

    def composed(hybrid):
        out = outs["composed hybrid" if hybrid else "composed quad"]

        def run():
            sim = rc._project(start, tables, dx)
            r = torch.where(sim != 0, data / sim, torch.zeros_like(sim))
            u = rc._backproject(r, tables, gx, gy, ws=ws)
            out.copy_(torch_update(start, u, colsum, w, hybrid))
            return out
        return run

    fns = {"fused quad": fused(False), "composed quad": composed(False), "fused hybrid": fused(True), "composed hybrid": composed(True)}
    # one iteration each from the same start, outside the graphs: the two paths compute the same thing
    once = {k: f().clone() for k, f in fns.items()}
    diff = {p: float((once[f"fused {p}"] - once[f"composed {p}"]).abs().max() / once[f"composed {p}"].abs().max()) for p in ("quad", "hybrid")}
    res = time_graphs({k: capture(f)[0] for k, f in fns.items()}, blocks, reps)
    lines = []
    for p in ("quad", "hybrid"):
        line = f"S={S:3d} grid {gx}x{gy} angles={A:3d} {p:6s}:"
        for k in (f"fused {p}", f"composed {p}"):
            v = res[k]
            line += f"  {k.split()[0]} median {np.median(v):10.1f} us (p10 {np.percentile(v, 10):10.1f}, p90 {np.percentile(v, 90):10.1f})"
        line += f"  ratio composed/fused {np.median(res[f'composed {p}']) / np.median(res[f'fused {p}']):.3f}"
        line += f"  [max |fused - composed| / max {diff[p]:.1e}; finite: {bool(torch.isfinite(outs[f'fused {p}']).all())}]"
        lines.append(line)
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r12_pml.txt"),
                   help="the lines are appended to this file")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"device {torch.cuda.get_device_name(0)}; one pml iteration (beta {BETA}, delta {DELTA}) from a fixed state; {a.blocks} alternated "
             f"blocks of {a.reps} graph replays per variant"]
    print(lines[0], flush=True)
    for S, n, A in ((3, 64, 45), (50, 128, 180)):
        for line in shape_case(S, n, A, a.blocks, a.reps, dev):
            lines.append(line)
            print(line, flush=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
