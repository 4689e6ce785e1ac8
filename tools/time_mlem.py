"""Times ONE MLEM iteration of recon(algorithm='mlem') -- the forward launch with the ratio store + the back-projector launch with
the multiply store (ctpvae_siddon_fwd_ratio_f32 / ctpvae_siddon_bwd_sel_mul_f32) -- against the composition the library offered
before them: _project -> torch.where(sim != 0, data / sim, 0) -> _backproject -> x * (u / colsum), at the two reconstruction grids of
the training sets: 50 slices x 184^2 x 180 angles and 32 slices x 728^2 x 90 angles.

Method (tools/time_siddon_loglik.py's): each variant is captured into a HIP graph after a warm-up, the graphs are replayed in
alternation (A B A B ...) on one box, HIP events bracket blocks of replays; per variant the median and the 10th / 90th percentile of
the block means are printed, in microseconds per iteration, and appended to profiles/r11_mlem.txt (--out).  Every replay of either
variant first restores its x from the same start (the second MLEM iterate; one copy of x, counted in both figures) and then runs ONE
iteration in place: the back-projector skips angles whose staged values are all zero, so a free-running iteration would be timed on
a drifting state.  The two results are compared once.

    python tools/time_mlem.py [--blocks 15] [--reps 10] [--out FILE]"""
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
    start = rc.recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=2)        # a plausible iterate, not the flat start
    xf, xc = start.clone(), start.clone()
    ratio = torch.empty_like(data)
    geo = (gx, gy, sin_t.data_ptr(), cos_t.data_ptr(), quad.data_ptr(), A, dx, ctypes.c_float(dx / 2.0))

    def fused():
        sp = _stream_ptr()
        xf.copy_(start)
        _lib.check(lib.ctpvae_siddon_fwd_ratio_f32(xf.data_ptr(), S, *geo, None, A, data.data_ptr(),
                                                   fws.data_ptr() if fws is not None else None, ratio.data_ptr(), sp), "fwd_ratio")
        _lib.check(lib.ctpvae_siddon_bwd_sel_mul_f32(ratio.data_ptr(), S, *geo, None, A, ws.data_ptr(), colsum.data_ptr(),
                                                     xf.data_ptr(), sp), "bwd_sel_mul")
        return xf

    def composed():
        xc.copy_(start)
        sim = rc._project(xc, tables, dx)
        r = torch.where(sim != 0, data / sim, torch.zeros_like(sim))
        u = rc._backproject(r, tables, gx, gy, ws=ws)
        xc.copy_(torch.where(colsum != 0, xc * (u / colsum), xc))
        return xc

    # one iteration each from the same start, outside the graphs: the two paths compute the same thing
    f1, c1 = fused().clone(), composed().clone()
    diff = float((f1 - c1).abs().max() / c1.abs().max())
    graphs = {"fused": capture(fused)[0], "composed": capture(composed)[0]}
    res = time_graphs(graphs, blocks, reps)
    line = f"S={S:3d} grid {gx}x{gy} angles={A:3d}:"
    for k, v in res.items():
        line += f"  {k} median {np.median(v):10.1f} us (p10 {np.percentile(v, 10):10.1f}, p90 {np.percentile(v, 90):10.1f})"
    line += f"  ratio composed/fused {np.median(res['composed']) / np.median(res['fused']):.3f}"
    line += f"  [max |fused - composed| / max {diff:.1e}; finite after the run: {bool(torch.isfinite(xf).all())}]"
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_mlem.txt"),
                   help="the lines are appended to this file")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"device {torch.cuda.get_device_name(0)}; one MLEM iteration from a fixed state (+ one copy of x); {a.blocks} alternated blocks of "
             f"{a.reps} graph replays per variant"]
    print(lines[0], flush=True)
    for S, n, A in ((50, 128, 180), (32, 512, 90)):
        lines.append(shape_case(S, n, A, a.blocks, a.reps, dev))
        print(lines[-1], flush=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
