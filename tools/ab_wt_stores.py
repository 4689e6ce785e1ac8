"""Developer tool: what the store policy of the planned nearest projector pair's OUTPUT stores buys (knob WT_STORES: 0 plain,
1 write-through `sc1`, 2 non-temporal `nt`; unset: the library's rule), on ONE box, in the style of tools/ab_compare.py.

    python tools/ab_wt_stores.py                                                        (the in-tree library: rule, then knob 0 / 1 / 2)
    CTPVAE_VARIANT_LIB=tools/libctpvae_radon_<tag>.bin python tools/ab_wt_stores.py     (another build: its own stores only)

Rows: 128 x 128 padded at B = 1, 5, 50, 400 x 20 angles and B = 50 x 180 angles -- forward alone, adjoint alone, the forward + adjoint
pair (the adjoint reads what the forward stored: a dependent boundary between the two and another to the next replay), the adjoint
followed by an elementwise reader of the gradient image, that reader alone -- and the training call (S = 10, 20 of 180 angles: its kernels have no twin; its consumer reads what the forward stored), the no-regression row.
Each figure: the median of five HIP-graph replays of N launches between two events, after three untimed replays; `spread` is the
largest minus the smallest of the five.  Run parent and change alternately, each process under its own time limit."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ct_pvae_amd import _lib

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
    """(median, spread) in microseconds per call of body"""
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
    return float(np.median(runs)), float(max(runs) - min(runs))


def has_knob():
    return _lib.load().ctpvae_tune_set(b"WT_STORES", -1) == 0


def rows(tag):
    for B, A in ((1, 20), (5, 20), (50, 20), (400, 20), (50, 180)):
        theta = phantoms.dense_theta(180)[:: 180 // A]
        plan = RotatePlan(theta, 128, 128, True, d)
        x = torch.rand((B, 128, 128), device=d)
        gs = torch.randn((B, A, plan.PW), device=d)
        out, gx = torch.empty_like(gs), torch.empty_like(x)
        n = 200 if B * A < 8000 else 50

        def pair():
            plan.forward(x, out=out)
            plan.backward(out, out=gx)
        def adj_read():     # ... and a consumer of the gradient image behind it: a write-through line has left the L2 it was written in
            plan.backward(gs, out=gx)
            torch.mul(gx, 0.5, out=half)
        half = torch.empty_like(gx)
        f, a, p = timed(lambda: plan.forward(x, out=out), n), timed(lambda: plan.backward(gs, out=gx), n), timed(pair, n)
        r, r0 = timed(adj_read, n), timed(lambda: torch.mul(gx, 0.5, out=half), n)
        names = f"{plan.forward_kernel_name(B)}{'_few' if plan.forward_form(B, x) else ''} / {plan.backward_kernel_name(B)}"
        print(f"{tag} B={B} A={A} [{names}]: fwd {f[0]:.2f} (spread {f[1]:.2f}) adj {a[0]:.2f} ({a[1]:.2f}) pair {p[0]:.2f} ({p[1]:.2f}) "
              f"adj+reader {r[0]:.2f} ({r[1]:.2f}) reader {r0[0]:.2f} ({r0[1]:.2f}) us", flush=True)
    theta = phantoms.dense_theta(180)
    dense = RotatePlan(theta, 128, 128, True, d)
    S = 10
    x = torch.rand((S, 128, 128), device=d)
    mask, meas = torch.full((S, 180), 0.05, device=d), torch.rand((S, 180, 184), device=d)
    pnm = torch.tensor(1e4, device=d)
    sub = torch.from_numpy(np.random.default_rng(0).permutation(180)[:20].astype(np.int32))
    w = torch.ones(S, device=d)
    dlp = dense.forward_loglik_sums(x, mask, meas, pnm, 1e-7, angles_i=sub, dense_inputs=True)[1]
    gx = torch.empty_like(x)

    def call():
        dense.forward_loglik_sums(x, mask, meas, pnm, 1e-7, angles_i=sub, dense_inputs=True)
        dense.backward(dlp, out=gx, scale=w, angles_i=sub)
    t = timed(call, 100)
    print(f"{tag} training call S=10, 20 of 180: fwd + likelihood + sums + adj {t[0]:.2f} ({t[1]:.2f}) us", flush=True)


print("library:", _lib.LIB_PATH, flush=True)
rows("rule")
if has_knob():
    for v, name in ((0, "plain"), (1, "sc1"), (2, "nt"), (0, "plain-again")):
        with _lib.tuned("WT_STORES", v):
            rows(name)
