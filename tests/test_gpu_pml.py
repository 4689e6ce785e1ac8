"""recon(algorithm='pml_quad' | 'pml_hybrid' | 'ospml_quad' | 'ospml_hybrid') on the MI355X against its numpy restatement
(tests/np_twin_pml.py, composed from the CPU oracle's projector pair), the new store on its own bit for bit, determinism, one
full-size call and the callers.

Bars.  Parity: `it` iterations within it * 1e-5 of the twin's maximum, the suite's bar for mlem (tests/test_gpu_mlem.py: one back-
projection's corner slivers per iteration).  It carries over because the root is no more sensitive to the gather's sum u and to
G = P + sum_dist than mlem's product x * u / sum_dist is: with x_new = -2 E / (G + S) and S^2 = G^2 - 8 E F (so that -8 E F =
(S - G) (S + G)),  d ln x_new / d ln E = (S + G) / (2 S), which lies in [0, 1], and  d x_new / d G = -x_new / S, i.e. |d x_new / d G| *
S / x_new = 1 with S >= |G|.  The store alone: the gather's sum is taken from ctpvae_siddon_bwd_sel_scaled_f32 (the
same gather, the same bits), the epilogue is fp32 +, -, *, /, sqrt in a stated order with contraction off, all correctly rounded
on both sides: assert_array_equal."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib, phantoms
from ct_pvae_amd.forward_functions import _stream_ptr
from ct_pvae_amd.helper_functions import _siddon_tables
from tests import np_twin_pml as tw

pytestmark = pytest.mark.gpu

rc = importlib.import_module("ct_pvae_amd.recon")        # (the package exports the function `recon` under the same name)
recon = rc.recon

REL = 1e-5
N, A, COUNTS = 64, 45, 50.0


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def nan_out(shape, device):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=device)


@pytest.fixture(scope="module")
def foam(oracle):
    """3 foam slices at 64^2, 45 angles over pi, pad=True, Poisson-noised at 50 counts per unit: the input of tests/test_pml_cpu.py.
    The reconstruction grid is 94 x 94: partial tiles in both directions, two tile columns."""
    img = phantoms.foam_batch(3, N, seed=4, supersample=2)
    theta = np.linspace(0.0, np.pi, A, endpoint=False).astype(np.float32)
    sino = np.ascontiguousarray(np.swapaxes(oracle.siddon_project(img, theta, pad=True), 0, 1))
    noisy = (np.random.default_rng(0).poisson(sino.astype(np.float64) * COUNTS) / COUNTS).astype(np.float32)
    return img, theta, sino, noisy


def twin_kw(kw):
    """recon()'s keywords -> np_twin_pml.pml's."""
    par = np.ones(2) if kw.get("reg_par") is None else np.asarray(kw["reg_par"], np.float64).reshape(-1)
    out = {"beta": float(par[0]), "hybrid": kw["algorithm"].endswith("hybrid")}
    if out["hybrid"]:
        out["delta"] = float(par[1])
    for k in ("num_block", "ind_block"):
        if k in kw:
            out[k] = kw[k]
    return out


def test_pml_matches_the_twin(foam):
    """Every rel_err is printed before any is asserted (run with -s; profiles/r12_pml.txt holds what has been recorded)."""
    _, theta, _, noisy = foam
    d = dev()
    data = torch.from_numpy(noisy).to(d)
    shuffled = np.random.default_rng(7).permutation(A)
    cases = [{"algorithm": "pml_quad"}, {"algorithm": "pml_hybrid", "reg_par": [1.0, 0.1]},
             {"algorithm": "ospml_quad", "num_block": 5}, {"algorithm": "ospml_quad", "num_block": 7},
             {"algorithm": "ospml_quad", "num_block": 7, "ind_block": shuffled}, {"algorithm": "ospml_hybrid", "num_block": 5}]
    worst = []
    for kw in cases:
        want = {}
        tw.pml(noisy, theta, 20, each=lambda it, x: want.__setitem__(it, x.copy()), **twin_kw(kw))
        for it in (1, 5, 20):
            got = to_np(recon(data, theta, sinogram_order=True, num_iter=it, **kw))
            assert got.shape == want[it].shape == (3, noisy.shape[2], noisy.shape[2]) and np.isfinite(got).all()
            e = rel_err(got, want[it])
            tag = f"{kw['algorithm']} {'shuffled ' if 'ind_block' in kw else ''}num_block={kw.get('num_block', '-')} num_iter={it}"
            print(f"rel_err {tag}: {e:.3e} (bound {it * REL:.0e})")
            worst.append((e <= it * REL, tag, e))
    assert all(ok for ok, _, _ in worst), [w for w in worst if not w[0]]


def test_equalities_and_determinism(foam):
    _, theta, _, noisy = foam
    d = dev()
    data = torch.from_numpy(noisy).to(d)
    quad5 = recon(data, theta, sinogram_order=True, algorithm="pml_quad", num_iter=5)
    assert torch.equal(recon(data, theta, sinogram_order=True, algorithm="ospml_quad", num_iter=5), quad5)      # tomopy's num_block = 1
    assert torch.equal(recon(data.permute(1, 0, 2), theta, algorithm="pml_quad", num_iter=5), quad5)            # tomopy's axis order
    kw = dict(sinogram_order=True, algorithm="ospml_hybrid", num_iter=5, num_block=5, reg_par=[1.0, 0.1])
    a, b = recon(data, theta, **kw), recon(data, theta, **kw)
    assert torch.equal(a, b) and torch.isfinite(a).all() and not torch.equal(a, quad5)


def test_beta_zero_is_mlem(foam):
    _, theta, _, noisy = foam
    data = torch.from_numpy(noisy).to(dev())
    got = to_np(recon(data, theta, sinogram_order=True, algorithm="pml_quad", reg_par=0, num_iter=5))
    want = to_np(recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=5))
    e = rel_err(got, want)
    print(f"pml_quad(beta = 0) against mlem, 5 iterations: {e:.3e}")
    assert np.isfinite(got).all() and e <= 5e-5


def raw_store(ratio, theta, gx, gy, x_in, beta, delta, hybrid, sel=None):
    """ctpvae_siddon_bwd_sel_pml_f32 on a workspace prepared for `theta`, into a NaN-filled x_out; u = A_sel^T ratio and the block's
    sum_dist come from ctpvae_siddon_bwd_sel_scaled_f32.  Returns (x_out, u, sum_dist) as numpy arrays."""
    lib = _lib.load()
    d = ratio.device
    tables = _siddon_tables(theta, d)
    sin_t, cos_t, quad = tables
    oy, n, dx = ratio.shape
    dt = sin_t.numel()
    ws = rc._bp_workspace(tables, oy, gx, gy, dt, dx, d)
    geo = (gx, gy, sin_t.data_ptr(), cos_t.data_ptr(), quad.data_ptr(), dt, dx, ctypes.c_float(dx / 2.0))
    selp = sel.data_ptr() if sel is not None else None
    colsum, u, x_out = nan_out((1, gx, gy), d), nan_out((oy, gx, gy), d), nan_out((oy, gx, gy), d)
    ones = torch.ones((1, n, dx), device=d)
    _lib.check(lib.ctpvae_siddon_bwd_sel_scaled_f32(ones.data_ptr(), 1, *geo, selp, n, ws.data_ptr(), None, 0, colsum.data_ptr(),
                                                    _stream_ptr()), "bwd_sel_scaled")
    _lib.check(lib.ctpvae_siddon_bwd_sel_scaled_f32(ratio.data_ptr(), oy, *geo, selp, n, ws.data_ptr(), None, 0, u.data_ptr(),
                                                    _stream_ptr()), "bwd_sel_scaled")
    _lib.check(lib.ctpvae_siddon_bwd_sel_pml_f32(ratio.data_ptr(), oy, *geo, selp, n, ws.data_ptr(), colsum.data_ptr(),
                                                 ctypes.c_float(beta), ctypes.c_float(delta), int(hybrid), x_in.data_ptr(),
                                                 x_out.data_ptr(), _stream_ptr()), "bwd_sel_pml")
    return to_np(x_out), to_np(u), to_np(colsum[0])


def store_state(oy, gx, gy, use_sel, scale, seed):
    """24 angles (or a shuffled 9-angle subset of them), a random ratio, x_in in [0, scale) with exact zeros."""
    rng = np.random.default_rng(seed)
    dt = 24
    dx = _lib.load().ctpvae_siddon_dx(gx, gy, 1)
    theta = np.sort(rng.uniform(0.0, np.pi, dt)).astype(np.float32)
    sel = rng.permutation(dt)[:9].astype(np.int32) if use_sel else None
    ratio = rng.random((oy, 9 if use_sel else dt, dx), dtype=np.float32) * np.float32(2.0)
    x0 = rng.random((oy, gx, gy), dtype=np.float32) * np.float32(scale)
    x0[rng.random((oy, gx, gy)) < 0.1] = 0.0
    return theta, sel, ratio, x0


def check_store(oy, gx, gy, use_sel, scale, seed):
    """Both penalties on one random state (scale chosen so that G takes both signs), x_out NaN-filled; bit comparison with the
    numpy epilogue; x_in untouched."""
    d = dev()
    theta, sel, ratio, x0 = store_state(oy, gx, gy, use_sel, scale, seed)
    sel = torch.from_numpy(sel).to(d) if use_sel else None
    ratio, x_in = torch.from_numpy(ratio).to(d), torch.from_numpy(x0).to(d)
    beta, delta = 0.3, 0.1
    for hybrid in (False, True):
        got, u, cs = raw_store(ratio, theta, gx, gy, x_in, beta, delta, hybrid, sel)
        assert not np.isnan(got).any() and np.isfinite(u).all() and (cs > 0).any()
        np.testing.assert_array_equal(to_np(x_in), x0)
        want = tw.update(x0, u, cs, beta, delta, hybrid)
        np.testing.assert_array_equal(got, want)
        assert not np.array_equal(got, x0)
    # the quadratic case's G = sum_dist - 2 beta sum_q w_q (x + x_k): both forms of the root are exercised
    w = tw.weights(gx, gy)
    G = cs - 2 * beta * sum(w[q] * (x0 + tw.neighbour(x0, di, dj)) for q, (di, dj) in enumerate(tw.NEIGHBOURS))
    assert (G > 0).any() and (G <= 0).any()


@pytest.mark.parametrize("use_sel", [False, True])
@pytest.mark.parametrize("oy", [1, 3, 5, 11])
def test_store_alone_bit_for_bit(oy, use_sel):
    """Grid 70 x 130: 8.75 tile rows; three tile columns, the last 2 wide, so halos cross columns 63|64 and 127|128.  oy: every
    number of slices per workgroup (1, 2, 4, 8), each with a remainder."""
    check_store(oy, 70, 130, use_sel, 60.0 if not use_sel else 25.0, seed=10 * oy + use_sel)


@pytest.mark.parametrize("gx,gy", [(2, 2), (9, 3)])
def test_store_on_edges_and_corners(gx, gy):
    """2 x 2: corners only (3 neighbours); 9 x 3: corners, edges and a single interior column, two tile rows."""
    check_store(3, gx, gy, False, 40.0, seed=gx)


def test_full_size_once(oracle):
    """4 slices on the 184^2 grid of the 128^2 training set, 180 angles, ospml_quad with 6 blocks, 2 iterations against the twin."""
    d = dev()
    theta = np.linspace(0.0, np.pi, 180, endpoint=False).astype(np.float32)
    img = phantoms.foam_batch(4, 128, seed=5, supersample=1)
    sino = np.ascontiguousarray(np.swapaxes(oracle.siddon_project(img, theta, pad=True), 0, 1))
    noisy = (np.random.default_rng(1).poisson(sino.astype(np.float64) * COUNTS) / COUNTS).astype(np.float32)
    assert noisy.shape == (4, 180, 184)
    got = to_np(recon(torch.from_numpy(noisy).to(d), theta, sinogram_order=True, algorithm="ospml_quad", num_block=6, num_iter=2))
    want = tw.pml(noisy, theta, 2, num_block=6)
    e = rel_err(got, want)
    print(f"full size: rel_err ospml_quad num_block=6 num_iter=2: {e:.3e} (bound 2e-05)")
    assert got.shape == (4, 184, 184) and np.isfinite(got).all() and e <= 2e-5


def test_callers(foam, tmp_path):
    img, theta, sino, noisy = foam
    d = dev()
    P = sino.shape[2]
    mask = np.zeros(A, np.float32)
    mask[::5] = 1.0 / 9
    pe, ne, r0, r1, r2 = cp.evaluate_sinogram(sino[0], sino[0] * 0.98, noisy[0] * mask[:, None], torch.from_numpy(mask), theta, N, N,
                                              algorithm="pml_hybrid", verbose=False)
    assert r0.shape == r1.shape == r2.shape == (N, N) and len(pe) == len(ne) == 3
    assert np.isfinite(np.asarray(pe + ne, np.float64)).all() and all(np.isfinite(r).all() for r in (r0, r1, r2))
    masks = torch.from_numpy(np.tile(mask, (3, 1))).to(d)
    samples = torch.from_numpy(noisy).to(d) * masks[..., None]
    enc = cp.iradon_all(samples, masks, P, theta, ["pml_quad", "gridrec"], 1e-7, N, N, save_path=str(tmp_path), train=True)
    assert tuple(enc.shape) == (3, N, N, 3) and torch.isfinite(enc).all()
    data = torch.from_numpy(noisy).to(d)
    with pytest.raises(ValueError):
        recon(data, theta, sinogram_order=True, algorithm="pml_quad", num_gridx=1)
    assert recon(data[:0], theta, sinogram_order=True, algorithm="ospml_hybrid").shape == (0, P, P)
