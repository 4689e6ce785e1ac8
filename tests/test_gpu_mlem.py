"""recon(algorithm='mlem' | 'osem') on the MI355X against its numpy restatement (tests/np_twin_mlem.py, composed from the CPU
oracle's projector pair), the two new entry points on their own, determinism, one full-size call and the callers.

Bars.  The forward's ray-sums are the oracle's bits and fp32 division is correctly rounded, so the ratio store is compared with
assert_array_equal.  The pixel-driven back-projector equals the ray-driven accumulation except for corner slivers (~1e-6 of the
image's range, include/ctpvae_radon.h): one iteration within the suite's REL = 1e-5, as 'sirt' at one iteration; every further
iteration adds one back-projection's error, so `it` iterations are held to it * 1e-5 (the suite's 5e-5 for five SIRT iterations)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib, phantoms
from ct_pvae_amd.forward_functions import _stream_ptr
from ct_pvae_amd.helper_functions import _siddon_forward, _siddon_tables, create_sinograms, poisson_log_prob
from tests import np_twin_mlem as tw

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
    """3 foam slices at 64^2, 45 angles over pi, pad=True, Poisson-noised at 50 counts per unit: the input of tests/test_mlem_cpu.py."""
    img = phantoms.foam_batch(3, N, seed=4, supersample=2)
    theta = np.linspace(0.0, np.pi, A, endpoint=False).astype(np.float32)
    sino = np.ascontiguousarray(np.swapaxes(oracle.siddon_project(img, theta, pad=True), 0, 1))
    noisy = (np.random.default_rng(0).poisson(sino.astype(np.float64) * COUNTS) / COUNTS).astype(np.float32)
    return img, theta, sino, noisy


def fwd_ratio(x, tables, dx, meas, sel=None):
    """Raw ctpvae_siddon_fwd_ratio_f32: x [oy][gx][gy], meas [oy][dt_all][dx] -> ratio [oy][rows][dx]."""
    lib = _lib.load()
    sin_t, cos_t, quad = tables
    oy, gx, gy = x.shape
    dt = sin_t.numel()
    n = dt if sel is None else sel.numel()
    need = lib.ctpvae_siddon_fwd_workspace_bytes(oy, gx, gy)
    ws = torch.empty(int(need), dtype=torch.uint8, device=x.device) if need else None
    out = nan_out((oy, n, dx), x.device)
    _lib.check(lib.ctpvae_siddon_fwd_ratio_f32(x.data_ptr(), oy, gx, gy, sin_t.data_ptr(), cos_t.data_ptr(), quad.data_ptr(), dt, dx,
                                               ctypes.c_float(dx / 2.0), sel.data_ptr() if sel is not None else None, n, meas.data_ptr(),
                                               ws.data_ptr() if ws is not None else None, out.data_ptr(), _stream_ptr()), "fwd_ratio")
    return out, bool(need)


def bwd_mul(ratio, tables, gx, gy, x, sel=None):
    """Raw ctpvae_siddon_bwd_sel_mul_f32 on a workspace prepared for `tables`, with the block's sum_dist from _bwd_sel_scaled of
    ones: returns (x * (A_sel^T ratio / sum_dist), sum_dist); x is not modified."""
    lib = _lib.load()
    sin_t, cos_t, quad = tables
    oy, n, dx = ratio.shape
    dt = sin_t.numel()
    ws = rc._bp_workspace(tables, oy, gx, gy, dt, dx, ratio.device)
    geo = (gx, gy, sin_t.data_ptr(), cos_t.data_ptr(), quad.data_ptr(), dt, dx, ctypes.c_float(dx / 2.0))
    selp = sel.data_ptr() if sel is not None else None
    ones = torch.ones((1, n, dx), device=ratio.device)
    colsum = nan_out((1, gx, gy), ratio.device)
    _lib.check(lib.ctpvae_siddon_bwd_sel_scaled_f32(ones.data_ptr(), 1, *geo, selp, n, ws.data_ptr(), None, 0, colsum.data_ptr(),
                                                    _stream_ptr()), "bwd_sel_scaled")
    out = x.clone()
    _lib.check(lib.ctpvae_siddon_bwd_sel_mul_f32(ratio.data_ptr(), oy, *geo, selp, n, ws.data_ptr(), colsum.data_ptr(), out.data_ptr(),
                                                 _stream_ptr()), "bwd_sel_mul")
    return out, colsum[0]


def test_mlem_and_osem_match_the_twin(foam):
    """Every rel_err is printed before any is asserted (run with -s; profiles/r11_mlem.txt section 3 holds what has been recorded)."""
    _, theta, _, noisy = foam
    d = dev()
    data = torch.from_numpy(noisy).to(d)
    shuffled = np.random.default_rng(7).permutation(A)
    cases = [("mlem", {}, {})] + [("osem", {"num_block": nb}, {"num_block": nb}) for nb in (1, 5, 7)] + \
            [("osem", {"num_block": 7, "ind_block": shuffled}, {"num_block": 7, "ind_block": shuffled})]
    worst = []
    for alg, kw, twin_kw in cases:
        want = {}
        tw.mlem(noisy, theta, 20, each=lambda it, x: want.__setitem__(it, x.copy()), **twin_kw)
        for it in (1, 5, 20):
            got = to_np(recon(data, theta, sinogram_order=True, algorithm=alg, num_iter=it, **kw))
            assert got.shape == want[it].shape == (3, noisy.shape[2], noisy.shape[2]) and np.isfinite(got).all()
            e = rel_err(got, want[it])
            tag = f"{alg} {'shuffled ' if 'ind_block' in kw else ''}num_block={kw.get('num_block', '-')} num_iter={it}"
            print(f"rel_err {tag}: {e:.3e} (bound {it * REL:.0e})")
            worst.append((e <= it * REL, tag, e))
    assert all(ok for ok, _, _ in worst), [w for w in worst if not w[0]]
    mlem5 = recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=5)
    assert torch.equal(recon(data, theta, sinogram_order=True, algorithm="osem", num_iter=5, num_block=1), mlem5)
    assert torch.equal(recon(data, theta, sinogram_order=True, algorithm="osem", num_iter=5), mlem5)          # tomopy's defaults
    assert torch.equal(recon(data.permute(1, 0, 2), theta, algorithm="mlem", num_iter=5), mlem5)               # tomopy's axis order


@pytest.mark.parametrize("oy,n", [(2, 64), (5, 256)])
def test_ratio_store_alone(oracle, oy, n):
    """ctpvae_siddon_fwd_ratio_f32 with sel = NULL against data / ctpvae_siddon_fwd_ws_f32(x), element for element: 2 slices take the
    LDS kernels, 5 slices of 256^2 (a pair does not fit LDS) the packed walk with its workspace.  The detector is the padded one,
    wider than the grid: rays that miss the grid have a ray-sum of 0 and must give exactly 0."""
    d = dev()
    rng = np.random.default_rng(oy)
    dx = _lib.load().ctpvae_siddon_dx(n, n, 1)
    theta = np.sort(rng.uniform(0.0, np.pi, 24)).astype(np.float32)
    tables = _siddon_tables(theta, d)
    x = torch.from_numpy(rng.random((oy, n, n), dtype=np.float32) + 0.1).to(d)
    x[0, : n // 2] = 0.0                                       # rays that cross pixels and still sum to 0
    meas = torch.from_numpy(rng.random((oy, 24, dx), dtype=np.float32) * 50.0).to(d)
    sim = to_np(_siddon_forward(x, tables, dx))
    # ... and those ray-sums are the CPU oracle's, element for element: neither side of the comparison below rests on the GPU alone
    np.testing.assert_array_equal(sim, np.swapaxes(oracle.siddon_project(to_np(x), theta, pad=True), 0, 1))
    got, used_workspace = fwd_ratio(x, tables, dx, meas)
    assert used_workspace == (oy >= 3)
    with np.errstate(all="ignore"):
        want = np.where(sim != 0, to_np(meas) / sim, np.float32(0.0)).astype(np.float32)
    np.testing.assert_array_equal(to_np(got), want)
    miss = sim == 0
    assert miss[:, :, 0].all() and miss[0].sum() > miss[1].sum() and (to_np(got)[miss] == 0).all()


def test_determinism_and_subsets(foam):
    """Two runs give equal bits; a launch over an angle subset of the dense geometry gives the bits of a call on the gathered
    tables and the gathered measurements (forward store and multiply store)."""
    _, theta, _, noisy = foam
    d = dev()
    data = torch.from_numpy(noisy).to(d)
    P = noisy.shape[2]
    kw = dict(sinogram_order=True, algorithm="osem", num_iter=6, num_block=5)
    assert torch.equal(recon(data, theta, **kw), recon(data, theta, **kw))
    assert torch.equal(recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=6),
                       recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=6))
    sub = np.random.default_rng(3).permutation(A)[:11].astype(np.int32)
    sel = torch.from_numpy(sub).to(d)
    dense, gathered = _siddon_tables(theta, d), _siddon_tables(np.ascontiguousarray(theta[sub]), d)
    x = torch.from_numpy(np.random.default_rng(4).random((3, P, P), dtype=np.float32) + 0.05).to(d)
    r_sel, _ = fwd_ratio(x, dense, P, data, sel)
    r_gat, _ = fwd_ratio(x, gathered, P, data[:, sel.long()].contiguous())
    assert torch.equal(r_sel, r_gat) and torch.isfinite(r_sel).all()
    x_sel, cs_sel = bwd_mul(r_sel, dense, P, P, x, sel)
    x_gat, cs_gat = bwd_mul(r_gat, gathered, P, P, x)
    assert torch.equal(cs_sel, cs_gat) and torch.equal(x_sel, x_gat) and torch.isfinite(x_sel).all()
    assert not torch.equal(x_sel, x)
    # the store itself: x * (A_sel^T ratio / sum_dist) where sum_dist != 0, else x
    # (in numpy: its float32 division is correctly rounded, as the kernel's is)
    upd, cs, x0 = to_np(rc._backproject(r_gat, gathered, P, P)), to_np(cs_gat), to_np(x)
    with np.errstate(all="ignore"):
        want = np.where(cs != 0, x0 * (upd / cs), x0).astype(np.float32)
    np.testing.assert_array_equal(to_np(x_sel), want)


def test_full_size_once():
    """8 slices on the 728^2 grid of the 512^2 training set, 90 angles, 2 iterations: finite, and the counts are preserved."""
    d = dev()
    theta = np.linspace(0.0, np.pi, 90, endpoint=False).astype(np.float32)
    img = torch.from_numpy(phantoms.foam_batch(8, 512, seed=5, supersample=1)).to(d)
    sino = create_sinograms(img, theta, pad=True)
    assert tuple(sino.shape) == (8, 90, 728)
    x = recon(sino, theta, sinogram_order=True, algorithm="mlem", num_iter=2)
    assert tuple(x.shape) == (8, 728, 728) and torch.isfinite(x).all()
    sim = rc._project(x, _siddon_tables(theta, d), 728)
    ratio = float(sim.double().sum() / sino.double().sum())
    print(f"full size: sum(A x) / sum(data) - 1 = {ratio - 1:.2e}")
    assert abs(ratio - 1.0) <= 1e-5


def test_callers_and_keywords(foam, oracle, tmp_path):
    img, theta, sino, noisy = foam
    d = dev()
    P = sino.shape[2]
    mask = np.zeros(A, np.float32)
    mask[::5] = 1.0 / 9
    pe, ne, r0, r1, r2 = cp.evaluate_sinogram(sino[0], sino[0] * 0.98, noisy[0] * mask[:, None], torch.from_numpy(mask), theta, N, N,
                                              algorithm="mlem", verbose=False)
    assert r0.shape == r1.shape == r2.shape == (N, N) and len(pe) == len(ne) == 3
    assert np.isfinite(np.asarray(pe + ne, np.float64)).all() and all(np.isfinite(r).all() for r in (r0, r1, r2))
    masks = torch.from_numpy(np.tile(mask, (3, 1))).to(d)
    samples = torch.from_numpy(noisy).to(d) * masks[..., None]
    enc = cp.iradon_all(samples, masks, P, theta, ["mlem", "gridrec"], 1e-7, N, N, save_path=str(tmp_path), train=True)
    assert tuple(enc.shape) == (3, N, N, 3) and torch.isfinite(enc).all()
    data = torch.from_numpy(noisy).to(d)
    for kw in ({"algorithm": "sirt", "num_block": 2}, {"algorithm": "osem", "num_block": 0}, {"algorithm": "sirt", "num_block": 0},
               {"algorithm": "osem", "num_block": A + 1}, {"algorithm": "osem", "ind_block": np.arange(A - 1)},
               {"algorithm": "mlem", "ind_block": np.arange(A)}):
        with pytest.raises(ValueError):
            recon(data, theta, sinogram_order=True, **kw)
    # init_recon is honoured: one iteration from a given positive image equals the twin from that image
    init = np.random.default_rng(9).random((3, P, P), dtype=np.float32) + 0.5
    for alg, kw in (("mlem", {}), ("osem", {"num_block": 5})):
        got = to_np(recon(data, theta, sinogram_order=True, algorithm=alg, init_recon=torch.from_numpy(init).to(d), **kw))
        e = rel_err(got, tw.mlem(noisy, theta, 1, init=init, **kw))
        print(f"rel_err {alg} from init_recon: {e:.3e}")
        assert e <= REL
    assert recon(data[:0], theta, sinogram_order=True, algorithm="mlem").shape == (0, P, P)


def test_mlem_raises_the_poisson_likelihood(foam):
    """The estimator and the training call's noise model agree: scored with the repo's own poisson_log_prob on
    create_sinograms(cropped reconstruction), 20 MLEM iterations beat 1, and beat 20 SIRT iterations on the same noisy data.  SIRT
    minimises a least-squares objective and leaves negative pixels; a negative ray-sum has log-probability NaN, so the raw SIRT
    image has no finite score (on the CPU restatements: NaN from 901 ray-sums, profiles/r11_mlem.txt).  Both figures are printed; the
    comparison is made with SIRT's image clamped at 0, the nearest image the model can score, and must hold for the raw image too
    whenever that one's score is finite."""
    _, theta, _, noisy = foam
    d = dev()
    data = torch.from_numpy(noisy).to(d)
    ones = torch.ones((3, A), device=d)

    def score(x):
        proj = create_sinograms(rc.crop(x, N, N, ignore_dim_0=True).contiguous(), theta, pad=True)
        return float(poisson_log_prob(proj, ones, data, COUNTS).double().sum())
    m1 = score(recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=1))
    m20 = score(recon(data, theta, sinogram_order=True, algorithm="mlem", num_iter=20))
    s20 = recon(data, theta, sinogram_order=True, algorithm="sirt", num_iter=20)
    s20_raw, s20_pos = score(s20), score(s20.clamp_min(0.0))
    print(f"summed Poisson log-probability: mlem x1 {m1:.5e}, mlem x20 {m20:.5e}, sirt x20 {s20_raw:.5e} (clamped at 0: {s20_pos:.5e})")
    assert np.isfinite(m1) and np.isfinite(m20) and m20 > m1
    assert np.isfinite(s20_pos) and m20 > s20_pos
    assert not np.isfinite(s20_raw) or m20 > s20_raw
