"""Every form and every store of the ray-driven projector pair (csrc/siddon.hip) on the MI355X, cell by cell, against
tests/np_twin_siddon.py (the CPU oracle's ray-sums and back-projections behind each store's expected value).

Forward: five forms (ctpvae_siddon_fwd_form: 0 global memory, 1 one slice in LDS, 2 a slice pair in LDS, 4 / 8 the packed walk)
times six stores (ray-sum, SIRT update, TV dual step, Gaussian likelihood, Poisson likelihood, ratio).  Back-projector:
siddon_bwd_gather_kernel<NS, EPI>, NS in 1 2 4 8 times EPI 0 plain, 1 SIRT +=, 2 TV primal, 3 scaled subset, 4 MLEM multiply, 5 PML.
Grids, angles, slice counts and data: np_twin_siddon's operands section.

Bars.  Ray-sums, the SIRT update, the ratio and the TV dual step: assert_array_equal (the walk's float32 expressions are the
oracle's, '/' is the IEEE quotient, no FMA contraction).  Gaussian lp: REL = 1e-5 of oracle.loglik (max-norm) and np_twin_gauss's
per-sample bar; dlp: that twin's bar; Poisson: np_twin_poisson.bar_from_twin.  Back-projector: the oracle's bits on an even grid
under an even detector, REL where rays lie ON grid lines (odd grid or odd detector: the degenerate-ray kernel, another order) --
the rule of test_random_siddon_and_tiled_geometries; `it` iterations of a recon algorithm: it * REL.  Across forms, knobs and chunked
launches: torch.equal -- a ray's sum runs along the ray and a pixel's sum over angles ascending, then rays, in EVERY form, and the
degenerate rays' image is the accumulator's start value in every form, so no addition moves.

Seen on the device (MI355X; the worst error over its bar per store, over all four grids; run with -s for the lines):
    ray-sums, SIRT update, TV dual step, ratio          equal bits in every form, 0 / 1 / 2 / 4 / 8, on every grid
    Gaussian lp against oracle.loglik                   0.015 of REL (1.5e-7 of the largest |lp|)
    Gaussian lp / dlp against the float64 twin's bar    0.47 / 0.25
    Poisson lp against bar_from_twin                    0.25, the -inf samples equal
    back-projector EPI 0 / 1 / 3 / 4                    equal bits on every grid (rel_err 0.0 on the odd grid too)
    two iterations of sirt / tv / mlem / osem / pml_quad / ospml_hybrid      rel_err 0.0 on every grid (bound 2e-5)
    forms, knobs (SIDDON_NS / _THREADS / _PPB / _BWD_NS / _BWD_CHUNKS) and MAX_SLICES = 4     torch.equal in every cell"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib
from ct_pvae_amd import helper_functions as hf
from ct_pvae_amd.forward_functions import _stream_ptr
from tests import np_twin_siddon as tw

pytestmark = pytest.mark.gpu

rc = importlib.import_module("ct_pvae_amd.recon")
recon = rc.recon

F = np.float32
REL = 1e-5
PNM, EPS = 1e4, 1.2e-7
GRIDS, SUBSET = tw.GRIDS, list(tw.SUBSET)
SLICES = (1, 3, 5, 9)
CHUNKED = 11                                      # slices of the chunked cells, cut by MAX_SLICES = 4
FWD_STORES = ("raysum", "sirt", "tv_dual", "gaussian", "poisson", "ratio")
FWD_FORMS = {s: ({0, 1, 2} if s == "poisson" else {0, 1, 2, 4, 8}) for s in FWD_STORES}
EPIS = {"plain": 0, "sirt_add": 1, "tv_primal": 2, "scaled": 3, "multiply": 4, "pml": 5}
RECON = {"sirt": {}, "tv": {"reg_par": [0.05]}, "mlem": {}, "osem": {"num_block": 3}, "pml_quad": {"reg_par": [0.3]},
         "ospml_hybrid": {"num_block": 3, "reg_par": [0.3, 0.5]}}


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def nan_out(*shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.float32, device=dev())


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def ptr(t):
    return t.data_ptr() if t is not None else None


def geo(tables, gx, gy, dx):
    sin_t, cos_t, quad = tables
    return (gx, gy, sin_t.data_ptr(), cos_t.data_ptr(), quad.data_ptr(), sin_t.numel(), dx, ctypes.c_float(dx / 2.0))


def fwd_form(oy, grid, rows, dx, store):
    f = _lib.load().ctpvae_siddon_fwd_form(oy, grid[0], grid[1], rows, dx, _lib.SIDDON_STORE[store])
    assert f >= 0, _lib.last_error()
    return f


def own_fwd_form(oy, grid, rows, dx, store):
    """The rule of csrc/siddon.hip siddon_fwd_form_rule with no knob set, restated for this module's grids (a pair fits LDS on the
    two small ones, one slice on (100, 258), nothing on (160, 258)); its edges: tests/test_siddon_form_cpu.py."""
    pair_fits, lds = grid[0] < 100, (0 if grid == (160, 258) else 1)
    packed = 8 if oy >= 6 else 4 if oy >= 3 else 0
    if packed and pair_fits and -(-oy // 2) * rows * dx <= 750 * 64:
        packed = 0
    if packed and store != "poisson":
        return packed
    return 2 if lds and oy >= 2 and pair_fits and oy * rows * dx > 500 * 64 else lds


def own_bwd_ns(oy):
    return 8 if oy >= 8 else 4 if oy >= 4 else 2 if oy >= 2 else 1


# ---- raw entry points: every output starts as NaN and none may survive -----------------------------------------------------------
def fwd(store, x, tables, dx, op):
    """One forward launch (plus the packed forms' interleaving pass) through the raw entry point of `store`; op: the store's
    operands on the device.  Returns the tuple of everything the launch wrote."""
    lib = _lib.load()
    oy, gx, gy = x.shape
    need = lib.ctpvae_siddon_fwd_workspace_bytes(oy, gx, gy)
    _lib.check(need, "siddon_fwd_workspace_bytes")
    ws = torch.empty(int(need), dtype=torch.uint8, device=x.device) if need else None
    g, sp = geo(tables, gx, gy, dx), _stream_ptr()
    dt = tables[0].numel()
    if store in ("raysum", "sirt"):
        out = nan_out(oy, dt, dx)
        meas, w = (op["meas"], op["w"]) if store == "sirt" else (None, None)
        _lib.check(lib.ctpvae_siddon_fwd_ws_f32(x.data_ptr(), oy, *g, ptr(meas), ptr(w), ptr(ws), out.data_ptr(), sp), "siddon_fwd_ws")
        outs = (out,)
    elif store == "tv_dual":
        p = op["p"].clone()
        _lib.check(lib.ctpvae_siddon_fwd_ws_tv_dual_f32(x.data_ptr(), oy, *g, op["meas"].data_ptr(), op["w"].data_ptr(), ptr(ws),
                                                        p.data_ptr(), sp), "siddon_fwd_ws_tv_dual")
        outs = (p,)
    elif store == "ratio":
        sel = op.get("sel")
        rows = dt if sel is None else sel.numel()
        out = nan_out(oy, rows, dx)
        _lib.check(lib.ctpvae_siddon_fwd_ratio_f32(x.data_ptr(), oy, *g, ptr(sel), rows, op["meas"].data_ptr(), ptr(ws), out.data_ptr(),
                                                   sp), "siddon_fwd_ratio")
        outs = (out,)
    else:
        sel = op.get("sel")
        rows = dt if sel is None else sel.numel()
        lp = nan_out(oy, rows, dx)
        sino = nan_out(oy, rows, dx) if op.get("want_sino", True) else None
        dlp = nan_out(oy, rows, dx) if op.get("want_dlp", True) else None
        dense = int(op.get("dense", 1 if sel is not None else 0))     # 0: mask [oy][rows], meas [oy][rows][dx], gathered by the caller
        assert tuple(op["mask"].shape) == (oy, dt if dense else rows) and tuple(op["meas"].shape) == (oy, dt if dense else rows, dx)
        head = (x.data_ptr(), oy, *g, ptr(sel), rows, op["mask"].data_ptr(), op["meas"].data_ptr(), dense,
                op["pnm"].data_ptr(), ctypes.c_float(EPS))
        tail = (ptr(ws), ptr(sino), lp.data_ptr(), ptr(dlp), sp)
        if store == "poisson":
            _lib.check(lib.ctpvae_siddon_fwd_loglik_noise_f32(*head, _lib.NOISE["poisson"], *tail), "siddon_fwd_loglik_noise")
        else:
            _lib.check(lib.ctpvae_siddon_fwd_loglik_f32(*head, *tail), "siddon_fwd_loglik")
        outs = tuple(t for t in (lp, sino, dlp) if t is not None)
        if sino is not None:
            assert not torch.isnan(sino).any(), f"{store}: a ray-sum was not written"
        if store == "poisson":      # lp is NaN at a negative rate and dlp at 0 * inf (a masked angle with counts): compared with the twin
            return outs
    for t in outs:
        assert not torch.isnan(t).any(), f"{store}: an element was not written"
    return outs


def bwd(store, data, tables, grid, op):
    """One back-projector launch pair (degenerate rays, gather) through the raw entry point of `store` on a workspace prepared for
    the dense `tables`; data [oy][rows][dx].  Returns the tuple of everything the launch wrote."""
    lib = _lib.load()
    gx, gy = grid
    oy, rows, dx = data.shape
    dt = tables[0].numel()
    ws = rc._bp_workspace(tables, oy, gx, gy, dt, dx, data.device)
    g, sp = geo(tables, gx, gy, dx), _stream_ptr()
    sel = op.get("sel")
    assert rows == (dt if sel is None else sel.numel())
    if store in ("plain", "sirt_add"):
        out = nan_out(oy, gx, gy) if store == "plain" else op["x"].clone()
        _lib.check(lib.ctpvae_siddon_bwd_prepared_f32(data.data_ptr(), oy, *g, ws.data_ptr(), ptr(op["colsum"]) if store == "sirt_add" else None,
                                                      out.data_ptr(), sp), "siddon_bwd_prepared")
        outs = (out,)
    elif store == "scaled":
        out = nan_out(oy, gx, gy)
        _lib.check(lib.ctpvae_siddon_bwd_sel_scaled_f32(data.data_ptr(), oy, *g, ptr(sel), rows, ws.data_ptr(), ptr(op.get("scale")),
                                                        int(op.get("stride", 0)), out.data_ptr(), sp), "siddon_bwd_sel_scaled")
        outs = (out,)
    elif store == "multiply":
        out = op["x"].clone()
        _lib.check(lib.ctpvae_siddon_bwd_sel_mul_f32(data.data_ptr(), oy, *g, ptr(sel), rows, ws.data_ptr(), op["colsum"].data_ptr(),
                                                     out.data_ptr(), sp), "siddon_bwd_sel_mul")
        outs = (out,)
    elif store == "pml":
        out = nan_out(oy, gx, gy)
        _lib.check(lib.ctpvae_siddon_bwd_sel_pml_f32(data.data_ptr(), oy, *g, ptr(sel), rows, ws.data_ptr(), op["colsum"].data_ptr(),
                                                     ctypes.c_float(op["beta"]), ctypes.c_float(op["delta"]), int(op["hybrid"]),
                                                     op["x"].data_ptr(), out.data_ptr(), sp), "siddon_bwd_sel_pml")
        outs = (out,)
    else:
        x = op["x"].clone()
        xbar, qx, qy = nan_out(oy, gx, gy), nan_out(oy, gx, gy), nan_out(oy, gx, gy)
        _lib.check(lib.ctpvae_siddon_bwd_tv_primal_f32(data.data_ptr(), oy, *g, ws.data_ptr(), op["tau"].data_ptr(), ctypes.c_float(op["lam"]),
                                                       x.data_ptr(), op["xbar"].data_ptr(), xbar.data_ptr(), op["qx"].data_ptr(),
                                                       op["qy"].data_ptr(), qx.data_ptr(), qy.data_ptr(), sp), "siddon_bwd_tv_primal")
        outs = (x, xbar, qx, qy)
    for t in outs:
        assert not torch.isnan(t).any(), f"{store}: an element was not written"
    return outs


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) or (torch.isnan(p).any() and np.array_equal(to_np(p), to_np(q), equal_nan=True))
                                    for p, q in zip(a, b))


# ---- operands --------------------------------------------------------------------------------------------------------------------
def fwd_operands(store, oy, grid, dx, dt, sel=None, seed=0):
    """Host operands of a forward store (float32 numpy; `sel` as a list) and the image."""
    positive = store in ("gaussian", "poisson", "ratio")
    x = tw.images(oy, grid, 100 + seed + oy, positive=positive)
    op = {}
    if store in ("sirt", "tv_dual"):
        op["meas"], op["w"] = tw.sinograms(oy, dt, dx, 200 + oy), tw.weights((dt, dx), 300 + oy)
        if store == "tv_dual":
            op["p"] = tw.sinograms(oy, dt, dx, 400 + oy)
    elif store == "ratio":
        op["meas"] = tw.sinograms(oy, dt, dx, 200 + oy, positive=True)
    elif store in ("gaussian", "poisson"):
        rng = np.random.default_rng(500 + oy)
        op["mask"] = rng.choice(np.asarray(tw.tg.MASKS, F), size=(oy, dt)).astype(F)
        op["meas"] = tw.sinograms(oy, dt, dx, 200 + oy, positive=True) * F(20.0)      # (overwritten below by counts of the ray-sums)
        op["pnm"] = np.asarray(PNM, F)
    if sel is not None and store in ("gaussian", "poisson", "ratio"):
        op["sel"] = np.asarray(sel, np.int32)
    return x, op


def on_device(op):
    return {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in op.items()}


def compact(op, sel):
    """The likelihood operands of a subset call in their COMPACT layout (dense = 0): mask [oy][n_sel], meas [oy][n_sel][dx] gathered
    on the host, the index operand kept -- the kernels then read row k, not table angle sel[k]."""
    return dict(op, sel=np.asarray(sel, np.int32), mask=np.ascontiguousarray(op["mask"][:, sel]),
                meas=np.ascontiguousarray(op["meas"][:, sel]), dense=0)


def counts_of(sim_dense, mask, store, seed):
    """Measurements near the model: Poisson counts of the masked ray-sums over pnm; for the Poisson store two samples are negative
    (outside the support: -inf on both sides)."""
    rng = np.random.default_rng(seed)
    meas = (rng.poisson(sim_dense.astype(np.float64) * mask[..., None] * PNM) / PNM).astype(F)
    if store == "poisson":
        meas.reshape(-1)[[5, meas.size // 2]] = -1.0
    return meas


# ---- forward against the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_forward_stores_against_the_twin(oracle, grid):
    """Ray-sums, SIRT update, ratio (dense and over the subset) and TV dual step at the library's own dispatch, for every slice
    count: the twin's bits.  One slice of (160, 258) is the global-memory form; the forms that ran are printed."""
    gx, gy = grid
    dx, th = tw.detector(grid), tw.angles()
    tables = hf._siddon_tables(th, dev())
    dt = th.size
    seen = set()
    for oy in SLICES:
        sims = {}
        for store in ("raysum", "sirt", "tv_dual", "ratio"):
            for sel in ((None, SUBSET) if store == "ratio" else (None,)):
                x, op = fwd_operands(store, oy, grid, dx, dt, sel)
                key = x.tobytes()
                if key not in sims:
                    sims[key] = tw.raysums(x, th, dx)
                sim = sims[key]
                rows = dt if sel is None else len(sel)
                seen.add((store, fwd_form(oy, grid, rows, dx, store)))
                got, = fwd(store, up(x), tables, dx, on_device(op))
                if store == "raysum":
                    want = sim
                    assert (want[0] == 0).any(), "some rays must miss the grid"
                elif store == "sirt":
                    want = tw.sirt_update(sim, op["meas"], op["w"])
                elif store == "tv_dual":
                    want = tw.tv_dual(op["p"], sim, op["meas"], op["w"])
                else:
                    want = tw.ratio(sim if sel is None else sim[:, sel], op["meas"] if sel is None else op["meas"][:, sel])
                np.testing.assert_array_equal(to_np(got), want, err_msg=f"{store} grid={grid} oy={oy} sel={sel}")
    print(f"forward stores, grid {grid}: (store, form) cells {sorted(seen)}")
    if grid == (160, 258):
        assert {("raysum", 0), ("sirt", 0), ("tv_dual", 0), ("ratio", 0)} <= seen


@pytest.mark.parametrize("noise", ["gaussian", "poisson"])
@pytest.mark.parametrize("grid", GRIDS)
def test_likelihood_stores_against_the_twin(oracle, grid, noise):
    """The grid as the object, pad True and False; the dense list, the subset with DENSE operands (read at the table angle) and the
    subset with COMPACT operands (gathered, read at the output row: the dense call's bits); ray-sums and derivative requested and
    not.  The Poisson derivative is six correctly rounded float32 operations (loglik_math.h poisson_dlogp; '/' is the IEEE
    quotient, no FMA contraction), so np_twin_poisson.twin_dlogp's BITS are expected, NaN and infinities included."""
    gx, gy = grid
    th = tw.angles()
    tables = hf._siddon_tables(th, dev())
    dt = th.size
    worst = {"lp/REL": 0.0, "lp/bar": 0.0, "dlp/bar": 0.0} if noise == "gaussian" else {"lp/bar": 0.0}
    seen = set()
    for pad in (True, False):
        dx = _lib.load().ctpvae_siddon_dx(gx, gy, 1 if pad else 0)
        for oy in (1, 5):
            x, op = fwd_operands(noise, oy, grid, dx, dt)
            sim = np.swapaxes(oracle.siddon_project(x, th, pad=pad), 0, 1)
            op["meas"] = counts_of(sim, op["mask"], noise, 600 + oy)
            for sel in (None, SUBSET):
                o = dict(op)
                if sel is not None:
                    o["sel"] = np.asarray(sel, np.int32)
                rows = dt if sel is None else len(sel)
                seen.add(fwd_form(oy, grid, rows, dx, noise))
                d_op = on_device(o)
                lp, sino, dlp = fwd(noise, up(x), tables, dx, d_op)
                lp_only, = fwd(noise, up(x), tables, dx, dict(d_op, want_sino=False, want_dlp=False))
                assert same((lp,), (lp_only,))
                s, m, y = (sim, op["mask"], op["meas"]) if sel is None else (sim[:, sel], op["mask"][:, sel], op["meas"][:, sel])
                np.testing.assert_array_equal(to_np(sino), s, err_msg=f"{noise} grid={grid} pad={pad} oy={oy} sel={sel}")
                if sel is not None:
                    c_op = on_device(compact(op, sel))
                    assert same(fwd(noise, up(x), tables, dx, c_op), (lp, sino, dlp)), (noise, grid, pad, oy, "compact with sel")
                    assert same(fwd(noise, up(x), tables, dx, dict(c_op, want_sino=False, want_dlp=False)), (lp,))
                if noise == "gaussian":
                    g = tw.gauss(s, m, y, PNM, EPS)
                    e_rel = rel_err(to_np(lp), g["lp_oracle"]) / REL
                    e_lp, k1 = tw.gauss_excess(to_np(lp), g["lp_ref"], g["lp_bar"])
                    e_dlp, k2 = tw.gauss_excess(to_np(dlp), g["dlp_ref"], g["dlp_bar"])
                    assert k1 and k2
                    worst = {"lp/REL": max(worst["lp/REL"], e_rel), "lp/bar": max(worst["lp/bar"], e_lp),
                             "dlp/bar": max(worst["dlp/bar"], e_dlp)}
                else:
                    want, atol, rtol = tw.poisson(s, m, y, PNM)
                    assert np.isneginf(want).sum() >= 1
                    e_lp, kind = tw.poisson_excess(to_np(lp), want, atol, rtol)
                    assert kind, "non-finite samples differ"
                    worst["lp/bar"] = max(worst["lp/bar"], e_lp)
                    np.testing.assert_array_equal(to_np(dlp), tw.tpo.twin_dlogp(s, m, y, PNM),
                                                  err_msg=f"poisson dlp grid={grid} pad={pad} oy={oy} sel={sel}")
    print(f"{noise} likelihood store, grid {grid}: forms {sorted(seen)}, worst error / bar {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- forward across forms --------------------------------------------------------------------------------------------------------
def _all_fwd_operands(store, oy, grid, dx, dt, tables):
    sel = SUBSET if store in ("gaussian", "poisson", "ratio") else None
    x, op = fwd_operands(store, oy, grid, dx, dt, sel)
    return up(x), on_device(op), (len(sel) if sel else dt)


@pytest.mark.parametrize("store", FWD_STORES)
def test_forward_forms_give_the_same_bits(store):
    """Every SIDDON_NS on every grid and slice count: the form that ran is asked from the library, the bits are those of
    SIDDON_NS = 1; the walk must have met every form the store has.  Then SIDDON_THREADS and SIDDON_PPB on the LDS and the
    global-memory forms."""
    th = tw.angles()
    tables = hf._siddon_tables(th, dev())
    dt = th.size
    seen = set()
    for grid in GRIDS:
        dx = tw.detector(grid)
        for oy in SLICES:
            x, op, rows = _all_fwd_operands(store, oy, grid, dx, dt, tables)
            with _lib.tuned("SIDDON_NS", 1):
                assert fwd_form(oy, grid, rows, dx, store) == (0 if grid == (160, 258) else 1)
                base = fwd(store, x, tables, dx, op)
            for ns in (1, 2, 4, 8, None):
                if ns is not None:
                    _lib.tune("SIDDON_NS", ns)
                try:
                    form = fwd_form(oy, grid, rows, dx, store)
                    got = fwd(store, x, tables, dx, op)
                finally:
                    _lib.tune("SIDDON_NS")
                lds = 0 if grid == (160, 258) else 1
                pair = 2 if oy >= 2 and grid[0] < 100 else lds
                want_form = {1: lds, 2: pair, 4: lds if store == "poisson" else 4, 8: lds if store == "poisson" else 8,
                             None: own_fwd_form(oy, grid, rows, dx, store)}[ns]
                assert form == want_form, (store, grid, oy, ns, form)
                seen.add(form)
                assert same(got, base), (store, grid, oy, ns, form)
    print(f"{store}: forms met {sorted(seen)}")
    assert seen == FWD_FORMS[store]
    for grid, ns, form in (((100, 258), 1, 1), ((12, 70), 2, 2), ((160, 258), 2, 0)):
        dx = tw.detector(grid)
        x, op, rows = _all_fwd_operands(store, 3, grid, dx, dt, tables)
        with _lib.tuned("SIDDON_NS", ns):
            assert fwd_form(3, grid, rows, dx, store) == form
            base = fwd(store, x, tables, dx, op)
            for threads in (64, 256, 1024):
                for ppb in (1, 3, 17):
                    with _lib.tuned("SIDDON_THREADS", threads), _lib.tuned("SIDDON_PPB", ppb):
                        assert same(fwd(store, x, tables, dx, op), base), (store, grid, threads, ppb)


# ---- back-projector --------------------------------------------------------------------------------------------------------------
def bwd_operands(store, oy, grid, dx, dt, seed=0):
    """(data [oy][rows][dx], host operands) of a back-projector store; the subset stores run over SUBSET."""
    gx, gy = grid
    rows = len(SUBSET) if store in ("scaled", "multiply", "pml") else dt
    positive = store in ("multiply", "pml")
    y = tw.sinograms(oy, rows, dx, 700 + seed + oy, positive=positive)
    op = {}
    if store in ("scaled", "multiply", "pml"):
        op["sel"] = np.asarray(SUBSET, np.int32)
    if store in ("sirt_add", "multiply"):
        op["colsum"] = tw.weights((gx, gy), 800 + oy)
        op["x"] = tw.images(oy, grid, 900 + oy, positive=positive)
    if store == "scaled":
        op["scale"], op["stride"] = np.random.default_rng(oy).uniform(0.5, 2.0, oy).astype(F), 1
    if store == "pml":
        op.update(colsum=tw.weights((gx, gy), 800 + oy) + F(0.5), x=tw.images(oy, grid, 900 + oy, positive=True), beta=0.3, delta=0.5, hybrid=1)
    if store == "tv_primal":
        op.update(tau=tw.weights((gx, gy), 800 + oy) * F(0.1), lam=0.05, x=tw.images(oy, grid, 900 + oy), xbar=tw.images(oy, grid, 901 + oy),
                  qx=tw.images(oy, grid, 902 + oy) * F(0.02), qy=tw.images(oy, grid, 903 + oy) * F(0.02))
    return y, op


@pytest.mark.parametrize("grid", GRIDS)
def test_backprojector_stores_against_the_twin(oracle, grid):
    """EPI 0, 1, 3 and 4 on the raw entry points at the library's own slices per workgroup, for every slice count."""
    gx, gy = grid
    dx, th = tw.detector(grid), tw.angles()
    tables = hf._siddon_tables(th, dev())
    dt = th.size
    bits = gx % 2 == 0 and gy % 2 == 0 and dx % 2 == 0
    worst, seen = {}, set()

    def check(tag, got, want):
        if bits:
            np.testing.assert_array_equal(to_np(got), want, err_msg=tag)
        worst[tag.split()[0]] = max(worst.get(tag.split()[0], 0.0), rel_err(to_np(got), want))

    for oy in SLICES:
        for store in ("plain", "sirt_add", "scaled", "multiply"):
            y, op = bwd_operands(store, oy, grid, dx, dt)
            t = th if "sel" not in op else th[SUBSET]
            bp = tw.backproject(y, t, gx, gy)
            seen.add((own_bwd_ns(oy), EPIS[store]))
            if store == "plain":
                check(f"plain oy={oy}", bwd(store, up(y), tables, grid, {})[0], bp)
                check(f"plain colsum=NULL/recon oy={oy}", rc.siddon_backproject(up(y), th, gx, gy), bp)
            elif store == "sirt_add":
                check(f"sirt_add oy={oy}", bwd(store, up(y), tables, grid, on_device(op))[0], tw.sirt_add(op["x"], bp, op["colsum"]))
            elif store == "multiply":
                check(f"multiply oy={oy}", bwd(store, up(y), tables, grid, on_device(op))[0], tw.multiply(op["x"], bp, op["colsum"]))
            else:
                d_op = on_device(op)
                check(f"scaled stride=1 oy={oy}", bwd(store, up(y), tables, grid, d_op)[0], tw.scaled(bp, op["scale"]))
                check(f"scaled stride=0 oy={oy}", bwd(store, up(y), tables, grid, dict(d_op, stride=0))[0], tw.scaled(bp, op["scale"][:1]))
                check(f"scaled none oy={oy}", bwd(store, up(y), tables, grid, {"sel": d_op["sel"]})[0], tw.scaled(bp))
    print(f"back-projector stores, grid {grid} ({'bits' if bits else 'REL'}): (NS, EPI) cells {sorted(seen)}, worst rel_err {worst}")
    assert all(v <= REL for v in worst.values()), worst


@pytest.mark.parametrize("algorithm", list(RECON))
def test_two_iterations_of_every_algorithm_against_its_twin(oracle, algorithm):
    """EPI 2 and 5 and the whole two-launch iterations through recon(...), the grid as num_gridx / num_gridy: 2 * REL."""
    th = tw.angles()
    kw = RECON[algorithm]
    worst = {}
    for grid in GRIDS:
        gx, gy = grid
        dx = tw.detector(grid)
        data = tw.sinograms(5, th.size, dx, 1000 + gx, positive=algorithm not in ("sirt", "tv"))
        got = to_np(recon(up(data), th, sinogram_order=True, algorithm=algorithm, num_iter=2, num_gridx=gx, num_gridy=gy, **kw))
        want = tw.recon(algorithm, data, th, 2, gx, gy, **kw)
        assert got.shape == want.shape == (5, gx, gy) and np.isfinite(got).all()
        worst[grid] = rel_err(got, want)
    print(f"recon {algorithm} num_iter=2: rel_err per grid {worst} (bound {2 * REL:.0e})")
    assert all(v <= 2 * REL for v in worst.values()), worst


@pytest.mark.parametrize("store", list(EPIS))
def test_backprojector_forms_give_the_same_bits(store):
    """SIDDON_BWD_NS x SIDDON_BWD_CHUNKS on every store, with slice counts that leave the last group part empty, on the ragged even
    grid and on the odd one (degenerate rays: the accumulator starts from their image)."""
    th = tw.angles()
    tables = hf._siddon_tables(th, dev())
    seen = set()
    for grid in GRIDS[:2]:
        dx = tw.detector(grid)
        for oy in (3, 5, 9):
            y, op = bwd_operands(store, oy, grid, dx, th.size)
            y, op = up(y), on_device(op)
            with _lib.tuned("SIDDON_BWD_NS", 1):
                base = bwd(store, y, tables, grid, op)
            for ns in (1, 2, 4, 8):
                for ch in (1, 4, None):
                    with _lib.tuned("SIDDON_BWD_NS", ns), _lib.tuned("SIDDON_BWD_CHUNKS", -1 if ch is None else ch):
                        got = bwd(store, y, tables, grid, op)
                    seen.add((ns, EPIS[store]))
                    assert same(got, base), (store, grid, oy, ns, ch)
            assert same(bwd(store, y, tables, grid, op), base), (store, grid, oy, "own dispatch")
            seen.add((own_bwd_ns(oy), EPIS[store]))
    assert seen == {(ns, EPIS[store]) for ns in (1, 2, 4, 8)}


# ---- chunked batches -------------------------------------------------------------------------------------------------------------
def test_chunked_batches_give_the_same_bits():
    """11 slices cut by MAX_SLICES = 4 (forward: chunks of 4, 4, 3 of the LDS / global-memory kernels -- the packed walk is not cut, so
    the large grids run with SIDDON_NS = 1; back-projector: chunks of whole groups) against the uncut call: every per-slice operand is
    re-based per chunk (likelihood masks and measurements: dense with the subset, compact with the subset, compact without; scale, TV
    state, PML ping-pong)."""
    th = tw.angles()
    tables = hf._siddon_tables(th, dev())
    dt = th.size
    for grid, ns in ((GRIDS[0], None), (GRIDS[1], None), (GRIDS[3], 1)):
        dx = tw.detector(grid)
        for store in FWD_STORES:
            likelihood = store in ("gaussian", "poisson")
            dense_bits = None
            for sel, layout in (((SUBSET, "dense"), (SUBSET, "compact"), (None, "compact")) if likelihood else ((SUBSET, "-"),)):
                x, op = fwd_operands(store, CHUNKED, grid, dx, dt, sel)
                if likelihood and sel is not None and layout == "compact":
                    op = compact(op, sel)
                x, op = up(x), on_device(op)
                rows = len(sel) if "sel" in op else dt
                if ns is not None:
                    _lib.tune("SIDDON_NS", ns)
                try:
                    assert fwd_form(CHUNKED, grid, rows, dx, store) < 4
                    want = fwd(store, x, tables, dx, op)
                    with _lib.tuned("MAX_SLICES", 4):
                        got = fwd(store, x, tables, dx, op)
                finally:
                    _lib.tune("SIDDON_NS")
                assert same(got, want), (store, grid, sel, layout)
                if likelihood and sel is not None:      # gathered operands at the output row = dense operands at the table angle
                    dense_bits = want if layout == "dense" else dense_bits
                    assert same(got, dense_bits), (store, grid, layout)
    for grid in GRIDS[:2]:
        dx = tw.detector(grid)
        for store in EPIS:
            y, op = bwd_operands(store, CHUNKED, grid, dx, dt)
            y, op = up(y), on_device(op)
            want = bwd(store, y, tables, grid, op)
            for bns in (None, 2):           # own dispatch: chunks of 8 and 3; pairs: chunks of 4, 4, 3
                with _lib.tuned("MAX_SLICES", 4), _lib.tuned("SIDDON_BWD_NS", -1 if bns is None else bns):
                    got = bwd(store, y, tables, grid, op)
                assert same(got, want), (store, grid, bns)


@pytest.mark.parametrize("algorithm", list(RECON))
def test_chunked_recon_gives_the_same_bits(algorithm):
    th = tw.angles()
    gx, gy = grid = GRIDS[1]
    dx = tw.detector(grid)
    data = up(tw.sinograms(CHUNKED, th.size, dx, 1100, positive=algorithm not in ("sirt", "tv")))
    kw = dict(sinogram_order=True, algorithm=algorithm, num_iter=2, num_gridx=gx, num_gridy=gy, **RECON[algorithm])
    assert fwd_form(CHUNKED, grid, th.size, dx, "ratio") < 4
    want = recon(data, th, **kw)
    with _lib.tuned("MAX_SLICES", 4):
        got = recon(data, th, **kw)
    assert torch.equal(got, want) and torch.isfinite(got).all()


@pytest.mark.parametrize("noise", ["gaussian", "poisson"])
def test_chunked_training_call_gives_the_same_bits(noise):
    """calculate_log_prob_M_given_R(model="siddon") with .backward(): the fused forward's dense operands with `sel`, and the scaled
    transpose with its per-slice factor, cut into chunks."""
    th = tw.angles()
    gx, gy = grid = GRIDS[1]
    dx = _lib.load().ctpvae_siddon_dx(gx, gy, 1)
    x, op = fwd_operands(noise, CHUNKED, grid, dx, th.size)
    mask = up(np.random.default_rng(12).uniform(0.02, 0.08, (CHUNKED, th.size)).astype(F))
    meas = up(tw.sinograms(CHUNKED, th.size, dx, 1200, positive=True) * F(0.5))
    w = torch.linspace(0.5, 2.0, CHUNKED, device=dev())

    def call(reduce):
        xr = up(x[..., None]).requires_grad_(True)
        out = cp.calculate_log_prob_M_given_R(xr, mask, meas, PNM, EPS, theta=th, angles_i=SUBSET, pad=True, model="siddon", noise=noise,
                                              reduce=reduce)
        ((out * w).sum() if reduce else (out.sum(dim=(1, 2, 3)) * w).sum()).backward()
        return out.detach(), xr.grad
    for reduce in (None, "per_object"):
        assert fwd_form(CHUNKED, grid, len(SUBSET), dx, noise) < 4
        want = call(reduce)
        with _lib.tuned("MAX_SLICES", 4):
            got = call(reduce)
        assert same(got, want) and (noise == "poisson" or torch.isfinite(want[1]).all()), (noise, reduce)
        assert not torch.equal(want[1], torch.zeros_like(want[1]))
