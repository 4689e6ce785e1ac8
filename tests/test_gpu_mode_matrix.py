"""The host dispatch of RotatePlan in all four (interpolation x backward) modes against the CPU oracle, on a real MI355X.

test_gpu_parity.py::test_dispatch_matrix_against_the_oracle walks the nearest / tf_compat dispatch cell by cell;
test_gpu_bilinear.py tests the bilinear and exact kernels one at a time.  This file walks the host code around them: every
public entry point, in each mode, on geometries that fit LDS (padded, unpadded) and tiled ones, with dense, device-resident
and host-resident angle subsets, and after each call history that changes which kernel a plan picks (the first forward
turns the tile workspace off on slices that fit LDS; a subset call builds plans; _cached_plan hands out a used plan).

Bars:
  * forward, both interpolations: the oracle's bits (tiled geometries: its tile-by-tile sum);
  * tf_compat backward (raw, subset, autograd, the drop-in layouts): the oracle's bits;
  * exact backward: <= 1e-5 of the oracle's scatter, equal bits run to run, across every call history and to the backward
    of a plan freshly built for the gathered table rows, and the transpose of the forward (float64 inner products);
  * forward_loglik / forward_loglik_sums (nearest): log-probabilities <= 1e-5 of the oracle, per-object sums the oracle's
    ordered sum of the kernel's own log-probabilities, bit for bit;
  * what a mode does not support (the likelihood entry points on a bilinear plan, a per-slice backward scale outside nearest
    / tf_compat) raises ValueError before anything is launched."""
import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import forward_functions as ff
from ct_pvae_amd.forward_functions import RotatePlan

pytestmark = pytest.mark.gpu

REL = 1e-5
MODES = [("nearest", "tf_compat"), ("nearest", "exact"), ("bilinear", "tf_compat"), ("bilinear", "exact")]
# (H, W), pad, A, S: fits LDS padded and not square; fits LDS unpadded and odd; tiled where the bilinear tile workspace is
# smaller than the nearest one; tiled at the project's size
GEOMETRIES = [((120, 140), True, 11, 5), ((97, 65), False, 7, 3), ((384, 384), True, 5, 2), ((512, 512), True, 5, 2)]
HISTORIES = ("fresh", "after_forward", "after_subset", "cached")
FORMS = ("dense", "device", "host")
LAYOUTS = ("vae", "dim3", "dim2", "low_mem")


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def _mode_matrix_cells():
    """(entry point, angle form, call history) -- every cell of a mode on a geometry (the bars depend on the mode)."""
    cells = []
    for hist in HISTORIES:
        for form in FORMS:
            cells += [("forward", form, hist), ("backward", form, hist), ("forward_loglik", form, hist),
                      ("forward_loglik_sums", form, hist), ("backward_scale", form, hist)]
            if form != "dense":
                cells.append(("subset", form, hist))            # plan.subset(idx).forward / .backward
        cells.append(("apply", "dense", hist))
    for layout in LAYOUTS:                                       # project_tf_fast / project_tf_low_mem: built, then cached
        cells += [(layout, "dense", "fresh"), (layout, "dense", "cached")]
    return cells


def _is_launch(name):
    """A projector or likelihood launch of the library (size / support queries and plan builds are not)."""
    return (name.startswith(("ctpvae_rotate_fwd_", "ctpvae_rotate_bwd_", "ctpvae_loglik_")) and name.endswith("_f32")
            and not name.endswith("_build_f32"))


class _NoLaunch:
    """The library, with every launch replaced by an AssertionError: a call that must be refused with a ValueError must be
    refused before it launches anything (an unsupported mode can mean a wrong kernel or a workspace of the wrong size)."""

    def __init__(self, lib):
        self._real = lib

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not _is_launch(name):
            return fn

        def refused(*args, **kwargs):
            raise AssertionError(f"{name} was launched by a call that must raise ValueError first")
        return refused


@pytest.mark.parametrize("interp,backward", MODES)
@pytest.mark.parametrize("shape,pad,A,S", GEOMETRIES)
def test_mode_matrix_against_the_oracle(oracle, torch_node, monkeypatch, interp, backward, shape, pad, A, S):
    """Every (entry point x angle form x call history) cell of one (interpolation, backward) mode on one geometry against the
    oracle, each cell on a plan of its own.  An exact subset is the gather a plan built for the gathered table rows runs, in
    every history (the parent's state once chose the scatter kernel: atomics, bits not fixed); the likelihood entry points of
    a bilinear plan raise before any launch (a tiled bilinear plan once ran the NEAREST tile kernel in the smaller bilinear
    workspace)."""
    d = dev()
    H, W = shape
    icode = oracle.NEAREST if interp == "nearest" else oracle.BILINEAR
    exact = backward == "exact"
    rng = np.random.default_rng(H * 7 + A + icode * 3 + int(exact))
    theta = rng.uniform(-1.0, 4.0, A).astype(np.float32)
    theta[0], theta[2] = 0.0, np.pi / 2                        # the subset below takes 0 once and pi / 2 twice
    sub = np.array([A - 1, 2, 0, 2], np.int32)                 # any order, a repeat
    geom = oracle.Geometry(H, W, pad)
    PW = geom.PW
    tiled = RotatePlan(theta, H, W, pad, d, interp=interp).tiled      # (a throwaway plan: .tiled has a side effect)
    assert tiled == (H * W > 200 * 200)
    mk = dict(interp=interp, backward=backward)
    # _cached_plan's caches, empty and private to this test: "fresh" and "cached" mean what they say
    for name in ("_PLAN_CACHE", "_HOST_THETA_PLANS", "_DEV_THETA_PLANS"):
        monkeypatch.setattr(ff, name, {})

    # ---- references ----
    T = oracle.rotate_transforms(theta, geom.PH, geom.PW)
    Tinv = oracle.invert_transforms(T)
    img = rng.random((S, H, W), dtype=np.float32)
    x = torch.from_numpy(img).to(d)

    def fwd_ref(TT, im=img):
        if tiled:
            return oracle.rotate_fwd_tiled(im, geom, TT, oracle.tile_shape(H, W, icode), interp=icode)
        return oracle.rotate_fwd(im, geom, TT, icode)

    T8d, Tinv8d = ff.rotate_tables(theta, geom.PH, geom.PW, d)
    rows = {"dense": slice(None), "sub": sub, "dense1": slice(None)}
    R = {}
    for kind, nimg in (("dense", S), ("sub", S), ("dense1", 1)):
        TT, TTi = T[rows[kind]], Tinv[rows[kind]]
        g = (rng.standard_normal((nimg, TT.shape[0], PW)) + 0.25).astype(np.float32)     # mean != 0: <Ax, g> far from 0
        ref = dict(sino=fwd_ref(TT, img[:nimg]), g=g, gt=torch.from_numpy(g).to(d), img=img[:nimg])
        if exact:
            ref["gimg"] = oracle.rotate_bwd_exact(g, geom, TT, icode)
            idx = torch.arange(A, device=d) if kind != "sub" else torch.from_numpy(sub).to(d).long()
            fresh = RotatePlan(None, H, W, pad, d, **mk, _tables=(T8d.index_select(0, idx), Tinv8d.index_select(0, idx)))
            ref["fresh"] = fresh.backward(ref["gt"])
        else:
            ref["gimg"] = oracle.rotate_bwd_tfcompat(g, geom, TTi, icode)
        R[kind] = ref
    mask = rng.uniform(0.01, 0.1, (S, A)).astype(np.float32)
    meas = (rng.random((S, A, PW), dtype=np.float32) * 3).astype(np.float32)
    mask_t, meas_t = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    pnm, eps = torch.tensor([1e4], device=d), 1.2e-7
    lp_ref = {"dense": oracle.loglik(R["dense"]["sino"], mask, meas, 1e4, eps),
              "sub": oracle.loglik(R["sub"]["sino"], mask[:, sub], meas[:, sub], 1e4, eps)}
    w = torch.from_numpy(rng.uniform(0.5, 2.0, S).astype(np.float32)).to(d)
    idx_dev = torch.from_numpy(sub).to(d)
    exact_bits = {}        # kind -> the first exact gradient: every later one, in every history and entry point, equals it

    def sel_of(form):
        if form == "dense":
            return None
        return idx_dev if form == "device" else cp.as_angle_index(sub, d, keep_host=True)

    def check_fwd(got, kind, tag):
        np.testing.assert_array_equal(to_np(got), R[kind]["sino"], err_msg=str(tag))

    def check_bwd(got, kind, tag, again=None):
        """got: the gradient image of cotangent R[kind]["g"]; again: a second run of the same call (exact mode)."""
        ref = R[kind]
        if not exact:
            np.testing.assert_array_equal(to_np(got), ref["gimg"], err_msg=str(tag))
            return
        assert rel_err(to_np(got), ref["gimg"]) <= REL, "exact backward further than 1e-5 from the oracle"
        if again is not None:
            assert torch.equal(again, got), "exact backward differs run to run"
        assert torch.equal(got, ref["fresh"]), "exact backward differs from a fresh plan of the gathered rows"
        first = exact_bits.setdefault(kind, got)
        assert torch.equal(got, first), "exact backward differs from another history / entry point"
        lhs = float((ref["sino"].astype(np.float64) * ref["g"]).sum())
        rhs = float((ref["img"].astype(np.float64) * to_np(got).astype(np.float64)).sum())
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), f"<Ax, g> = {lhs} but <x, A^T g> = {rhs}"

    def prime(hist):
        """A plan of this mode in call history `hist`."""
        if hist == "cached":
            for cache in (ff._PLAN_CACHE, ff._HOST_THETA_PLANS, ff._DEV_THETA_PLANS):
                cache.clear()
            x4 = x[..., None].clone().requires_grad_(True)
            cp.project_tf_fast(x4, theta, pad=pad, dim=2, integrate_vae=True, **mk).backward(R["dense"]["gt"][..., None])
            plan = ff._cached_plan(theta, H, W, pad, d, interp, backward)
            assert len(ff._PLAN_CACHE) == 1 and ff._cached_plan(theta, H, W, pad, d, interp, backward) is plan
            return plan
        plan = RotatePlan(theta, H, W, pad, d, **mk)
        if hist == "after_forward":
            plan.forward(x)
        elif hist == "after_subset":
            plan.forward(x, angles_i=idx_dev)
            plan.backward(R["sub"]["gt"], angles_i=idx_dev)
        return plan

    def refused(plan, call):
        """call() raises ValueError with the library's launches replaced -- here and in any plan it builds (subset())."""
        proxy = _NoLaunch(plan._lib)
        with monkeypatch.context() as m:
            m.setattr(ff._lib, "load", lambda: proxy)
            m.setattr(plan, "_lib", proxy)
            try:
                call()
            except ValueError:
                return
        raise AssertionError("no ValueError")

    assert _is_launch("ctpvae_rotate_fwd_tiled_compact_f32") and _is_launch("ctpvae_loglik_object_sums_f32")
    assert not any(_is_launch(n) for n in ("ctpvae_rotate_fwd_tiled_workspace_bytes", "ctpvae_loglik_part_floats",
                                           "ctpvae_rotate_bwd_step_plan_build_f32", "ctpvae_rotate_exact_wplan_build_f32"))
    def run_cell(entry, form, hist, tag):
        if entry in LAYOUTS:
            run_layout(entry, hist, tag)
            return
        plan = prime(hist)
        sel = sel_of(form)
        kind = "dense" if sel is None else "sub"
        if entry == "forward":
            check_fwd(plan.forward(x, angles_i=sel), kind, tag)
        elif entry == "backward":
            got = plan.backward(R[kind]["gt"], angles_i=sel)
            check_bwd(got, kind, tag, again=plan.backward(R[kind]["gt"], angles_i=sel) if exact else None)
        elif entry == "subset":
            sp = plan.subset(sel)
            check_fwd(sp.forward(x), "sub", tag)
            got = sp.backward(R["sub"]["gt"])
            check_bwd(got, "sub", tag, again=sp.backward(R["sub"]["gt"]) if exact else None)
        elif entry == "apply":
            xr = x.clone().requires_grad_(True)
            out = plan.apply(xr)
            check_fwd(out, "dense", tag)
            out.backward(R["dense"]["gt"])
            check_bwd(xr.grad, "dense", tag)
        elif entry in ("forward_loglik", "forward_loglik_sums"):
            args = (x, mask_t, meas_t, pnm, eps)
            kw = dict(angles_i=sel, dense_inputs=sel is not None)
            if interp != "nearest":
                refused(plan, lambda: getattr(plan, entry)(*args, **kw))
            elif entry == "forward_loglik":
                sino, lp = plan.forward_loglik(*args, **kw)
                check_fwd(sino, kind, tag)
                assert rel_err(to_np(lp), lp_ref[kind]) <= REL, "log-probabilities further than 1e-5 from the oracle"
            else:
                sums, _ = plan.forward_loglik_sums(*args, **kw)
                _, lp_k = plan.forward_loglik(*args, **kw)           # the kernel's own log-probabilities
                assert rel_err(to_np(lp_k), lp_ref[kind]) <= REL, "log-probabilities further than 1e-5 from the oracle"
                np.testing.assert_array_equal(to_np(sums), oracle.loglik_object_sums(to_np(lp_k), 1 if tiled else 0),
                                              err_msg=str(tag))
        elif entry == "backward_scale":
            if (interp, backward) != ("nearest", "tf_compat"):
                refused(plan, lambda: plan.backward(R[kind]["gt"], scale=w, angles_i=sel))
            else:
                got = plan.backward(R[kind]["gt"], scale=w, angles_i=sel)
                np.testing.assert_array_equal(to_np(got), to_np(w)[:, None, None] * R[kind]["gimg"], err_msg=str(tag))
        else:
            raise AssertionError(f"unknown cell {tag}")

    def run_layout(layout, hist, tag):
        """The drop-in calls: "fresh" builds the plan, "cached" (the next cell) is handed the same plan by _cached_plan."""
        if hist == "fresh":
            for cache in (ff._PLAN_CACHE, ff._HOST_THETA_PLANS, ff._DEV_THETA_PLANS):
                cache.clear()
        if layout == "vae":
            xi = x[..., None].clone().requires_grad_(True)
            out = cp.project_tf_fast(xi, theta, pad=pad, dim=2, integrate_vae=True, **mk)
            sino, kind = out[..., 0], "dense"
            out.backward(R[kind]["gt"][..., None])
            gimg = xi.grad[..., 0]
        elif layout == "dim2":
            xi = x[0].clone().requires_grad_(True)
            out = cp.project_tf_fast(xi, theta, pad=pad, dim=2, **mk)                    # [A][P][1]
            sino, kind = out.permute(2, 0, 1), "dense1"
            out.backward(R[kind]["gt"].permute(1, 2, 0))
            gimg = xi.grad[None]
        else:
            xi = x.permute(1, 2, 0).contiguous().requires_grad_(True)                    # [X][Y][Z]
            if layout == "dim3":
                out = cp.project_tf_fast(xi, theta, pad=pad, dim=3, **mk)
            else:
                out = cp.project_tf_low_mem(xi, theta, pad=pad, **mk)
            sino, kind = out.permute(2, 0, 1), "dense"
            out.backward(R[kind]["gt"].permute(1, 2, 0))
            gimg = xi.grad.permute(2, 0, 1)
        assert len(ff._PLAN_CACHE) == 1, tag
        check_fwd(sino, kind, tag)
        check_bwd(gimg.contiguous(), kind, tag)

    # every cell runs; the failures are reported together (an error that is not a failed check ends the test at once)
    seen, failures = set(), []
    for cell in _mode_matrix_cells():
        tag = (interp, backward, shape) + cell
        try:
            run_cell(*cell, tag)
        except AssertionError as e:
            failures.append(f"{tag}: " + " | ".join([ln.strip() for ln in str(e).splitlines() if ln.strip()][:3]))
        seen.add(cell)
    missing = set(_mode_matrix_cells()) - seen
    assert not missing, f"cells that did not run: {sorted(missing)}"
    assert not failures, f"{len(failures)} of {len(seen)} cells failed:\n" + "\n".join(failures)
