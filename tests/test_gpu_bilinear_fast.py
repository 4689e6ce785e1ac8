"""precision="fast": the bilinear forward's lerp / FMA instantiation (rotate_fwd_bilin_kernel<..., FAST>) on a real MI355X.

The fast kernel takes the exact kernel's samples -- coordinates, floors, ownership, taps, row order -- and blends the four taps
as three fused lerps instead of TensorFlow's ten unfused operations.  Bars:
  * against the CPU oracle (the exact blend)           <= 1e-5 of the sinogram's maximum (REL of tests/test_gpu_bilinear.py, the
                                                        project's north star), for the library's choice and every forced form;
  * run to run, and between the forms of one association: equal bits.  Every whole-slice form (1 / 2 / 4 slices per cell, plain /
    sorted / row-split tasks) adds a ray's rows in canvas-row order, and a row this form visits and that one does not adds +0
    (fma(w, 0 - 0, 0)), so ALL whole-slice forms share one association and must agree to the bit; tiles add per-tile partial sums
    and agree among themselves (slices per cell, sorted or not);
  * the fast result is NOT bit-equal to the exact one (else the flag is not wired through);
  * precision="exact" and no keyword: the oracle's bits, also after fast launches in the same process;
  * the backward of a fast plan: the exact plan's bits (the same kernels)."""
import contextlib
import os

import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib, phantoms
from ct_pvae_amd.forward_functions import RotatePlan

pytestmark = pytest.mark.gpu
REL = 1e-5


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def oT(oracle, theta, plan):
    return oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW)


def fuzz_cases(rng, n):
    """(H, W, pad, theta, S): the generator of tests/test_gpu_bilinear.py -- odd sizes, one-pixel slices, unpadded canvases,
    axis-aligned angles, 1..7 slices."""
    fixed = [(1, 1), (1, 77), (93, 1), (3, 2), (2, 2), (128, 128), (129, 127), (64, 160)]
    for case in range(n):
        H, W = fixed[case] if case < len(fixed) else (int(rng.integers(1, 150)), int(rng.integers(1, 150)))
        pad, A, S = bool(rng.integers(0, 2)), int(rng.integers(1, 25)), int(rng.integers(1, 8))
        theta = rng.uniform(-2 * np.pi, 2 * np.pi, A)
        if case % 3 == 0:
            theta[: min(A, 4)] = [0.0, np.pi / 2, np.pi, -np.pi / 2][: min(A, 4)]
        yield case, H, W, pad, theta, S


def fast_plan(theta, H, W, pad, d, **kw):
    return RotatePlan(theta, H, W, pad, d, interp="bilinear", precision="fast", **kw)


def test_fast_forward_random_geometries_every_forced_form(oracle):
    d = dev()
    rng = np.random.default_rng(int(os.environ.get("CTPVAE_FUZZ_SEED", 20261005)))
    worst = (0.0, "")
    for case, H, W, pad, theta, S in fuzz_cases(rng, int(os.environ.get("CTPVAE_FUZZ_CASES", 28))):
        img = rng.standard_normal((S, H, W)).astype(np.float32)
        geom = oracle.Geometry(H, W, pad)
        plan = fast_plan(theta, H, W, pad, d)
        want = oracle.rotate_fwd(img, geom, oT(oracle, theta, plan), 1)
        x = torch.from_numpy(img).to(d)
        msg = f"case {case}: {H}x{W} pad={pad} A={len(theta)} S={S}"

        def check(form):
            got = plan.forward(x)
            e = rel_err(to_np(got), want)
            nonlocal worst
            worst = max(worst, (e, form + " " + msg))
            assert e <= REL, (e, form, msg)             # (a NaN -- an output a launch skipped -- fails this too)
            assert torch.equal(got, first), ("whole-slice forms share one association", form, msg)

        first = plan.forward(x)
        check("library's choice")
        for ns in (1, 2, 4):
            with _lib.tuned("BNS", ns):
                check(f"BNS={ns}")
                for bsort in (0, 1):
                    with _lib.tuned("BSORT", bsort):
                        check(f"BNS={ns} BSORT={bsort}")
                for rsplit in (0, 1):
                    with _lib.tuned("BSORT", 0), _lib.tuned("BRSPLIT", rsplit):
                        check(f"BNS={ns} BRSPLIT={rsplit}")
    print("worst rel err of the fast forward against the oracle:", worst)


@pytest.mark.parametrize("S,A", [(50, 20), (50, 180)])
def test_fast_forward_full_sizes(oracle, S, A):
    """The headline shape and the dense 180-angle shape (sorted band tasks, several chunks) against the oracle."""
    d = dev()
    rng = np.random.default_rng(S + A)
    theta = phantoms.dense_theta(180)[:: 180 // A][:A]
    img = rng.standard_normal((S, 128, 128)).astype(np.float32)
    plan = fast_plan(theta, 128, 128, True, d)
    want = oracle.rotate_fwd(img, oracle.Geometry(128, 128, True), oT(oracle, theta, plan), 1)
    x = torch.from_numpy(img).to(d)
    got = plan.forward(x)
    e = rel_err(to_np(got), want)
    print(f"{S} x 128^2 x {A}: rel err {e:.3e}")
    assert e <= REL, e
    for bsort, G in ((0, -1), (1, 1), (1, 5), (0, 3)):
        with _lib.tuned("BSORT", bsort), _lib.tuned("BW", G):
            assert torch.equal(plan.forward(x), got), f"BSORT={bsort} G={G}"


@pytest.mark.parametrize("H,W,S,A", [(512, 512, 3, 6), (300, 200, 5, 4), (190, 260, 2, 5)])
def test_fast_tiles_against_the_untiled_oracle(oracle, H, W, S, A):
    """Slices larger than LDS: the tile kernel's fast twin and the reduce pass, against the UNTILED oracle sum (the sizes and
    rng.random pixels of test_bilinear_tiles_against_the_tiled_oracle, for which the exact tiled kernel stays within the bar)."""
    d = dev()
    rng = np.random.default_rng(H + W)
    theta = np.concatenate([[0.0, np.pi / 2], rng.uniform(0, np.pi, A - 2)])
    img = rng.random((S, H, W)).astype(np.float32)
    geom = oracle.Geometry(H, W, True)
    plan = fast_plan(theta, H, W, True, d)
    assert plan.tiled
    x = torch.from_numpy(img).to(d)
    got = plan.forward(x)
    e = rel_err(to_np(got), oracle.rotate_fwd(img, geom, oT(oracle, theta, plan), 1))
    print(f"tiles {H}x{W}: rel err {e:.3e}")
    assert e <= REL, e
    exact = RotatePlan(theta, H, W, True, d, interp="bilinear").forward(x)
    assert not torch.equal(got, exact)
    for ns in (1, 2, 4):
        for bsort in (0, 1):
            with _lib.tuned("BNS", ns), _lib.tuned("BSORT", bsort):
                assert torch.equal(plan.forward(x), got), f"BNS={ns} BSORT={bsort}"


def test_fast_forced_tiles_on_small_unpadded_slices(oracle):
    """TILED_FORCE cuts slices that fit LDS into tiles: ragged edge tiles, one-row tiles, unpadded canvases (white noise)."""
    d = dev()
    rng = np.random.default_rng(11)
    for H, W, pad in ((150, 100, True), (97, 65, False), (130, 129, False), (64, 64, True), (1, 200, True)):
        theta = rng.uniform(-np.pi, np.pi, 5)
        img = rng.standard_normal((3, H, W)).astype(np.float32)
        geom = oracle.Geometry(H, W, pad)
        x = torch.from_numpy(img).to(d)
        with _lib.tuned("TILED_FORCE", 1):
            plan = fast_plan(theta, H, W, pad, d)
            assert plan.tiled
            got = plan.forward(x)
            for bsort in (0, 1):
                with _lib.tuned("BSORT", bsort):
                    assert torch.equal(plan.forward(x), got), f"BSORT={bsort}"
        e = rel_err(to_np(got), oracle.rotate_fwd(img, geom, oT(oracle, theta, plan), 1))
        assert e <= REL, (e, H, W, pad)


@pytest.mark.parametrize("S,A", [(300, 20), (151, 180)])
def test_fast_forward_long_launches(oracle, S, A):
    """Batches whose workgroups come in several rounds: no output left NaN, one task group per class gives the same bits, the
    oracle on a few slices."""
    d = dev()
    rng = np.random.default_rng(S + A)
    theta = phantoms.dense_theta(180)[:: 180 // A][:A]
    img = rng.standard_normal((S, 128, 128)).astype(np.float32)
    plan = fast_plan(theta, 128, 128, True, d)
    x = torch.from_numpy(img).to(d)
    got = plan.forward(x)
    assert not bool(torch.isnan(got).any())
    with _lib.tuned("BW", 1):
        assert torch.equal(plan.forward(x), got)
    pick = [0, S // 2, S - 1]
    want = oracle.rotate_fwd(img[pick], oracle.Geometry(128, 128, True), oT(oracle, theta, plan), 1)
    assert rel_err(to_np(got[pick]), want) <= REL


def test_fast_is_another_kernel_deterministic_and_the_default_did_not_move(oracle):
    d = dev()
    rng = np.random.default_rng(50)
    theta = phantoms.dense_theta(180)[phantoms.sparse_angle_indices(180, 20)]
    img = rng.standard_normal((50, 128, 128)).astype(np.float32)
    geom = oracle.Geometry(128, 128, True)
    x = torch.from_numpy(img).to(d)
    fast = fast_plan(theta, 128, 128, True, d)
    exact = RotatePlan(theta, 128, 128, True, d, interp="bilinear", precision="exact")
    plain = RotatePlan(theta, 128, 128, True, d, interp="bilinear")
    assert fast.forward_kernel_name(50) != exact.forward_kernel_name(50) == plain.forward_kernel_name(50)
    want = oracle.rotate_fwd(img, geom, oT(oracle, theta, exact), 1)
    got_f = fast.forward(x)
    assert torch.equal(got_f, fast.forward(x)), "run to run"
    for ns in (1, 2, 4):                       # every whole-slice form adds a ray's rows in canvas order: one association
        for knobs in ((("BSORT", 0), ("BRSPLIT", 0)), (("BSORT", 0), ("BRSPLIT", 1)), (("BSORT", 1),)):
            with contextlib.ExitStack() as stack:
                stack.enter_context(_lib.tuned("BNS", ns))
                for k, v in knobs:
                    stack.enter_context(_lib.tuned(k, v))
                assert torch.equal(fast.forward(x), got_f), (ns, knobs)
    assert rel_err(to_np(got_f), want) <= REL
    # exact launches AFTER fast ones, interleaved: the oracle's bits, with and without the keyword
    got_e = exact.forward(x)
    assert not torch.equal(got_f, got_e), "the fast plan ran the exact kernel"
    np.testing.assert_array_equal(to_np(got_e), want)
    assert torch.equal(fast.forward(x), got_f)
    np.testing.assert_array_equal(to_np(plain.forward(x)), want)
    # ... and through the drop-in call, whose plan cache is keyed on the precision
    xz = torch.from_numpy(np.ascontiguousarray(img[:3].transpose(1, 2, 0))).to(d)
    out_f = cp.project_tf_low_mem(xz, theta, pad=True, precision="fast")
    out_e = cp.project_tf_low_mem(xz, theta, pad=True, precision="exact")
    out_p = cp.project_tf_low_mem(xz, theta, pad=True)
    out_f2 = cp.project_tf_fast(xz, theta, pad=True, interp="bilinear", precision="fast")
    assert torch.equal(out_e, out_p) and not torch.equal(out_f, out_e) and torch.equal(out_f, out_f2)
    np.testing.assert_array_equal(to_np(out_e), want[:3].transpose(1, 2, 0))
    assert torch.equal(out_f, got_f[:3].permute(1, 2, 0)), "a slice's fast sinogram does not depend on its batch"


def test_fast_slice_independence_subsets_and_autograd(oracle):
    d = dev()
    rng = np.random.default_rng(3)
    theta = phantoms.dense_theta(180)[::12]
    A = len(theta)
    img = rng.standard_normal((9, 128, 128)).astype(np.float32)
    x = torch.from_numpy(img).to(d)
    plan = fast_plan(theta, 128, 128, True, d)
    full = plan.forward(x)
    for S in (1, 2, 3, 5, 9):
        assert torch.equal(plan.forward(x[:S].contiguous()), full[:S]), f"S={S}"
    # angle subsets: equal to a plan built for the gathered angles, and still the fast kernel
    sub = np.array([7, 0, 3, 3, 8])
    gathered = fast_plan(theta[sub], 128, 128, True, d).forward(x)
    exact_sub = RotatePlan(theta[sub], 128, 128, True, d, interp="bilinear").forward(x)
    for where in ("device", "host"):
        idx = cp.as_angle_index(sub, d, keep_host=(where == "host"))
        assert plan.subset(idx).precision == "fast"
        got = plan.forward(x, angles_i=idx)
        assert torch.equal(got, gathered), where
        assert not torch.equal(got, exact_sub), where
    # autograd through the drop-in call: the gradient is the exact plan's, bit for bit, in both backward modes
    xz0 = np.ascontiguousarray(img[:5].transpose(1, 2, 0))
    geom = oracle.Geometry(128, 128, True)
    gz = rng.standard_normal((A, geom.PW, 5)).astype(np.float32)
    gzt = torch.from_numpy(gz).to(d)
    for back in ("tf_compat", "exact"):
        grads = {}
        for prec in ("fast", "exact"):
            xz = torch.from_numpy(xz0).to(d).requires_grad_(True)
            out = cp.project_tf_low_mem(xz, theta, pad=True, backward=back, precision=prec)
            out.backward(gzt)
            grads[prec] = (xz.grad, out.detach())
        assert torch.equal(grads["fast"][0], grads["exact"][0]), back
        assert not torch.equal(grads["fast"][1], grads["exact"][1]), back
        if back == "exact":   # <A_fast x, g> against <x, A^T g> of the exact adjoint
            lhs = float((to_np(grads["fast"][1]).astype(np.float64) * gz).sum())
            rhs = float((to_np(grads["exact"][0]).astype(np.float64) * xz0).sum())
            assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    # the raw operator pair of a fast plan: backward bits of an exact plan
    g = torch.from_numpy(rng.standard_normal((9, A, geom.PW)).astype(np.float32)).to(d)
    for back in ("tf_compat", "exact"):
        pf, pe = fast_plan(theta, 128, 128, True, d, backward=back), RotatePlan(theta, 128, 128, True, d, interp="bilinear", backward=back)
        assert pf.backward_kernel_name(9) == pe.backward_kernel_name(9)
        assert torch.equal(pf.backward(g), pe.backward(g)), back


def test_fast_refusals_come_before_any_launch():
    d = dev()
    theta = np.linspace(0.0, np.pi, 6, endpoint=False)
    with pytest.raises(ValueError, match="bilinear"):
        RotatePlan(theta, 32, 32, True, d, interp="nearest", precision="fast")
    with pytest.raises(ValueError, match="precision"):
        RotatePlan(theta, 32, 32, True, d, interp="bilinear", precision="faster")
    x32 = torch.zeros((32, 32, 2), device=d)
    with pytest.raises(ValueError, match="bilinear"):
        cp.project_tf_fast(x32, theta, pad=True, precision="fast")                     # interp defaults to nearest there
    with pytest.raises(ValueError, match="bilinear"):
        cp.project_tf_low_mem(x32, theta, pad=True, interp="nearest", precision="fast")
    with pytest.raises(ValueError, match="precision"):
        cp.project_tf_low_mem(x32, theta, pad=True, precision="approximate")
    with pytest.raises(ValueError, match="float64"):
        cp.project_tf_low_mem(x32.double(), theta, pad=True, precision="fast")
    with pytest.raises(ValueError, match="float64"):
        RotatePlan(theta, 32, 32, True, d, interp="bilinear", precision="fast").forward_f64(torch.zeros((2, 32, 32), device=d, dtype=torch.float64))
    # model="siddon" ignores the keyword like it ignores interp
    out = cp.project_tf_fast(x32, theta, pad=True, model="siddon", precision="fast")
    assert out.shape[0] == 6


def test_fast_has_no_form_for_thousands_of_angles():
    """The bilinear LDS kernel keeps its angles' tables in LDS; a call it does not take is refused by a fast plan, not handed to an
    exact kernel."""
    d = dev()
    theta = np.random.default_rng(9).uniform(0, np.pi, 4300)
    plan = fast_plan(theta, 40, 40, True, d)
    with pytest.raises(ValueError, match="no fast form"):
        plan.forward(torch.zeros((1, 40, 40), device=d))
