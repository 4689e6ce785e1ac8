"""The gradient of a float64 projection, computed in float64 on the MI355X (ctpvae_rotate_bwd_f64, RotatePlan.backward_f64):
TensorFlow's gradient for T = double ("tf_compat") and the transpose of the float64 forward ("exact"), both equal in every bit to
the numpy twin (tests/np_twin64.py), through every layout of project_tf_fast / project_tf_low_mem."""
import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan
from tests import np_twin64 as twin

pytestmark = pytest.mark.gpu
INTERP = {"nearest": 0, "bilinear": 1}
PAIRS = [(i, b) for i in ("nearest", "bilinear") for b in ("tf_compat", "exact")]
FUZZ_GEOMS = [(1, 1, True), (1, 1, False), (2, 2, False), (17, 13, True), (17, 13, False), (33, 64, True), (33, 64, False),
              (130, 129, True), (130, 129, False)]


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def plan_for(oracle, theta, H, W, pad, interp, backward):
    """A plan on the oracle's tables (the twin's), and the oracle geometry of the same canvas."""
    geom = oracle.Geometry(H, W, pad)
    T, Tinv = twin.tables(theta, geom)
    d = dev()
    plan = RotatePlan(None, H, W, pad, d, interp=interp, backward=backward,
                      _tables=(torch.from_numpy(T).to(d), torch.from_numpy(Tinv).to(d)))
    return plan, geom, T, Tinv


def want(geom, T, Tinv, g, interp, backward):
    if backward == "tf_compat":
        return twin.bwd_tfcompat(g, geom, Tinv, INTERP[interp])
    return twin.bwd_exact(g, geom, T, INTERP[interp])


def cotangent(rng, shape):
    g = rng.standard_normal(shape)
    assert (g != g.astype(np.float32)).all()        # not representable in fp32: a cast would lose digits
    return g


def adjoint_gap(plan, x, g):
    """|<A x, g> - <x, A^T g>| over the sum of |terms|, A = forward_f64, A^T = backward_f64 (an exact plan)."""
    ax = to_np(plan.forward_f64(torch.from_numpy(x).to(dev())))
    atg = to_np(plan.backward_f64(torch.from_numpy(g).to(dev())))
    lhs, rhs = float((ax * g).sum()), float((x * atg).sum())
    return abs(lhs - rhs) / float(np.abs(ax * g).sum())


@pytest.mark.parametrize("backward", ["tf_compat", "exact"])
@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_backward_f64_equals_the_twin_on_fuzz_geometries(oracle, interp, backward):
    rng = np.random.default_rng(600 + 2 * INTERP[interp] + (backward == "exact"))
    for H, W, pad in FUZZ_GEOMS:
        for A in (1, 7, 20, 180):
            S = 1 + (H + A) % 3
            plan, geom, T, Tinv = plan_for(oracle, twin.angle_set(A, rng), H, W, pad, interp, backward)
            g = cotangent(rng, (S, A, geom.PW))
            got = plan.backward_f64(torch.from_numpy(g).to(dev()))
            assert got.dtype == torch.float64 and tuple(got.shape) == (S, H, W)
            np.testing.assert_array_equal(to_np(got), want(geom, T, Tinv, g, interp, backward),
                                          err_msg=f"{interp}/{backward} {H}x{W} pad={pad} A={A} S={S}")


@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
def test_full_size_128(oracle, interp):
    """50 x 128^2 x 20 angles: tf_compat equals the twin; exact is the transpose of forward_f64 to <= 1e-13."""
    rng = np.random.default_rng(128 + INTERP[interp])
    theta = twin.angle_set(20, rng)
    g = cotangent(rng, (50, 20, 184))
    plan, geom, T, Tinv = plan_for(oracle, theta, 128, 128, True, interp, "tf_compat")
    np.testing.assert_array_equal(to_np(plan.backward_f64(torch.from_numpy(g).to(dev()))),
                                  twin.bwd_tfcompat(g, geom, Tinv, INTERP[interp]))
    ex, _, _, _ = plan_for(oracle, theta, 128, 128, True, interp, "exact")
    gap = adjoint_gap(ex, rng.random((50, 128, 128)), g)
    assert gap <= 1e-13, gap


def test_full_size_512_bilinear(oracle):
    """512^2 bilinear (a slice that does not fit LDS in double): both modes equal the twin on 1 slice x 10 angles; exact is
    the transpose of forward_f64 to <= 1e-13 on the 4 x 512^2 x 90 launch."""
    rng = np.random.default_rng(512)
    theta = twin.angle_set(10, rng)
    for backward in ("tf_compat", "exact"):
        plan, geom, T, Tinv = plan_for(oracle, theta, 512, 512, True, "bilinear", backward)
        g = cotangent(rng, (1, 10, geom.PW))
        np.testing.assert_array_equal(to_np(plan.backward_f64(torch.from_numpy(g).to(dev()))),
                                      want(geom, T, Tinv, g, "bilinear", backward), err_msg=backward)
    ex, geom, _, _ = plan_for(oracle, twin.angle_set(90, rng), 512, 512, True, "bilinear", "exact")
    gap = adjoint_gap(ex, rng.random((4, 512, 512)), cotangent(rng, (4, 90, geom.PW)))
    assert gap <= 1e-13, gap


@pytest.mark.parametrize("backward", ["tf_compat", "exact"])
def test_bits_fixed_run_to_run_and_across_slice_chunks(oracle, backward):
    rng = np.random.default_rng(7)
    for interp in ("nearest", "bilinear"):
        plan, geom, _, _ = plan_for(oracle, twin.angle_set(20, rng), 33, 64, True, interp, backward)
        g = torch.from_numpy(cotangent(rng, (12, 20, geom.PW))).to(dev())
        a = plan.backward_f64(g)
        assert torch.equal(a, plan.backward_f64(g))
        with _lib.tuned("MAX_SLICES", 5):                 # three launches of 5, 5 and 2 slices
            assert torch.equal(a, plan.backward_f64(g))


def layouts(rng, H, W, Z):
    """(name, call(x, theta, pad, interp, backward), x, slices of x [S][H][W], cotangent slices [S][A][PW] of a gout)."""
    return [
        ("integrate_vae", lambda x, th, pad, i, b: cp.project_tf_fast(x, th, pad=pad, integrate_vae=True, interp=i, backward=b),
         rng.random((Z, H, W, 1)), lambda v: v[..., 0], lambda go: go[..., 0], lambda s: s[..., None]),
        ("dim=3", lambda x, th, pad, i, b: cp.project_tf_fast(x, th, pad=pad, dim=3, interp=i, backward=b),
         rng.random((H, W, Z)), lambda v: v.transpose(2, 0, 1), lambda go: go.transpose(2, 0, 1), lambda s: s.transpose(1, 2, 0)),
        ("dim=2", lambda x, th, pad, i, b: cp.project_tf_fast(x, th, pad=pad, dim=2, interp=i, backward=b),
         rng.random((H, W)), lambda v: v[None], lambda go: go.transpose(2, 0, 1), lambda s: s[0]),
        ("low_mem", lambda x, th, pad, i, b: cp.project_tf_low_mem(x, th, pad=pad, interp=i, backward=b),
         rng.random((H, W, Z)), lambda v: v.transpose(2, 0, 1), lambda go: go.transpose(2, 0, 1), lambda s: s.transpose(1, 2, 0)),
    ]


@pytest.mark.parametrize("interp,backward", PAIRS)
def test_float64_calls_get_the_float64_gradient(oracle, interp, backward):
    """project_tf_fast / project_tf_low_mem on float64 x: x.grad is float64 and equal in every bit to the twin (before, the
    cotangent went through the fp32 backward and came back ~1e-7 off)."""
    d = dev()
    rng = np.random.default_rng(64 + 2 * INTERP[interp] + (backward == "exact"))
    H, W, Z, A, pad = 33, 40, 3, 20, True
    theta = twin.angle_set(A, rng)
    geom = oracle.Geometry(H, W, pad)
    T, Tinv = twin.tables(theta, geom)
    for name, call, x0, _, gslices, unslice in layouts(rng, H, W, Z):
        x = torch.from_numpy(x0).to(d).requires_grad_(True)
        out = call(x, theta, pad, interp, backward)
        assert out.dtype == torch.float64, name
        gout = cotangent(rng, tuple(out.shape))
        out.backward(torch.from_numpy(gout).to(d))
        assert x.grad.dtype == torch.float64, name
        np.testing.assert_array_equal(to_np(x.grad), unslice(want(geom, T, Tinv, np.ascontiguousarray(gslices(gout)), interp, backward)),
                                      err_msg=f"{name} {interp}/{backward}")
    # the slices layout: RotatePlan.apply
    plan, geom, T, Tinv = plan_for(oracle, theta, H, W, pad, interp, backward)
    x = torch.from_numpy(rng.random((2, H, W))).to(d).requires_grad_(True)
    out = plan.apply(x)
    g = cotangent(rng, tuple(out.shape))
    out.backward(torch.from_numpy(g).to(d))
    np.testing.assert_array_equal(to_np(x.grad), want(geom, T, Tinv, g, interp, backward), err_msg="slices")


@pytest.mark.parametrize("interp,backward", PAIRS)
def test_gradcheck(interp, backward):
    """torch.autograd.gradcheck on a 9 x 7 padded slice.  tf_compat is TensorFlow's gradient, which is the transpose of the
    forward only where resampling with the inverted rows hits the forward's own taps: quarter turns (there it agrees with the
    exact transpose to ~1e-6, inside gradcheck's tolerance); exact is the transpose at any angle."""
    theta = np.arange(4) * (np.pi / 2) if backward == "tf_compat" else np.array([0.0, np.pi / 4, 1.1, 2.5, 4.0])
    x = torch.from_numpy(np.random.default_rng(9).random((9, 7))).to(dev()).requires_grad_(True)
    fn = lambda v: cp.project_tf_fast(v, theta, pad=True, dim=2, interp=interp, backward=backward)   # noqa: E731
    assert torch.autograd.gradcheck(fn, (x,))


@pytest.mark.parametrize("interp,backward", PAIRS)
def test_float32_gradient_unchanged(interp, backward):
    """float32 calls keep their paths: x.grad is torch.equal to plan.backward of the same cotangent."""
    d = dev()
    rng = np.random.default_rng(32)
    H, W, Z, A, pad = 33, 40, 3, 20, True
    theta = twin.angle_set(A, rng).astype(np.float32)
    plan = RotatePlan(theta, H, W, pad, d, interp=interp, backward=backward)
    for name, call, x0, _, gslices, unslice in layouts(rng, H, W, Z):
        x = torch.from_numpy(x0.astype(np.float32)).to(d).requires_grad_(True)
        out = call(x, theta, pad, interp, backward)
        gout = torch.from_numpy(rng.standard_normal(tuple(out.shape)).astype(np.float32)).to(d)
        out.backward(gout)
        assert x.grad.dtype == torch.float32, name
        ref = plan.backward(torch.from_numpy(np.ascontiguousarray(gslices(to_np(gout)))).to(d))
        assert torch.equal(x.grad, torch.from_numpy(np.ascontiguousarray(unslice(to_np(ref)))).to(d)), name


def test_backward_f64_refuses_angle_subsets_and_bad_operands():
    d = dev()
    plan = RotatePlan(np.linspace(0, np.pi, 8, endpoint=False), 16, 16, True, d)
    g = torch.zeros((2, 8, plan.PW), dtype=torch.float64, device=d)
    with pytest.raises(ValueError):
        plan.backward_f64(g, angles_i=torch.arange(4, dtype=torch.int32, device=d))
    with pytest.raises(ValueError):
        plan.backward_f64(g.float())
    with pytest.raises(ValueError):
        plan.backward_f64(g[:, :4])
    assert plan.backward_f64(g[:0]).shape == (0, 16, 16)
