"""The default noise model on a real MI355X: the Gaussian-approximated Poisson log-probability, d lp / d proj and d lp / d pnm of
every kernel that evaluates csrc/loglik_math.h, held per sample to the float64 reference of tests/np_twin_gauss.py.

Rule: for EVERY sample |got - ref| <= MARGIN * R * bar -- bar the first-order float32 error bar of that sample, R >= 1 the float32
numpy twin's own worst excess on the same operands (against the reference, never against the device; <= 16 by the CPU test), MARGIN
= 4.  No sample is left out; where the bar is 0 (mask == 0; an upstream gradient of 0) the gradient is exactly 0; samples whose
reference is not finite agree in kind.  Every test prints its worst excess before it asserts (run with -s).

    a  the elementwise kernels (gaussian_poisson_log_prob and its backward), 4 kinds x 4 pnm x 3 eps x 3 shapes, and 540 060
       elements -- past 2048 x 256, the second trip of the grid-stride loop -- for one kind per pnm; d / d pnm against the float64
       sum, with the worst case of any float32 summation order of the kernel's shape added to its bar
    b  non-finite and edge samples in one launch
    c  the lp / dlp planes the projector launches store (u16 plan, compact plan, tile plan, direct tiled kernel; dense and angle
       subsets; the ray-driven projector at SIDDON_NS 1, 2, 4, 8), against the reference on the ray-sums the same launch returned,
       and bit for bit against the elementwise kernels on those ray-sums.  The fused epilogue exists for the nearest planned and
       tiled forwards only: bilinear plans and plan-less small geometries refuse forward_loglik (asserted) and take the elementwise
       kernels of (a).

Seen on the MI355X: no sample of any case outside the rule, no defect.  Worst |err| / bar (allowed: 4 R, R <= 6.4 here) --
elementwise lp 3.65, dlp 6.64 (at most 0.53 and 0.43 of the allowance), d / d pnm at most 0.035 of its per-sample term; edge launch
lp 2.18, dlp 1.27, NaN / +inf samples equal in kind; u16 and compact plans lp 1.66, dlp 2.59; tile plan and direct tiled lp 2.03,
dlp 2.35; ray-driven lp 2.11, dlp 2.77.  torch.equal held for every fused kernel: no kernel differs from the elementwise bits.
"""
import math

import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib
from ct_pvae_amd import helper_functions as hf
from ct_pvae_amd.forward_functions import RotatePlan
from tests import np_twin_gauss as tw

pytestmark = pytest.mark.gpu

PNMS = (1e2, 1e3, 1e4, 1e6)
EPSS = (tw.FLT_EPSILON, 1e-7, 1e-3)
SHAPES = ((1, 1, 1), (2, 3, 65), (5, 12, 184))
BIG = (3, 20, 9001)                     # 540 060 elements > 2048 x 256
BIG_CASES = ((1e2, "near", tw.FLT_EPSILON), (1e3, "far", 1e-7), (1e4, "zero", 1e-3), (1e6, "tiny", tw.FLT_EPSILON))   # one kind per pnm


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def held(what, got, a, tag, up=None):
    """The rule for one output plane.  what: logp / dlogp / dpnm; a = (proj, mask, x, pnm, eps) on the host; up: an upstream
    gradient that multiplies the reference and the bar.  Returns the worst excess (in units of the bar)."""
    want, bar = getattr(tw, "reference_" + what)(*a), getattr(tw, "bar_" + what)(*a)
    R = tw.twin_ratio(getattr(tw, "twin_" + what)(*a), want, bar)
    if up is not None:
        with np.errstate(invalid="ignore"):
            want, bar = want * up.astype(np.float64), bar * np.abs(up.astype(np.float64))
    worst, same = tw.worst_excess(got, want, bar)
    print(f"[gauss] {tag} {what}: n {want.size} non-finite {int((~np.isfinite(want)).sum())} R {R:.2f} worst |err| / bar {worst:.2f} "
          f"(allowed {tw.MARGIN * R:.2f})")
    assert same, f"{tag} {what}: non-finite samples differ in kind from the reference"
    assert worst <= tw.MARGIN * R, f"{tag} {what}: a sample misses MARGIN R bar: {worst:.2f} > {tw.MARGIN * R:.2f}"
    return worst


def upstream(shape, seed):
    rng = np.random.default_rng(seed)
    up = rng.standard_normal(shape).astype(np.float32)
    up[rng.random(shape) < 0.1] = 0.0
    return up


def run_elementwise(kind, pnm, eps, shape, seed):
    d = dev()
    proj, mask, x = tw.operands(kind, shape, pnm, seed)
    a = (proj, mask, x, pnm, eps)
    tag = f"elementwise {kind} pnm {pnm:g} eps {eps:g} {shape}"
    up = upstream(shape, seed + 1)
    pt = torch.from_numpy(proj).to(d).requires_grad_(True)
    nt = torch.tensor(pnm, dtype=torch.float32, device=d, requires_grad=True)
    lp = cp.gaussian_poisson_log_prob(pt, torch.from_numpy(mask).to(d), torch.from_numpy(x).to(d), nt, eps)
    (lp * torch.from_numpy(up).to(d)).sum().backward()
    torch.cuda.synchronize()
    held("logp", to_np(lp), a, tag)
    g = to_np(pt.grad)
    held("dlogp", g, a, tag, up=up)
    zero = np.broadcast_to(mask[..., None] == 0, shape) | (up == 0)
    assert (g[zero] == 0).all(), f"{tag}: a gradient at mask == 0 or at a zero upstream is not exactly 0"
    # d / d pnm: the float64 sum, and every order in which the kernel may have added it in float32 (serial per thread, a 6-step
    # shuffle, 4 waves, `grid` atomics)
    want, bar = tw.reference_dpnm(*a), tw.bar_dpnm(*a)
    R = tw.twin_ratio(tw.twin_dpnm(*a), want, bar)
    n = proj.size
    grid = min(math.ceil(n / 256), 2048)
    up64 = up.astype(np.float64)
    first = tw.MARGIN * R * float((np.abs(up64) * bar).sum())
    second = tw.U * (math.ceil(n / (grid * 256)) + 6 + 4 + grid) * float(np.abs(up64 * want).sum())
    err = abs(float(nt.grad.item()) - float((up64 * want).sum()))
    print(f"[gauss] {tag} d/dpnm: {nt.grad.item():.9e} against {(up64 * want).sum():.9e}: |err| {err:.3e}, allowed {first:.3e} (samples) "
          f"+ {second:.3e} (summation), R {R:.2f}")
    assert err <= first + second


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("pnm", PNMS)
@pytest.mark.parametrize("kind", tw.KINDS)
def test_elementwise_kernels(kind, pnm, eps, shape):
    run_elementwise(kind, pnm, eps, shape, seed=11)


@pytest.mark.parametrize("pnm,kind,eps", BIG_CASES)
def test_elementwise_kernels_past_one_grid(pnm, kind, eps):
    """540 060 elements: the grid-stride loop's second trip, and k / P past it (the arithmetic regimes are the small shapes' job: one
    kind and one eps per pnm here)."""
    assert BIG[0] * BIG[1] * BIG[2] > 2048 * 256
    run_elementwise(kind, pnm, eps, BIG, seed=13)


def test_edge_samples_in_one_launch():
    """A negative radicand (NaN in lp and dlp, as the reference), a radicand of exactly 0 (root = 0: lp finite, dlp infinite, the same
    infinity), a small negative ray-sum that keeps the radicand positive, proj = x = 0 on unmasked rays (dlp = -0.5 m / (scale root
    pnm), in the thousands), x = 0 and a far x at a large loc -- each under the masks 1, 0.5, 1 / 180 and 0.  Nothing traps."""
    d = dev()
    pnm, eps = 1024.0, tw.FLT_EPSILON
    e = np.float32(eps)
    pairs = [(-1.0, 0.0), (-1.0, 0.7), (-e * np.float32(pnm), 0.0), (-e * np.float32(pnm), 0.3), (-1e-6, 0.0), (0.0, 0.0), (0.0, 1e-3),
             (1e4, 0.0), (1e4, 1e4), (6e4, 3.0), (1e-8, 0.0), (3.0, 3.0)]
    proj = np.tile(np.float32([p for p, _ in pairs]), (1, 4, 1))
    x = np.tile(np.float32([v for _, v in pairs]), (1, 4, 1))
    mask = np.float32([[1.0, 0.5, 1.0 / 180.0, 0.0]])
    a = (proj, mask, x, pnm, eps)
    want = tw.reference_dlogp(*a)
    assert np.isnan(want[0, 0, :2]).all() and np.isinf(want[0, 0, 2:4]).all() and np.isfinite(want[0, 0, 4:]).all()
    assert np.isfinite(want[0, 3]).all() and (want[0, 3] == 0).all()                 # a masked-out row: loc = 0 whatever proj is
    s = np.float64(e) + np.sqrt(np.float64(e))
    assert abs(want[0, 0, 5] - (-0.5 / (s * np.sqrt(np.float64(e)) * pnm))) <= 1e-12 * abs(want[0, 0, 5])
    pt = torch.from_numpy(proj).to(d).requires_grad_(True)
    nt = torch.tensor(pnm, dtype=torch.float32, device=d, requires_grad=True)
    lp = cp.gaussian_poisson_log_prob(pt, torch.from_numpy(mask).to(d), torch.from_numpy(x).to(d), nt, eps)
    lp.sum().backward()
    torch.cuda.synchronize()                                                         # (a trap would surface here)
    held("logp", to_np(lp), a, "edge")
    g = to_np(pt.grad)
    held("dlogp", g, a, "edge")
    assert (g[0, 3] == 0).all()
    # the same samples one by one: d / d pnm of each (the sum over all of them is NaN)
    for j in range(4, len(pairs)):
        b = (proj[:, :, j:j + 1], mask, x[:, :, j:j + 1], pnm, eps)
        n1 = torch.tensor(pnm, dtype=torch.float32, device=d, requires_grad=True)
        p1 = torch.from_numpy(np.ascontiguousarray(b[0])).to(d)
        cp.gaussian_poisson_log_prob(p1, torch.from_numpy(mask).to(d), torch.from_numpy(np.ascontiguousarray(b[2])).to(d), n1, eps).sum().backward()
        ref, bar = tw.reference_dpnm(*b), tw.bar_dpnm(*b)
        R = tw.twin_ratio(tw.twin_dpnm(*b), ref, bar)
        allowed = tw.MARGIN * R * float(bar.sum()) + tw.U * (1 + 6 + 4 + 1) * float(np.abs(ref).sum())
        assert abs(float(n1.grad.item()) - float(ref.sum())) <= allowed, (pairs[j], n1.grad.item(), ref.sum())


# ---- c: the planes the projector launches store -------------------------------------------------------------------------------
def masks_and_measurements(sino, pnm, seed):
    """mask [B][A] from the twin's values with whole rows of zeros; measurements next to loc on even angles (Poisson(loc pnm) / pnm),
    far from it on odd ones (uniform in [0, 3))."""
    rng = np.random.default_rng(seed)
    B, A, P = sino.shape
    mask = rng.choice(np.float32(tw.MASKS[1:]), size=(B, A)).astype(np.float32)
    mask[:, ::3] = 0.0
    mask[0, :] = np.roll(mask[0, :], 1)
    loc = sino.astype(np.float64) * mask[..., None]
    meas = (rng.poisson(loc * pnm) / pnm).astype(np.float32)
    meas[:, 1::2] = (rng.random((B, A, P)) * 3.0).astype(np.float32)[:, 1::2]
    return mask, meas


def check_planes(tag, sino, lp, dlp, mask, meas, pnm, eps):
    """lp, dlp of a projector launch against the reference on the launch's own ray-sums, and against the elementwise kernels."""
    d = dev()
    assert torch.isfinite(sino).all()
    a = (to_np(sino), mask, meas, pnm, eps)
    held("logp", to_np(lp), a, tag)
    held("dlogp", to_np(dlp), a, tag)
    zero = np.broadcast_to(mask[..., None] == 0, a[0].shape)
    assert zero.any() and (to_np(dlp)[zero] == 0).all(), f"{tag}: dlp at mask == 0 is not exactly 0"
    p = sino.detach().clone().requires_grad_(True)
    two = cp.gaussian_poisson_log_prob(p, torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), pnm, eps)
    two.backward(torch.ones_like(two))
    assert torch.equal(lp, two.detach()), f"{tag}: lp differs from the elementwise kernel's bits"
    assert torch.equal(dlp, p.grad), f"{tag}: dlp differs from the elementwise backward's bits"


ROTATE_CASES = [(fmt, shape, A, B) for fmt in ("u16", "compact") for shape, A, B in (((16, 16), 5, 3), ((33, 47), 7, 4))] + \
               [(fmt, (190, 211), 3, 2) for fmt in ("tile_plan", "tile_direct")]


@pytest.mark.parametrize("pnm", [1e3, 1e4])
@pytest.mark.parametrize("angles", ["dense", "subset"])
@pytest.mark.parametrize("fmt,shape,A,B", ROTATE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_planes_of_the_rotate_launches(fmt, shape, A, B, angles, pnm):
    d = dev()
    H, W = shape
    eps = tw.FLT_EPSILON
    rng = np.random.default_rng(H + A)
    theta = np.sort(rng.uniform(0.0, np.pi, A)).astype(np.float32)
    theta[0] = 0.0
    plan = RotatePlan(theta, H, W, True, d, plan_format={"tile_plan": "auto", "tile_direct": "u16"}.get(fmt, fmt))
    if fmt.startswith("tile"):
        assert plan.tiled and (plan._tplan is not None) == (fmt == "tile_plan")
    else:
        assert plan.planned[0] and not plan.tiled and plan.compact == (fmt == "compact")
    x = torch.from_numpy(rng.random((B, H, W), dtype=np.float32)).to(d)
    mask, meas = masks_and_measurements(to_np(plan.forward(x)), pnm, seed=A)
    pt = torch.tensor(pnm, dtype=torch.float32, device=d)
    mt, yt = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    if angles == "dense":
        sino, lp, dlp = plan.forward_loglik(x, mt, yt, pt, eps, with_dlp=True)
        sub = np.arange(A)
    else:
        sub = np.array([A - 1, 0, 2, 2, 1][:A + 1], np.int32)       # any order, a repeat, a masked-out row (0)
        sino, lp, dlp = plan.forward_loglik(x, mt, yt, pt, eps, with_dlp=True, angles_i=torch.from_numpy(sub).to(d), dense_inputs=True)
    assert tuple(lp.shape) == tuple(dlp.shape) == (B, len(sub), plan.PW)
    assert torch.equal(sino, plan.forward(x)[:, torch.from_numpy(sub).to(d).long()])
    check_planes(f"rotate {fmt} {H}x{W} {angles} pnm {pnm:g}", sino, lp, dlp, np.ascontiguousarray(mask[:, sub]),
                 np.ascontiguousarray(meas[:, sub]), pnm, eps)


def test_no_fused_store_without_a_nearest_plan():
    """Bilinear plans and plan-less geometries that fit LDS have no likelihood epilogue: forward_loglik refuses them, and the training
    call evaluates the elementwise kernels on their ray-sums."""
    d = dev()
    theta = np.linspace(0.0, np.pi, 5, endpoint=False).astype(np.float32)
    x = torch.zeros((3, 16, 16), device=d)
    m, y, p = torch.zeros((3, 5), device=d), torch.zeros((3, 5, 26), device=d), torch.tensor(1e3, device=d)
    for kw in (dict(interp="bilinear"), dict(use_plan=False)):
        with pytest.raises(ValueError, match="planned or tiled forward"):
            RotatePlan(theta, 16, 16, True, d, **kw).forward_loglik(x, m, y, p, tw.FLT_EPSILON, with_dlp=True)


@pytest.mark.parametrize("ns", [1, 2, 4, 8])
@pytest.mark.parametrize("pad", [True, False])
def test_planes_of_the_siddon_launch(pad, ns):
    d = dev()
    B, shape, A = 4, (33, 47), 7
    rng = np.random.default_rng(7)
    img = rng.random((B,) + shape, dtype=np.float32)
    theta = np.ascontiguousarray(rng.uniform(0.0, np.pi, A), dtype=np.float32)
    theta[:2] = [0.0, np.pi / 2]                                    # rays along the grid lines
    x = torch.from_numpy(img).to(d)
    st = hf._siddon_loglik_state(theta, B, shape[0], shape[1], pad, d)
    dense = to_np(cp.project_tf_fast(x[..., None], theta, pad=pad, dim=2, integrate_vae=True, model="siddon"))[..., 0]
    for pnm in (1e3, 1e4):
        mask, meas = masks_and_measurements(dense, pnm, seed=ns)
        pt = torch.tensor(pnm, dtype=torch.float32, device=d)
        mt, yt = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
        for sub in (None, [6, 0, 0, 3, 1]):
            with _lib.tuned("SIDDON_NS", ns):
                sino, lp, dlp = hf._siddon_loglik_forward(st, x, mt, yt, pt, tw.FLT_EPSILON, None if sub is None else st.sel(sub),
                                                          want_sino=True, want_dlp=True)
            rows = np.arange(A) if sub is None else np.asarray(sub)
            np.testing.assert_array_equal(to_np(sino), dense[:, rows])
            check_planes(f"siddon {shape} pad {pad} NS {ns} {'dense' if sub is None else 'subset'} pnm {pnm:g}", sino, lp, dlp,
                         np.ascontiguousarray(mask[:, rows]), np.ascontiguousarray(meas[:, rows]), pnm, tw.FLT_EPSILON)
