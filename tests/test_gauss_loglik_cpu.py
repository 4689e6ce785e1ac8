"""The Gaussian-approximated Poisson log-probability (the default noise model) without a GPU: the float32 twin of csrc/loglik_math.h
against the float64 reference under the per-sample bars of tests/np_twin_gauss.py, the reference's derivatives against float64
autograd, the golden log-probabilities under the rule, and a negative control: two wrong derivatives the rule must refuse.

Seen here (300 000 samples per regime, 4 kinds x pnm in {1e2, 1e3, 1e4, 1e6} x eps in {FLT_EPSILON, 1e-3}): the twin's worst excess
is 2.97 for lp, 6.59 for dlp and 8.74 for dpnm, against R_MAX = 16.  The two wrong derivatives miss the bar by factors of 2e5 .. 1.7e7;
the max-normalised error that the older tests bound by 1e-4 is 1.8e-5 for the derivative without its dscale term on "near" at
pnm = 1e6, eps = 1e-3 and 5.9e-5 for the one with 1 / scale applied once on "far" at pnm = 1e2: that bar passes both there."""
import os

import numpy as np
import pytest
import torch

from tests import np_twin_gauss as tw
from tests.conftest import ROOT

PNMS = (1e2, 1e3, 1e4, 1e6)
EPSS = (tw.FLT_EPSILON, 1e-3)
SHAPE = (5, 40, 1500)                   # 300 000 samples per regime
WHAT = ("logp", "dlogp", "dpnm")


def evaluate(what, fn, a):
    want, bar = getattr(tw, "reference_" + what)(*a), getattr(tw, "bar_" + what)(*a)
    return tw.worst_excess(fn(*a), want, bar)


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("pnm", PNMS)
def test_twin_within_the_bars_of_the_reference(pnm, eps):
    for kind in tw.KINDS:
        a = tw.operands(kind, SHAPE, pnm, seed=1) + (pnm, eps)
        assert (a[1] == 0).any() and (a[1] == 1).any()                      # masked-out rows are in
        r = {}
        for what in WHAT:
            r[what], same = evaluate(what, getattr(tw, "twin_" + what), a)
            assert same, f"{kind} {what}: non-finite samples"
        print(f"[gauss] twin vs float64, {kind} pnm {pnm:g} eps {eps:g}: worst excess lp {r['logp']:.2f} dlp {r['dlogp']:.2f} "
              f"dpnm {r['dpnm']:.2f}")
        for what in WHAT:
            assert r[what] <= tw.R_MAX, f"{kind} {what}: the twin misses its own bar by {r[what]:.2f} > R_MAX"
        # the exact zeros of the rule
        dlp, dpnm = tw.twin_dlogp(*a), tw.twin_dpnm(*a)
        m = np.broadcast_to(a[1][..., None], a[0].shape)
        assert (dlp[m == 0] == 0).all() and (dpnm[(a[0] * m) == 0] == 0).all()


def test_operands_are_what_they_say():
    for kind in tw.KINDS:
        proj, mask, x = tw.operands(kind, (2, 30, 65), 1e4, seed=3)
        assert proj.dtype == mask.dtype == x.dtype == np.float32 and proj.shape == x.shape == (2, 30, 65) and mask.shape == (2, 30)
        assert set(np.unique(mask)) <= set(np.float32(tw.MASKS)) and (proj >= 0).all() and (x >= 0).all()
        if kind == "zero":
            assert (proj.reshape(-1)[::2] == 0).all() and (proj.reshape(-1)[1::2] > 0).any()
        if kind == "tiny":
            assert proj.max() <= 1.0 and proj.min() >= 1e-8 * 0.999
        if kind == "far":
            assert x.max() < 3.0
    with pytest.raises(ValueError):
        tw.operands("other", (1, 1, 1), 1e4, 0)


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("pnm", PNMS)
def test_reference_derivatives_are_float64_autograd(pnm, eps):
    """d / d proj and d / d pnm (per sample: pnm is expanded) of torch.distributions.Normal(loc, scale).log_prob(x) in float64,
    on the samples with mask > 0, to 1e-12 relative per sample.

    Both sides are float64 evaluations of z^2 - 1 (and of t1 + t2): each carries about 6.5 2^-53 z^2 of rounding into that
    difference, so two CORRECT evaluations differ by up to 1.4e-15 / |z^2 - 1| relative, which is 1e-12 once a sample has
    |z^2 - 1| < 1.4e-3 -- one sample in 1 400 where z is standard normal ("near").  The formula is what this test checks, not the
    conditioning of float64, so it takes 160 samples per kind (640 per regime: every mask value, every kind, |z| from 0 to 1e4)
    and holds each to the plain 1e-12.  Seen: 12 000 samples per kind differ by up to 2.5e-12, at |z^2 - 1| ~ 1e-4."""
    worst = 0.0
    for kind in tw.KINDS:
        proj, mask, x = tw.operands(kind, (4, 5, 8), pnm, seed=2)
        assert len(np.unique(mask)) == len(tw.MASKS)
        p64 = torch.from_numpy(proj.astype(np.float64)).requires_grad_(True)
        n64 = torch.full(proj.shape, float(np.float32(pnm)), dtype=torch.float64, requires_grad=True)
        e64 = float(np.float32(eps))
        loc = p64 * torch.from_numpy(mask.astype(np.float64))[..., None]
        scale = e64 + torch.sqrt(loc / n64 + e64)
        torch.distributions.Normal(loc, scale).log_prob(torch.from_numpy(x.astype(np.float64))).sum().backward()
        on = np.broadcast_to(mask[..., None] > 0, proj.shape)
        for got, want in ((tw.reference_dlogp(proj, mask, x, pnm, eps), p64.grad.numpy()),
                          (tw.reference_dpnm(proj, mask, x, pnm, eps), n64.grad.numpy())):
            assert np.isfinite(want[on]).all()
            rel = np.abs(got[on] - want[on]) / np.maximum(np.abs(want[on]), 1e-300)
            rel = np.where(got[on] == want[on], 0.0, rel)
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-12, f"{kind}: {rel.max():.3e}"
    print(f"[gauss] reference derivatives vs float64 autograd, pnm {pnm:g} eps {eps:g}: worst relative difference {worst:.3e}")


def test_reference_edge_values():
    one = np.ones((1, 1), np.float32)
    eps = tw.FLT_EPSILON
    # proj = x = 0 on an unmasked ray: z = 0, d lp / d proj = -0.5 m / (scale root pnm)
    for m in (1.0, 0.5, 1.0 / 180.0):
        got = tw.reference_dlogp(np.zeros((1, 1, 1), np.float32), m * one, np.zeros((1, 1, 1), np.float32), 1e4, eps)[0, 0, 0]
        e = np.float64(np.float32(eps))
        want = -0.5 * np.float64(np.float32(m)) / ((e + np.sqrt(e)) * np.sqrt(e) * 1e4)
        assert abs(got - want) <= 1e-14 * abs(want)
        assert tw.twin_dpnm(np.zeros((1, 1, 1), np.float32), m * one, np.zeros((1, 1, 1), np.float32), 1e4, eps)[0, 0, 0] == 0
    # a negative radicand: NaN everywhere, in both
    a = (np.full((1, 1, 1), -1.0, np.float32), one, np.zeros((1, 1, 1), np.float32), 1e2, eps)
    for what in WHAT:
        assert np.isnan(getattr(tw, "reference_" + what)(*a)).all() and np.isnan(getattr(tw, "twin_" + what)(*a)).all()
    # worst_excess: exact zeros where the bar is 0, kinds of the non-finite samples
    want, bar = np.array([0.0, 1.0, np.nan, np.inf]), np.array([0.0, 1e-3, np.nan, np.nan])
    assert tw.worst_excess(np.array([0.0, 1.0005, np.nan, np.inf]), want, bar) == (pytest.approx(0.5), True)
    assert tw.worst_excess(np.array([1e-30, 1.0, np.nan, np.inf]), want, bar) == (np.inf, True)
    assert tw.worst_excess(np.array([0.0, 1.0, np.nan, -np.inf]), want, bar)[1] is False
    assert tw.worst_excess(np.array([0.0, 1.0, 0.0, np.inf]), want, bar)[1] is False
    assert tw.worst_excess(np.array([0.0, np.nan, np.nan, np.inf]), want, bar)[0] == np.inf


def test_golden_log_probabilities_within_the_rule():
    z = np.load(os.path.join(ROOT, "tests", "golden", "loglik.npz"))
    a = (z["proj"], z["mask"], z["x"], float(z["pnm"]), float(z["eps"]))
    want, bar = tw.reference_logp(*a), tw.bar_logp(*a)
    R = tw.twin_ratio(tw.twin_logp(*a), want, bar)
    worst, same = tw.worst_excess(z["out"], want, bar)
    print(f"[gauss] golden loglik.npz: n {want.size} R {R:.2f}, worst |out - ref| / bar {worst:.2f} (allowed {tw.MARGIN * R:.2f})")
    assert same and R <= tw.R_MAX and worst <= tw.MARGIN * R


@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("pnm", PNMS)
def test_the_rule_refuses_wrong_derivatives(pnm, eps):
    """Negative control: without the dscale term, and with 1 / scale applied once instead of twice, the twin fails the rule on
    every kind -- while the max-normalised error (printed) is in places below the 1e-4 that used to be the only bar."""
    for kind in tw.KINDS:
        a = tw.operands(kind, SHAPE, pnm, seed=1) + (pnm, eps)
        want, bar = tw.reference_dlogp(*a), tw.bar_dlogp(*a)
        R = tw.twin_ratio(tw.twin_dlogp(*a), want, bar)
        for name, fn in (("no dscale", tw.twin_dlogp_without_dscale), ("rs once", tw.twin_dlogp_rs_once)):
            got = fn(*a)
            worst, _ = tw.worst_excess(got, want, bar)
            maxnorm = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"[gauss] negative control '{name}', {kind} pnm {pnm:g} eps {eps:g}: worst excess {worst:.3g} against "
                  f"MARGIN R = {tw.MARGIN * R:.1f}; max-normalised error {maxnorm:.2e} (old bar 1e-4)")
            assert worst > tw.MARGIN * R, f"the rule accepts '{name}' on {kind}"
