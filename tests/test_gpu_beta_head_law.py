"""The LAW of the fused Beta output head on the device (csrc/beta_head.hip, beta_head.h): the assertions of
tests/test_beta_head_law_cpu.py -- its cells, seeds, draws and closed forms -- on the device's own lg (aux[..., 3]), x and gradients.
Nothing here takes the law from np_twin_beta's search or compose: the PITs are scipy's (tests/np_law.py), the gradient means'
targets closed forms.  The float64 composition at the device's accepted draws enters ONLY as the gradient means' standard error
(6 SE is the bound) and as the per-sample reference the device's mean must stay within 0.5 SE of.

One launch of n = 1, pix = 2^20 per cell (under 64 MB of device memory); the trainer's way of calling -- many small launches over
consecutive draws -- is the last law test.

Measured on an MI355X, as ratios to the bound (the figures the tests print; none of them sets a bound):
    cells                  worst KS / dkw 0.514 (lg_1 of the cell (1e-3, 0.05)), of x 0.474 (the cell (7, 40));
                           worst |corr| / corr_bound 0.358 (lg_0 against lg_1 of the cell (0.5, 0.5)).  Per cell, worst KS / dkw and
                           worst |corr| / corr_bound: (1e-3, 0.05) 0.514 0.232; (0.3, 0.999) 0.369 0.170; seam 0.353 0.099;
                           (0.5, 0.5) 0.371 0.358; (1.5, 2.5) 0.256 0.220; (7, 40) 0.474 0.234; (40, 300) 0.374 0.198
    pooled ranges          KS / dkw of lg_0, lg_1: trainer 0.155 0.253; small 0.261 0.505; large 0.219 0.319; mixed 0.203 0.330
    86 small launches      KS / dkw 0.264 (lg_0), 0.333 (lg_1); |corr| of adjacent draws / corr_bound 0.131, 0.044
    gradient means         |mean - closed form| / SE, g_alpha and g_beta:
                             (1.5, 2.5)  (a) 1.54 1.39   (b) 1.52 0.88   (c) 0.49 0.78
                             (7, 40)     (a) 0.89 0.85   (b) 0.80 0.70   (c) 1.10 1.19
                             (0.8, 0.9)  (a) 2.22 1.29   (b) 1.24 0.16   (c) 0.66 1.48
                           |mean - the float64 reference's mean| / SE: at most 0.0009 (bound 0.5)"""
import numpy as np
import pytest

from tests import np_law as law
from tests import np_twin_beta as tb
from tests import test_beta_head_law_cpu as cpu
from tests.test_gpu_beta_head import run_head

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
N = cpu.N
TRAINER_SHAPE, TRAINER_FIRST_OBJECT, TRAINER_DRAWS, TRAINER_DRAW0, TRAINER_OPERAND_SEED = (3, 41, 100), 7, 86, 32, 104


def device_sample(alpha, beta, draw, first_object=0, X=1):
    """(lg [n][pix][2] float32, x [n][pix] float32, aux) of one launch with the CPU file's seed."""
    d = run_head(alpha, beta, first_object, draw, seed=cpu.SEED, X=X)
    assert np.isfinite(d["aux"][..., 3]).all() and np.isfinite(d["x"]).all()
    return d["aux"][..., 3], d["x"], d["aux"]


@pytest.mark.parametrize("i", cpu.LAW_CELLS, ids=[cpu.CELLS[i][0] for i in cpu.LAW_CELLS])
def test_cell_follows_the_gamma_and_beta_laws(i):
    """KS of the PIT of the device's lg_0, lg_1 (and x from concentration 0.3 on) <= dkw(N); the two gammas' PITs, and each gamma's
    PITs of neighbouring pixels, uncorrelated within corr_bound(N)."""
    alpha, beta = cpu.cell_operands(i)
    c, _ = cpu.concentrations(alpha, beta)
    lg, x, _ = device_sample(alpha, beta, i)
    with_x = float(c.min()) >= cpu.X_LAW_FROM * (1 - 2e-6)
    assert with_x == (i != 0)
    r = cpu.law_stats(c, lg, x if with_x else None)
    for k, v in r.items():
        print(f"cell {cpu.CELLS[i][0]} device {k}: {v:.3f} of its bound")
    ks, co = [v for k, v in r.items() if k.startswith("KS")], [v for k, v in r.items() if k.startswith("corr")]
    print(f"cell {cpu.CELLS[i][0]}: worst KS / dkw {max(ks):.3f}, worst |corr| / corr_bound {max(co):.3f}")
    assert len(ks) == (3 if with_x else 2) and len(co) == 3
    for k, v in r.items():
        assert v <= 1.0, (cpu.CELLS[i][0], k, v)


@pytest.mark.parametrize("kind", list(tb.RANGES))
def test_pooled_range_follows_the_gamma_law(kind):
    """2^20 pixels with operands uniform on the raw range: the pooled PITs of each gamma's logarithm are uniform."""
    seed, draw = cpu.POOLED[kind]
    alpha, beta = tb.operands(kind, 1, N, seed)
    c, _ = cpu.concentrations(alpha, beta)
    lg, _, _ = device_sample(alpha, beta, draw)
    for j in (0, 1):
        ratio = law.ks_uniform(law.pit_log_gamma(c[..., j], lg[..., j])) / law.dkw(N)
        print(f"pooled {kind} device KS lg_{j}: {ratio:.3f} of dkw")
        assert ratio <= 1.0, (kind, j, ratio)


def test_many_small_launches_over_consecutive_draws():
    """The trainer's way of calling the head: (3, 41, 100) with first_object = 7, the "mixed" range, 86 consecutive draws -- 1.06 M
    samples through 86 launches.  The pooled PITs of each gamma are uniform (dkw of the pooled size), and the PITs of one pixel at
    adjacent draws are uncorrelated within corr_bound."""
    n, X, Y = TRAINER_SHAPE
    alpha, beta = tb.operands("mixed", n, X * Y, TRAINER_OPERAND_SEED)
    c, _ = cpu.concentrations(alpha, beta)
    lg = np.stack([device_sample(alpha, beta, TRAINER_DRAW0 + t, TRAINER_FIRST_OBJECT, X=X)[0] for t in range(TRAINER_DRAWS)])
    total = TRAINER_DRAWS * n * X * Y
    assert lg.shape == (TRAINER_DRAWS, n, X * Y, 2) and total >= 2 ** 20
    for j in (0, 1):
        p = law.pit_log_gamma(c[None, ..., j], lg[..., j])
        ks = law.ks_uniform(p) / law.dkw(total)
        co = abs(law.corr(p[:-1], p[1:])) / law.corr_bound(total - n * X * Y)
        print(f"86 launches, lg_{j}: KS / dkw {ks:.3f}, |corr| of adjacent draws / corr_bound {co:.3f}")
        assert ks <= 1.0 and co <= 1.0, (j, ks, co)


@pytest.mark.parametrize("i", cpu.GRAD_CELLS, ids=[cpu.CELLS[i][0] for i in cpu.GRAD_CELLS])
def test_gradient_means_are_the_derivatives_of_the_moments(i):
    """The device's g_alpha and g_beta over 2^20 samples, sr = eps: their means are within 6 SE of (a) the derivatives of E[x], (b) of
    E[x^2], (c) of minus the entropy, each times pr' -- SE from the float64 composition's gradients at the device's accepted draws,
    not from the device's values -- and within 0.5 SE of that reference's own mean (the tie to the per-sample test)."""
    alpha, beta = cpu.cell_operands(i)
    _, _, aux = device_sample(alpha, beta, i)
    ref, dl, grads = cpu.reference_gradients(alpha, beta, (aux[..., 0], aux[..., 1]))
    want = cpu.closed_forms(*cpu.scalars_of(alpha, beta))
    for k in "abc":
        g_x, g_LP = cpu.cotangents_of(k, ref["x"])
        d = run_head(alpha, beta, 0, i, g_x, g_LP, seed=cpu.SEED)
        got = (d["g_alpha"], d["g_beta"])
        assert all(np.isfinite(g).all() for g in got)
        ratios = cpu.mean_errors(got, want[k], grads[k])
        tie = cpu.mean_errors(got, [float(np.mean(g)) for g in grads[k]], grads[k])
        print(f"cell {cpu.CELLS[i][0]} identity ({k}) device: |mean - closed form| / SE = {ratios[0]:.2f} (g_alpha), {ratios[1]:.2f} "
              f"(g_beta); |mean - the reference's mean| / SE = {tie[0]:.4f}, {tie[1]:.4f}")
        assert max(ratios) <= 6.0, (cpu.CELLS[i][0], k, ratios)
        assert max(tie) <= 0.5, (cpu.CELLS[i][0], k, tie)
