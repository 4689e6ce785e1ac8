"""The LAW of the Beta head's sampler, on the CPU twins (tests/np_twin_beta.py: search_lazy + compose): x is a Beta(a, b) sample and
each log-gamma a log Gamma(c, 1) sample, by scipy's CDFs (tests/np_law.py) -- not by the twins, which restate the kernel's algorithm
and would share its mistakes.  The device's own numbers: tests/test_gpu_beta_head_law.py, which takes its cells, seeds and closed
forms from this file.

Every Kolmogorov assertion is KS <= dkw(N) (the Dvoretzky-Kiefer-Wolfowitz bound at 1e-6 per statistic), every correlation
|corr| <= corr_bound(N) = 5.5 / sqrt(N), every gradient mean within 6 standard errors of its closed form, the standard error from
the float64 reference's own gradients.  N = 2^20 per cell (dkw = 2.63e-3): at 2^17 the rejection step is invisible above c = 2.

Measured at N = 2^20, as ratios to the bound (the figures the tests print; none of them sets a bound):
    cells, both twins      worst KS / dkw 0.51 (lg_1 of the cell (1e-3, 0.05)), of x 0.47 (the cell (7, 40)); the float32 twin's
                           ratios equal the float64 twin's to 1e-3;  worst |corr| / corr_bound 0.36
    pooled ranges          worst KS / dkw 0.51 ("small", lg_1); trainer 0.25, large 0.32, mixed 0.33
    controls, worst KS / dkw of lg_0, lg_1 per cell (refused where > 1; the float64 search with ONE line wrong), the cells in
    the order (1e-3, 0.05), (0.3, 0.999), seam, (0.5, 0.5), (1.5, 2.5), (7, 40), (40, 300):
        (i)   no_squeeze     1.44    3.87   9.32    3.55   5.63   0.89   0.38     (invisible from c = 7 on, as at 2^17 from 2.5 on)
        (ii)  no_half_zn2    1.81   15.85  31.68   11.21  31.44  31.62  31.56
        (iii) d_is_cb        6.95   26.36  56.09   24.44  44.37  19.68   8.20
        (iv)  no_boost     377.41  218.74   0.35  184.02   0.26   0.31   0.37     (cells without a concentration below 1: untouched)
        (v)   boost_cb     376.57  154.40   0.35  111.26   0.26   0.31   0.37
    gradient means         worst |mean - closed form| / SE over (a), (b), (c), g_alpha and g_beta: 1.54 on (1.5, 2.5), 1.19 on
                           (7, 40), 2.22 on (0.8, 0.9).  Identity (c) on (0.8, 0.9) is KEPT: 0.66 and 1.48 SE; the clamp binds on 5
                           of its 2^20 samples
    dlg scaled by 1 + s    worst of (a), (b) over the three cells: s = 1e-4: 2.38 SE, 3e-4: 3.06, 1e-3: 8.12, 3e-3: 22.59,
                           1e-2: 73.21 -- the smallest refused scale of that ladder is 1e-3"""
import math

import numpy as np
import pytest
from scipy import special

from tests import np_law as law
from tests import np_twin_beta as tb

F, D = np.float32, np.float64
SEED = 0x5EED0123456789
N = 2 ** 20


def raw(c):
    """The float32 raw operand whose positive_range is the concentration c: c itself from 1 on, 1 + log(c - eps) below."""
    return F(c) if c >= 1 else F(1.0 + math.log(c - tb.EPS32))


# (name, raw alpha, raw beta); `draw` is the cell's index in this tuple.  The seam: alpha = 1 is the first operand WITHOUT boost
# (pr(t) = t from t = 1 on) and pr(nextafter(1, 0)) = exp(-2^-24) + 2^-23 is 1 + 2^-24 in float64 and rounds to 1 in float32: the last
# operand of the exponential branch lands at or just above 1, without boost too.
CELLS = (("1e-3,0.05", raw(1e-3), raw(0.05)),
         ("0.3,0.999", raw(0.3), raw(0.999)),
         ("seam", F(1), np.nextafter(F(1), F(0))),
         ("0.5,0.5", raw(0.5), raw(0.5)),
         ("1.5,2.5", raw(1.5), raw(2.5)),
         ("7,40", raw(7), raw(40)),
         ("40,300", raw(40), raw(300)),
         ("0.8,0.9", raw(0.8), raw(0.9)))              # the gradient identities' third cell only (raw operands below 1: pr' enters)
LAW_CELLS = tuple(range(7))
GRAD_CELLS = (4, 5, 7)
POOLED = {kind: (100 + i, 16 + i) for i, kind in enumerate(tb.RANGES)}          # range -> (operand seed, draw)
CONTROLS = {"no_squeeze": ("no_squeeze", None), "no_half_zn2": ("no_half_zn2", None), "d_is_cb": ("d_is_cb", "d_is_cb"),
            "no_boost": (None, "no_boost"), "boost_cb": (None, "boost_cb")}     # name -> (search_lazy's defect, compose's defect)
X_LAW_FROM = 0.3            # below this concentration x saturates at 0 and 1 in float32: its law is tested through lg alone


def cell_operands(i, n=N):
    _, ta, tb_ = CELLS[i]
    return np.full((1, n), ta, F), np.full((1, n), tb_, F)


def concentrations(alpha, beta):
    """[n][pix][2] float64 (a, b) = positive_range of the float32 operands, and pr' -- the definition, whatever the sampler did."""
    t = np.stack([alpha, beta], axis=-1)
    return tb._pr(t, D)


def law_stats(c, lg, x=None):
    """The statistics of one sample set as ratios to their bounds: {name: KS / dkw or |corr| / corr_bound}.  c, lg [n][pix][2]; x
    [n][pix] or None (its law is left to lg).  y = 1 - x is recomputed in float64 from the two lg."""
    n = lg.shape[0] * lg.shape[1]
    lg = np.asarray(lg, D)
    p = [law.pit_log_gamma(c[..., j], lg[..., j]).ravel() for j in (0, 1)]
    out = {f"KS lg_{j}": law.ks_uniform(p[j]) / law.dkw(n) for j in (0, 1)}
    if x is not None:
        with np.errstate(over="ignore"):
            y = 1.0 / (1.0 + np.exp(lg[..., 0] - lg[..., 1]))
        out["KS x"] = law.ks_uniform(law.pit_beta(c[..., 0], c[..., 1], np.asarray(x, D), y)) / law.dkw(n)
    out["corr lg_0 lg_1"] = abs(law.corr(p[0], p[1])) / law.corr_bound(n)
    for j in (0, 1):
        out[f"corr lg_{j} neighbour"] = abs(law.corr(p[j][:-1], p[j][1:])) / law.corr_bound(n - 1)
    return out


def twin_sample(alpha, beta, draw, dtype, control=None, cache=None):
    """(lg [n][pix][2], x [n][pix]) of the twin's sampler in `dtype`: search_lazy's accepted draws through compose."""
    sd, cd = CONTROLS[control] if control else (None, None)
    key = (np.dtype(dtype).name, sd)
    if cache is None or key not in cache:
        sch = tb.search_lazy(alpha, beta, SEED, draw, dtype, defect=sd, cache=cache)
        if cache is None:
            return _composed(alpha, beta, sch, dtype, cd)
        cache[key] = sch
    return _composed(alpha, beta, cache[key], dtype, cd)


def _composed(alpha, beta, sch, dtype, cd):
    c = tb.compose(alpha, beta, (sch["zn"], sch["ub"]), dtype, defect=cd)
    return c["lg"], c["x"]


_results = {}


def cell_result(i):
    """{(twin or control, statistic): ratio} of law cell i: the float64 and the float32 twin's full statistics, every control's KS of
    lg_0 and lg_1 (the float64 search with the one line wrong).  Computed once."""
    if i not in _results:
        alpha, beta = cell_operands(i)
        c, _ = concentrations(alpha, beta)
        with_x = float(c.min()) >= X_LAW_FROM * (1 - 2e-6)            # (the cell (0.3, 0.999) is 0.3 up to the rounding of its raw operand)
        cache, out = {}, {}
        for name, dt in (("float64", D), ("float32", F)):
            lg, x = twin_sample(alpha, beta, i, dt, cache=cache)
            out.update({(name, k): v for k, v in law_stats(c, lg, x if with_x else None).items()})
        for control in CONTROLS:
            lg, _ = twin_sample(alpha, beta, i, D, control, cache=cache)
            for j in (0, 1):
                out[(control, f"KS lg_{j}")] = law.ks_uniform(law.pit_log_gamma(c[..., j], lg[..., j])) / law.dkw(N)
        for (who, k), v in out.items():
            print(f"cell {CELLS[i][0]} {who} {k}: {v:.3f} of its bound")
        _results[i] = out
    return _results[i]


@pytest.mark.parametrize("kind", list(tb.RANGES))
def test_search_lazy_is_search(kind):
    """k, zn and ub of the lazy search equal search's on the words of the same (seed, draw, first_object), in both dtypes, on the
    shapes of tests/test_beta_head_cpu.py's cases (and with a first_object)."""
    n, pix, seed = 4, 4096, 11
    alpha, beta = tb.operands(kind, n, pix, seed)
    for draw, fo in ((0, 0), (3, 7)):
        w = tb.words(n, pix, seed, draw, fo)
        for dt in (F, D):
            want, got = tb.search(alpha, beta, w, dt), tb.search_lazy(alpha, beta, seed, draw, dt, first_object=fo)
            assert (want["k"] > 0).any()
            for k in ("k", "zn", "ub"):
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (kind, dt, k)


def test_the_cells_are_the_stated_concentrations():
    for i, want in enumerate(((1e-3, 0.05), (0.3, 0.999), (1.0, 1.0), (0.5, 0.5), (1.5, 2.5), (7, 40), (40, 300), (0.8, 0.9))):
        a, b = (float(v) for v in concentrations(*cell_operands(i, 1))[0].ravel())
        assert abs(a / want[0] - 1) <= 2e-6 and abs(b / want[1] - 1) <= 2e-6, (i, a, b)
    _, ta, tb_ = CELLS[2]
    c32, _ = tb._pr(np.array([ta, tb_]), F)
    c64, _ = tb._pr(np.array([ta, tb_]), D)
    assert ta == 1 and tb_ < 1 and c32[0] == 1 and 1 <= c32[1] <= 1 + 2.0 ** -22 and 1 < c64[1] < 1 + 2.0 ** -23      # the seam: neither gamma is boosted
    ref = tb.compose(*cell_operands(2, 1), (np.zeros((1, 1, 2), F), np.full((1, 1, 2), 0.25, F)), F)
    assert (ref["boost"] == 0).all()


@pytest.mark.parametrize("i", LAW_CELLS, ids=[CELLS[i][0] for i in LAW_CELLS])
def test_cell_follows_the_gamma_and_beta_laws(i):
    """Both twins: KS of the PIT of lg_0, lg_1 (and x from concentration 0.3 on) <= dkw(N); the two gammas' PITs, and each gamma's
    PITs of neighbouring pixels, are uncorrelated within corr_bound(N)."""
    r = cell_result(i)
    seen = 0
    for (who, k), v in r.items():
        if who in ("float64", "float32"):
            seen += 1
            assert v <= 1.0, (CELLS[i][0], who, k, v)
    assert seen == 2 * (6 if ("float64", "KS x") in r else 5)
    assert (("float64", "KS x") in r) == (i != 0)


@pytest.mark.parametrize("kind", list(tb.RANGES))
def test_pooled_range_follows_the_gamma_law(kind):
    """2^20 pixels with operands uniform on the raw range: the pooled PITs of each gamma's logarithm are uniform, both twins."""
    seed, draw = POOLED[kind]
    alpha, beta = tb.operands(kind, 1, N, seed)
    c, _ = concentrations(alpha, beta)
    cache = {}
    for name, dt in (("float64", D), ("float32", F)):
        lg, _ = twin_sample(alpha, beta, draw, dt, cache=cache)
        for j in (0, 1):
            ratio = law.ks_uniform(law.pit_log_gamma(c[..., j], lg[..., j])) / law.dkw(N)
            print(f"pooled {kind} {name} KS lg_{j}: {ratio:.3f} of dkw")
            assert ratio <= 1.0, (kind, name, j, ratio)


@pytest.mark.parametrize("control", list(CONTROLS))
def test_the_law_test_bites(control):
    """A sampler with one line wrong is refused by the KS assertion in at least one cell: (i) the first attempt with w > 0 taken
    without the squeeze, (ii) the squeeze without 0.5 zn^2, (iii) d = cb, (iv) no boost, (v) the boost divided by cb."""
    worst = {CELLS[i][0]: max(cell_result(i)[(control, f"KS lg_{j}")] for j in (0, 1)) for i in LAW_CELLS}
    print(f"control {control}: worst KS / dkw per cell " + ", ".join(f"{k}: {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) > 1.0, (control, worst)


# ---- the gradient means ----------------------------------------------------------------------------------------------------------
def closed_forms(a, b, da, db):
    """{identity: (mean g_alpha, mean g_beta)} for scalar concentrations a, b and slopes pr'(alpha), pr'(beta):
    (a) d E[x], (b) d E[x^2], (c) d (-entropy) = d E[lp]."""
    s = a + b
    m2 = a * (a + 1) / (s * (s + 1))
    tri = lambda v: float(special.polygamma(1, v))                                        # noqa: E731
    return {"a": (da * b / s ** 2, -db * a / s ** 2),
            "b": (da * m2 * (1 / a + 1 / (a + 1) - 1 / s - 1 / (s + 1)), db * m2 * (-1 / s - 1 / (s + 1))),
            "c": (da * ((a - 1) * tri(a) - (s - 2) * tri(s)), db * ((b - 1) * tri(b) - (s - 2) * tri(s)))}


def cotangents_of(identity, x):
    """(g_x [n][pix], g_LP [n]) of the identity: (a) g_x = 1, (b) g_x = 2 x, (c) G = 1."""
    n = x.shape[0]
    if identity == "a":
        return np.ones(x.shape, F), np.zeros(n, F)
    if identity == "b":
        return (2 * x).astype(F), np.zeros(n, F)
    return np.zeros(x.shape, F), np.ones(n, F)


def scalars_of(alpha, beta):
    c, dc = concentrations(alpha, beta)
    return float(c[0, 0, 0]), float(c[0, 0, 1]), float(dc[0, 0, 0]), float(dc[0, 0, 1])


def reference_gradients(alpha, beta, draws):
    """The float64 composition at `draws`, its dlg (computed once) and {identity: (g_alpha, g_beta)} float64 [n][pix]."""
    ref = tb.compose(alpha, beta, draws, D)
    dl = (tb.dlg(ref["a"], ref["lg"][..., 0]), tb.dlg(ref["b"], ref["lg"][..., 1]))
    return ref, dl, {k: tb.gradients(ref, *cotangents_of(k, ref["x"]), dlg_=dl) for k in "abc"}


_grad = {}


def grad_cell(i):
    if i not in _grad:
        alpha, beta = cell_operands(i)
        sch = tb.search_lazy(alpha, beta, SEED, i, D)
        _grad[i] = (alpha, beta) + reference_gradients(alpha, beta, (sch["zn"], sch["ub"]))
    return _grad[i]


def mean_errors(g, want, ref_g):
    """|mean of g - closed form| / SE for (g_alpha, g_beta); SE = the float64 REFERENCE gradients' (ref_g) own standard deviation /
    sqrt(N), whatever g is (the reference itself, a defective twin, the device)."""
    se = [float(np.std(v.astype(D))) / math.sqrt(v.size) for v in ref_g]
    return [abs(float(np.mean(v.astype(D))) - w) / s for v, w, s in zip(g, want, se)]


@pytest.mark.parametrize("i", GRAD_CELLS, ids=[CELLS[i][0] for i in GRAD_CELLS])
def test_gradient_means_are_the_derivatives_of_the_moments(i):
    """The float64 twin at its own draws, sr = eps: the means of g_alpha and g_beta over 2^20 samples are, within 6 standard errors,
    (a) the derivatives of E[x] = a / (a + b), (b) of E[x^2], (c) of minus the entropy, each times pr'."""
    alpha, beta, ref, dl, grads = grad_cell(i)
    assert np.isfinite(dl[0]).all() and np.isfinite(dl[1]).all()
    print(f"cell {CELLS[i][0]}: the clamp binds on {int((~ref['passes']).sum())} of {N} samples")
    want = closed_forms(*scalars_of(alpha, beta))
    for k in "abc":
        ratios = mean_errors(grads[k], want[k], grads[k])
        print(f"cell {CELLS[i][0]} identity ({k}): |mean - closed form| / SE = {ratios[0]:.2f} (g_alpha), {ratios[1]:.2f} (g_beta)")
        assert max(ratios) <= 6.0, (CELLS[i][0], k, ratios)


def test_the_gradient_means_bite():
    """dlg scaled by 1 + s (gradients' defect "dlg_1e-4" scaled up): s = 1e-2 is refused by identity (a) or (b) on at least one cell.
    The ladder of scales is printed; the smallest refused one is recorded in this file's docstring."""
    refused = {}
    for s in (1e-4, 3e-4, 1e-3, 3e-3, 1e-2):
        worst = 0.0
        for i in GRAD_CELLS:
            alpha, beta, ref, dl, grads = grad_cell(i)
            want = closed_forms(*scalars_of(alpha, beta))
            for k in "ab":
                g = tb.gradients(ref, *cotangents_of(k, ref["x"]), defect="dlg_1e-4", defect_scale=s / 1e-4, dlg_=dl)
                worst = max(worst, max(mean_errors(g, want[k], grads[k])))
        refused[s] = worst
        print(f"dlg scaled by 1 + {s:g}: worst |mean - closed form| / SE over (a), (b) = {worst:.2f}")
    assert refused[1e-2] > 6.0, refused
