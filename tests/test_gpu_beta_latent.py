"""The fused Beta latent block on the device (ct_pvae_amd/beta_latents.py, csrc/beta_latent.hip) against the twins of
tests/np_twin_beta_latent.py: the draws against the numpy Philox under the latents' counter word, every value and gradient against the
float64 composition evaluated AT THE DEVICE'S ACCEPTED DRAWS under that file's per-sample rule |got - ref| <= 4 R bar, the fixed order
of the per-object sum, reproducibility, split and sample-count invariance, want_kl=False, a NaN operand, the iteration bound of the
implicit gradient, the law of z and of its gradient, and the trainer with --fused_beta_latents.

Measured on an MI355X, as ratios to the bound (the figures the tests print; none of them sets a bound): worst |got - ref| / bar over
all shapes and ranges 0.72 (z), 0.99 (kl: its bar is the final rounding), 0.31 (g_loc), 0.34 (g_ls), R <= 1.003 (bound 4 R); the
accepted attempt differs from the float64 search on no gamma; law cells: worst KS / dkw 0.34, worst |corr| / corr_bound 0.35
(levels 0 and 1 at (0.7, 3)); controls: s dropped 93 times the bound, gamma on the attempt's low bit 1.23 times; gradient means
0.33 and 0.76 SE from the closed form; the trainer's kl within 0.04 of its tolerance, its loglik bit-equal."""
import math

import numpy as np
import pytest
import torch
from scipy import special

from ct_pvae_amd import beta_latents
from ct_pvae_amd import trainer as tr
from tests import np_law as law
from tests import np_twin_beta as tb
from tests import np_twin_beta_latent as tbl
from tests import np_twin_hmc

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
SEED = 0x5EED0123456789
DRAW = 5
#          B  C  H   W   ns first_object level
SHAPES = {"1x1x1x3": (1, 1, 1, 3, 1, 0, 0),                      # one ragged quad
          "3x1x5x7": (3, 1, 5, 7, 2, 2, 3),                      # len 35: every row after the first is misaligned
          "2x2x8x8": (2, 2, 8, 8, 3, 0, 255),
          "2x1x41x100": (2, 1, 41, 100, 2, (2 ** 32) // 4100, 1)}   # len 4100 = 1025 quads: a KL thread takes a second quad, five sample
#                                                                   workgroups per row, the last with 4 elements; e crosses 2^32 in object 0
_cases = {}


def _dev():
    return torch.device("cuda", 0)


def run_latents(loc, ls, ns, first_object, level, chw, g_z=None, g_KL=None, draw=DRAW, seed=SEED, want_kl=True):
    """The device's results as numpy arrays: z [ns][B][len], KL [B], kl [B][len], aux [ns][B][len][2][4], g_loc, g_ls [B][len] (when
    a cotangent is given), all through the autograd function (kl_elem and aux by its private keyword)."""
    B, length = loc.shape
    C, H, W = chw
    assert C * H * W == length
    dev = _dev()
    skip = torch.from_numpy(np.stack([loc, ls], axis=1)).to(dev).reshape(B, 2 * C, H, W).requires_grad_(True)
    ex = {}
    z, KL = beta_latents(skip, ns=ns, seed=seed, draw=draw, level=level, first_object=first_object, want_kl=want_kl, _extras=ex)
    assert z.shape == (ns * B, C, H, W) and z.dtype == torch.float32
    out = dict(z=z.detach().reshape(ns, B, length).cpu().numpy(), aux=ex["aux"].reshape(ns, B, length, 2, 4).cpu().numpy(), KL=None, kl=None)
    if want_kl:
        assert KL.shape == (B,) and KL.dtype == torch.float32
        out["KL"], out["kl"] = KL.detach().cpu().numpy(), ex["kl_elem"].cpu().numpy()
    else:
        assert KL is None and ex["kl_elem"] is None
    if g_z is not None or g_KL is not None:
        loss = 0.0
        if g_z is not None:
            loss = loss + (z.reshape(ns, B, length) * torch.from_numpy(g_z).to(dev)).sum()
        if g_KL is not None:
            loss = loss + (KL * torch.from_numpy(g_KL).to(dev)).sum()
        g, = torch.autograd.grad(loss, skip)
        g = g.reshape(B, 2, length).cpu().numpy()
        out["g_loc"], out["g_ls"] = g[:, 0], g[:, 1]
    return out


def device_case(shape, kind):
    """One (shape, range): the device's results with both cotangents, and the CPU reference at the device's accepted draws (computed
    once, shared, left unchanged)."""
    key = (shape, kind)
    if key not in _cases:
        B, C, H, W, ns, fo, level = SHAPES[shape]
        length = C * H * W
        loc, ls = tbl.operands(kind, B, length, 17)
        g_z, g_KL = tbl.cotangents(ns, B, length, 18)
        dev = run_latents(loc, ls, ns, fo, level, (C, H, W), g_z, g_KL)
        c = tbl.case(kind, B, length, ns, 17, draws=(dev["aux"][..., 0], dev["aux"][..., 1]))
        assert np.array_equal(c["loc"], loc) and np.array_equal(c["g_z"], g_z) and np.array_equal(c["g_KL"], g_KL)
        c["dev"], c["shape"] = dev, SHAPES[shape]
        _cases[key] = c
    return _cases[key]


@pytest.mark.parametrize("kind", list(tbl.RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_draws_are_the_numpy_philox_at_the_reported_attempt(shape, kind):
    """aux's ub equals the numpy Philox draw under the latents' counter word bit for bit at the attempt k the device reports, for every
    sample s -- at levels 0, 3, 255 and 1, and with e crossing 2^32 (the 4100-element shape); zn is the device's normcdfinvf of the numpy
    u24(word 0), held to 4 ulps of the float64 ndtri of that uniform as in tests/test_gpu_beta_head.py.  k equals the float64 search on all
    but at most 1e-4 of the gammas, and every disagreement is a draw whose float64 acceptance margin is inside its own bar."""
    c = device_case(shape, kind)
    B, C, H, W, ns, fo, level = SHAPES[shape]
    length = C * H * W
    for s in range(ns):
        w = tbl.words(B, length, SEED, DRAW, level, s, fo)
        aux = c["dev"]["aux"][s]
        k = aux[..., 2].astype(np.int64)
        assert ((k >= 0) & (k < tbl.ATTEMPTS)).all() and np.array_equal(k.astype(F), aux[..., 2])
        at = np.take_along_axis(w, k[..., None, None], axis=3)[:, :, :, 0]                     # [B][len][2][4]
        assert np.array_equal(np_twin_hmc.u24(at[..., 2]).view(np.uint32), aux[..., 1].view(np.uint32)), (shape, kind, s)
        zn64 = special.ndtri(np_twin_hmc.u24(at[..., 0]).astype(D))
        assert (np.abs(aux[..., 0] - zn64) <= 4 * tb.U * (1 + np.abs(zn64))).all()
        s64 = tb.search(c["loc"], c["ls"], w, D)
        dis = k != s64["k"]
        print(f"{shape} {kind} s={s}: k differs on {int(dis.sum())} of {dis.size} gammas; attempts used: {np.bincount(k.ravel()).tolist()}")
        assert dis.sum() <= 1e-4 * dis.size
        first = np.minimum(k, s64["k"])[..., None]
        m = np.take_along_axis(s64["margin"], first, axis=-1)[..., 0]
        b = np.take_along_axis(s64["bar"], first, axis=-1)[..., 0]
        assert (np.abs(m[dis]) <= tb.MARGIN * b[dis]).all()
        assert np.isfinite(aux[..., 3]).all()
    if fo:
        assert shape != "2x1x41x100" or (fo * length < 2 ** 32 < (fo + B) * length)


def _assert_within_bars(tag, dev, c, quantities):
    for k in quantities:
        worst = float(np.max(tb.excess(dev[k], c["want"][k], c["bar"][k])))
        print(f"{tag} {k}: worst |got - ref| / bar = {worst:.3f}, R = {c['R'][k]:.3f}")
        assert c["R"][k] <= tbl.R_MAX
        assert np.isfinite(dev[k]).all(), k                               # (also: no element left at its NaN poison)
        assert worst <= tbl.MARGIN * c["R"][k], (k, worst, c["R"][k])


@pytest.mark.parametrize("kind", list(tbl.RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_sample_within_its_bar_of_float64(shape, kind):
    """z, kl_elem, g_skip[loc] and g_skip[log_scale] against the float64 composition evaluated at the device's accepted draws, with both
    cotangents."""
    c = device_case(shape, kind)
    _assert_within_bars(f"{shape} {kind}", c["dev"], c, ("z", "kl", "g_loc", "g_ls"))


@pytest.mark.parametrize("shape", ["3x1x5x7", "2x2x8x8"])
def test_each_cotangent_alone_and_null_equals_zero(shape):
    """g_z only and g_KL only obey the same bars (the reference and the bars built for that cotangent alone), and a missing cotangent
    gives the same BITS as a zero one."""
    c = device_case(shape, "mixed")
    B, C, H, W, ns, fo, level = c["shape"]
    length = C * H * W
    draws = (c["dev"]["aux"][..., 0], c["dev"]["aux"][..., 1])
    for name, gz_on, gk_on in (("g_z only", True, False), ("g_KL only", False, True)):
        alone = tbl.case("mixed", B, length, ns, 17, draws=draws, g_z=gz_on, g_KL=gk_on)
        d = run_latents(c["loc"], c["ls"], ns, fo, level, (C, H, W), c["g_z"] if gz_on else None, c["g_KL"] if gk_on else None)
        _assert_within_bars(f"{shape} {name}", d, alone, ("g_loc", "g_ls"))
        zero = run_latents(c["loc"], c["ls"], ns, fo, level, (C, H, W), c["g_z"] if gz_on else np.zeros_like(c["g_z"]),
                           c["g_KL"] if gk_on else np.zeros_like(c["g_KL"]))
        for k in ("g_loc", "g_ls"):
            assert np.array_equal(zero[k].view(np.uint32), d[k].view(np.uint32)), (name, k)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_object_sum_is_the_stated_order_bit_for_bit(shape):
    c = device_case(shape, "mixed")
    want = np.array([tbl.ordered_sum(row) for row in c["dev"]["kl"]], F)
    assert np.array_equal(want.view(np.uint32), c["dev"]["KL"].view(np.uint32)), (want, c["dev"]["KL"])


def test_reproducible_split_and_sample_count_invariant():
    """Two calls give the same bits; the batch cut in two with first_object gives the whole batch's z, KL and g_skip (3 x 35: the cut's
    objects sit at another alignment); samples 0, 1 of ns = 3 are the two samples of ns = 2; another draw, level or seed draws other
    numbers; want_kl=False gives the same z and no KL."""
    c = device_case("3x1x5x7", "mixed")
    B, C, H, W, ns, fo, level = c["shape"]
    chw = (C, H, W)
    dev = c["dev"]
    again = run_latents(c["loc"], c["ls"], ns, fo, level, chw, c["g_z"], c["g_KL"])
    for k in ("z", "KL", "kl", "g_loc", "g_ls"):
        assert np.array_equal(again[k].view(np.uint32), dev[k].view(np.uint32)), k
    a = run_latents(c["loc"][:1], c["ls"][:1], ns, fo, level, chw, c["g_z"][:, :1], c["g_KL"][:1])
    b = run_latents(np.ascontiguousarray(c["loc"][1:]), np.ascontiguousarray(c["ls"][1:]), ns, fo + 1, level, chw,
                    np.ascontiguousarray(c["g_z"][:, 1:]), c["g_KL"][1:])
    assert np.array_equal(np.concatenate([a["z"], b["z"]], axis=1).view(np.uint32), dev["z"].view(np.uint32))
    for k in ("KL", "g_loc", "g_ls"):
        assert np.array_equal(np.concatenate([a[k], b[k]]).view(np.uint32), dev[k].view(np.uint32)), k
    three = run_latents(c["loc"], c["ls"], 3, fo, level, chw)
    assert np.array_equal(three["z"][:2].view(np.uint32), dev["z"].view(np.uint32))
    assert np.array_equal(three["KL"].view(np.uint32), dev["KL"].view(np.uint32))
    assert not np.array_equal(three["z"][2], three["z"][0]) and not np.array_equal(three["z"][2], three["z"][1])
    for kw in (dict(draw=DRAW + 1), dict(level=level + 1), dict(seed=SEED + 1)):
        args = dict(dict(draw=DRAW, level=level, seed=SEED), **kw)
        other = run_latents(c["loc"], c["ls"], ns, fo, args["level"], chw, draw=args["draw"], seed=args["seed"])
        assert not np.array_equal(other["z"], dev["z"]), kw
    nokl = run_latents(c["loc"], c["ls"], ns, fo, level, chw, c["g_z"], None, want_kl=False)
    assert nokl["KL"] is None and np.array_equal(nokl["z"].view(np.uint32), dev["z"].view(np.uint32))
    only = run_latents(c["loc"], c["ls"], ns, fo, level, chw, c["g_z"], None)
    for k in ("g_loc", "g_ls"):
        assert np.array_equal(nokl[k].view(np.uint32), only[k].view(np.uint32)), k
    big = device_case("2x1x41x100", "mixed")
    B, C, H, W, ns, fo, level = big["shape"]
    a = run_latents(big["loc"][:1], big["ls"][:1], ns, fo, level, (C, H, W))
    b = run_latents(np.ascontiguousarray(big["loc"][1:]), np.ascontiguousarray(big["ls"][1:]), ns, fo + 1, level, (C, H, W))
    assert np.array_equal(np.concatenate([a["z"], b["z"]], axis=1).view(np.uint32), big["dev"]["z"].view(np.uint32))
    assert np.array_equal(np.concatenate([a["KL"], b["KL"]]).view(np.uint32), big["dev"]["KL"].view(np.uint32))


def test_one_nan_operand_stays_in_its_element_and_its_objects_sum():
    """One NaN loc: that element's z is NaN in every sample, its object's KL is NaN, its two gradients are NaN, and nothing else moves;
    the call returns (the attempt loop leaves after 16 refusals)."""
    c = device_case("3x1x5x7", "mixed")
    B, C, H, W, ns, fo, level = c["shape"]
    loc = c["loc"].copy()
    loc[1, 9] = np.nan
    d = run_latents(loc, c["ls"], ns, fo, level, (C, H, W), c["g_z"], c["g_KL"])
    hit = np.zeros(loc.shape, bool)
    hit[1, 9] = True
    assert np.isnan(d["z"][:, hit]).all() and np.isnan(d["KL"][1]) and np.isnan(d["kl"][hit]).all()
    assert (d["aux"][:, 1, 9, 0, 2] == tbl.ATTEMPTS - 1).all()
    assert np.array_equal(d["z"][:, ~hit].view(np.uint32), c["dev"]["z"][:, ~hit].view(np.uint32))
    assert np.array_equal(d["KL"][[0, 2]].view(np.uint32), c["dev"]["KL"][[0, 2]].view(np.uint32))
    assert np.array_equal(d["kl"][~hit].view(np.uint32), c["dev"]["kl"][~hit].view(np.uint32))
    assert np.isnan(d["g_loc"][hit]).all() and np.isnan(d["g_ls"][hit]).all()
    for k in ("g_loc", "g_ls"):
        assert np.array_equal(d[k][~hit].view(np.uint32), c["dev"][k][~hit].view(np.uint32)), k


def test_iteration_bound_of_the_implicit_gradient():
    """kDlgMaxTerms = 2048 iterations serve every concentration up to 4e4: at a = 3e4 values and gradients obey their bars.  At
    a = 2e5 the series would need about 4200: a sample whose draw lies below a + 1 takes the series, the kernel stops at its bound and the
    element's g_loc is NaN, not a truncated sum (an element all of whose draws lie above takes the continued fraction and stays
    right); z, kl, g_log_scale and every other element stay finite and inside their bars."""
    B, length, ns = 1, 8, 2
    loc = np.array([[3e4] * 4 + [2e5] * 4], F)
    ls = np.full((B, length), 2.0, F)
    g_z, g_KL = tbl.cotangents(ns, B, length, 8)
    d = run_latents(loc, ls, ns, 0, 2, (1, 1, length), g_z, g_KL, draw=3)
    c = tbl.case(None, B, length, ns, 7, draws=(d["aux"][..., 0], d["aux"][..., 1]), operands_=(loc, ls))
    assert np.array_equal(c["g_z"], g_z)
    ok = np.arange(length) < 4
    for k in ("z", "kl", "g_loc", "g_ls"):
        cols = ok if k == "g_loc" else np.ones(length, bool)
        worst = float(np.max(tb.excess(d[k], c["want"][k], c["bar"][k])[..., cols]))
        print(f"a = 3e4 / 2e5 {k}: worst {worst:.3f}, R = {c['R'][k]:.3f}")
        assert worst <= tbl.MARGIN * c["R"][k], (k, worst)
    series = np.zeros(length, bool)
    for p in c["ref"]["s"]:
        series |= (np.exp(p["lg"][0, :, 0]) <= p["a"][0] + 1)
    far = ~ok
    assert (series & far).any() and np.isnan(d["g_loc"][0, series & far]).all() and np.isfinite(c["want"]["g_loc"]).all()
    e = tb.excess(d["g_loc"], c["want"]["g_loc"], c["bar"]["g_loc"])[0]
    assert (e[far & ~series] <= tbl.MARGIN * c["R"]["g_loc"]).all()


# ---- the law ----------------------------------------------------------------------------------------------------------------------
N = 2 ** 20
CELLS = {"(0.05, 0.05)": (0.05, 0.05), "(0.7, 3)": (0.7, 3.0), "(40, 300)": (40.0, 300.0)}
GRAD_CELLS = ("(0.7, 3)", "(40, 300)")
LAW_SEED, LAW_DRAW = 0x1A770000BEEF, 11
_law = {}


def cell_operands(name, n=N):
    """float32 raw operands [1][n] whose positive_range is the cell's (a, b) up to float32 rounding."""
    raw = [c if c >= 1 else 1.0 + math.log(c - tb.EPS32) for c in CELLS[name]]
    return np.full((1, n), raw[0], F), np.full((1, n), raw[1], F)


def pits(loc, ls, z, lg):
    """PIT of z [ns][1][n] under Beta(a, b) of the float32 concentrations: I_z(a, b) below 0.5, 1 - I_y(b, a) above, y = 1 - z taken
    without cancellation from the sampler's own lg, in float64; where the float32 z has rounded to 0 (or below the normal range: an atom
    of the rounding, not of the law, 0.6 % at (0.05, 0.05)) z too is the float64 sigmoid of those lg."""
    a, b = tb._pr(loc, D)[0], tb._pr(ls, D)[0]
    dl = lg[..., 1].astype(D) - lg[..., 0].astype(D)
    with np.errstate(over="ignore"):
        z64, y64 = 1.0 / (1.0 + np.exp(dl)), 1.0 / (1.0 + np.exp(-dl))
    x = np.where(z < tb.TINY, z64, z.astype(D))
    return law.pit_beta(a[None], b[None], x, y64)


def gamma_pits(loc, ls, lg):
    """The PITs of the two log-gammas of one sample, lg [1][n][2]."""
    return law.pit_log_gamma(tb._pr(loc, D)[0], lg[..., 0]), law.pit_log_gamma(tb._pr(ls, D)[0], lg[..., 1])


def law_stats(p, p_other_level, pg):
    """Every statistic as a ratio to its bound: KS of the PITs of each sample, |corr| between s = 0 and s = 1, between levels, between
    neighbouring elements, and between the PITs of the two gammas of sample 0."""
    n = p.shape[-1]
    r = {f"KS s={s}": law.ks_uniform(p[s]) / law.dkw(n) for s in range(p.shape[0])}
    r["corr s=0|s=1"] = abs(law.corr(p[0], p[1])) / law.corr_bound(n)
    r["corr level 0|1"] = abs(law.corr(p[0], p_other_level)) / law.corr_bound(n)
    r["corr neighbours"] = abs(law.corr(p[0, 0, :-1], p[0, 0, 1:])) / law.corr_bound(n - 1)
    r["corr gammas"] = abs(law.corr(*pg)) / law.corr_bound(n)
    return r


def device_law(name):
    if name not in _law:
        loc, ls = cell_operands(name)
        d0 = run_latents(loc, ls, 2, 0, 0, (1, 1024, 1024), draw=LAW_DRAW, seed=LAW_SEED)
        d1 = run_latents(loc, ls, 1, 0, 1, (1, 1024, 1024), draw=LAW_DRAW, seed=LAW_SEED)
        assert np.isfinite(d0["z"]).all() and np.isfinite(d0["aux"][..., 3]).all()
        _law[name] = (loc, ls, d0, pits(loc, ls, d0["z"], d0["aux"][..., 3]), pits(loc, ls, d1["z"], d1["aux"][..., 3])[0])
    return _law[name]


@pytest.mark.parametrize("name", list(CELLS))
def test_z_follows_the_beta_law_and_its_samples_are_independent(name):
    """One launch of 2^20 elements, ns = 2 (and one of level 1): KS of the PIT of z under Beta(a, b1) <= dkw(N) for each sample; the
    PITs of s = 0 and s = 1, of levels 0 and 1 and of neighbouring elements uncorrelated within 5.5 / sqrt(N) -- the statistics a wrong
    packing of the counter word breaks (the controls below)."""
    loc, ls, d0, p, p1 = device_law(name)
    r = law_stats(p, p1, gamma_pits(loc, ls, d0["aux"][0][..., 3]))
    for k, v in r.items():
        print(f"cell {name} device {k}: {v:.3f} of its bound")
    assert len(r) == 6
    for k, v in r.items():
        assert v <= 1.0, (name, k, v)


def _host_sample(loc, ls, level, s, defect):
    sch = tbl.search_lazy(loc, ls, LAW_SEED, LAW_DRAW, level, s, F, defect=defect)
    c = tb.compose(loc, ls, (sch["zn"], sch["ub"]), F)
    return c["x"], c["lg"]


@pytest.mark.parametrize("defect", [d for d in tbl.SEARCH_DEFECTS if d is not None])
def test_a_wrong_packing_of_the_counter_word_is_refused(defect):
    """The controls, restated on the host with the twin's search_lazy (the kernel is not broken for them), at the cell (0.7, 3) with
    2^18 elements (the bounds are those of that size): with the sample index dropped from the word s = 1 repeats s = 0; with the gamma
    bit overlapping the attempt's lowest bit the second gamma's first attempt is the first gamma's second.  Each must push at least one
    statistic of the law test past its bound -- and the right packing, through the same host code, none."""
    name = "(0.7, 3)"
    loc, ls = cell_operands(name, 2 ** 18)

    def stats(d):
        zs, lgs = zip(*(_host_sample(loc, ls, 0, s, d) for s in (0, 1)))
        z1, lg1 = _host_sample(loc, ls, 1, 0, d)
        return law_stats(pits(loc, ls, np.stack(zs), np.stack(lgs)), pits(loc, ls, z1[None], lg1[None])[0], gamma_pits(loc, ls, lgs[0]))
    good, bad = stats(None), stats(defect)
    print(f"right packing: {good}\n{defect}: {bad}")
    assert max(good.values()) <= 1.0
    assert max(bad.values()) > 1.0, (defect, bad)


@pytest.mark.parametrize("name", GRAD_CELLS)
def test_gradient_mean_is_the_derivative_of_the_mean(name):
    """g_z = 1 on both samples: g_loc / ns averaged over the 2^20 elements is d E[z] / d a * pr'(loc) = b / (a + b)^2 * pr'(loc)
    within 6 standard errors, the standard error from the float64 reference's per-sample gradients at the device's accepted draws (not
    from the device's values), whose own mean the device's must match within 0.5 SE."""
    loc, ls, d0, _, _ = device_law(name)
    ns = 2
    g = run_latents(loc, ls, ns, 0, 0, (1, 1024, 1024), np.ones((ns, 1, N), F), None, draw=LAW_DRAW, seed=LAW_SEED)
    a, b = float(tb._pr(loc[:, :1], D)[0][0, 0]), float(tb._pr(ls[:, :1], D)[0][0, 0])
    da = float(tb._pr(loc[:, :1], D)[1][0, 0])
    want = b / (a + b) ** 2 * da
    M = 2 ** 18                                                           # the reference's gradients: the first 2^18 elements
    per = []
    for s in range(ns):
        ref = tb.compose(loc[:, :M], ls[:, :M], (d0["aux"][s][:, :M, :, 0], d0["aux"][s][:, :M, :, 1]), D)
        per.append(ref["x"] * ref["y"] * tb.dlg(ref["a"], ref["lg"][..., 0]) * da)
    per = np.stack(per)                                                   # [ns][1][M], the reference's gradient of each sample
    sd = float(per.std(ddof=1))
    se, se_m = sd / math.sqrt(ns * N), sd / math.sqrt(ns * M)
    got = float(np.mean(g["g_loc"].astype(D))) / ns
    got_m = float(np.mean(g["g_loc"][:, :M].astype(D))) / ns
    print(f"cell {name}: mean g_loc / ns {got:.6e}, closed form {want:.6e}, |diff| / SE {abs(got - want) / se:.2f}; on the first 2^18 "
          f"elements |mean - the reference's mean| / SE {abs(got_m - float(per.mean())) / se_m:.4f}")
    assert np.isfinite(g["g_loc"]).all()
    assert abs(got - want) <= 6.0 * se and abs(got_m - float(per.mean())) <= 0.5 * se_m


# ---- the trainer ------------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def test_find_loss_with_fused_beta_latents_matches_the_twin_fed_unfused_path(monkeypatch):
    """find_loss_vae_unsup(fused_beta_latents=(seed, draw, first_object)) against the UNFUSED branch of the same call whose
    Beta.rsample is replaced by the float64 twin's samples at the device's own accepted draws (level by level, sample-major, cast to
    float32); the output head is the fused Beta head under one key in both runs, so nothing else draws.  Level 0 is called without a
    KL.  Bars, propagated:
      kl[b]    sum over the levels >= 1 and the elements of 4 R bar_kl (the device against float64) + 8 U T (torch's float32
               _kl_beta_beta: a few ulps on each of its terms, T = ln pi + |lgamma a| + |lgamma b| + |lgamma(a + b)| + |(a - 1/2) psi(a)| +
               |(b - 1/2) psi(b)| + |(1 - a - b) psi(a + b)|) + the float32 sums' rounding 2 U log2(n) sum |kl|
      loglik   2 sum over all levels and elements of |d loglik / d z| (4 R bar_z + U |z|) (first order, from autograd of the unfused
               run, doubled for the maxouts' switches; U |z|: the twin's cast to float32) + 2 U log2(n) |loglik|
      loss     kl_anneal klm (kl's) + loglik's."""
    t = _small_trainer()
    ns, B = 2, 3
    seed, draw, fo = 99, 4, 6
    head_key = (seed, draw, 0)
    ps, m, ie = t._batch()
    angles_i = torch.from_numpy(np.ascontiguousarray(t.angles.next().astype(np.int32)))
    calls = []
    real = beta_latents

    def spy(skip, **kw):
        calls.append((kw["level"], kw["want_kl"]))
        return real(skip, **kw)
    monkeypatch.setattr(tr, "beta_latents", spy)
    common = dict(num_samples=ns, theta=t.theta_host, angles_i=angles_i, pad=t.pad, deterministic=False, use_normal=False,
                  fused_beta_head=head_key)
    with torch.no_grad():
        skips = [sk.contiguous() for sk in t.enc(ie / 300)]
        loss_f, kl_f, ll_f, _ = tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, fused_beta_latents=(seed, draw, fo),
                                                       **common)
    assert calls == [(level, level > 0) for level in range(len(skips))]
    # the twin at the device's draws, level by level
    twins, tol_kl = [], np.zeros(B)
    for level, sk in enumerate(skips):
        C, H, W = sk.shape[1] // 2, sk.shape[2], sk.shape[3]
        flat = sk.reshape(B, 2, C * H * W).cpu().numpy()
        ex = {}
        z_dev, _ = real(sk, ns=ns, seed=seed, draw=draw, level=level, first_object=fo, _extras=ex)
        aux = ex["aux"].reshape(ns, B, C * H * W, 2, 4).cpu().numpy()
        ref = tbl.compose(flat[:, 0], flat[:, 1], (aux[..., 0], aux[..., 1]), D)
        twin = tbl.compose(flat[:, 0], flat[:, 1], (aux[..., 0], aux[..., 1]), F)
        bar = tbl.bars(ref, None, None, values_only=True)
        R = {k: tb.twin_ratio(twin[k], ref[k], bar[k]) for k in ("z", "kl")}
        assert max(R.values()) <= tbl.R_MAX
        worst = float(np.max(tb.excess(z_dev.reshape(ns, B, -1).cpu().numpy(), ref["z"], bar["z"])))
        assert worst <= tbl.MARGIN * R["z"], (level, worst)
        twins.append((ref, tbl.MARGIN * R["z"] * bar["z"] + tb.U * np.abs(ref["z"]), (ns, B, C, H, W)))
        if level >= 1:
            a, b = ref["a"], ref["b"]
            T = (tbl.LN_PI + np.abs(special.gammaln(a)) + np.abs(special.gammaln(b)) + np.abs(special.gammaln(a + b)) + np.abs((a - 0.5) * special.digamma(a))
                 + np.abs((b - 0.5) * special.digamma(b)) + np.abs((1 - a - b) * special.digamma(a + b)))
            tol_kl += ((tbl.MARGIN * R["kl"] * bar["kl"] + 8 * tb.U * T).sum(axis=1)
                       + 2 * tb.U * math.log2(a.shape[1]) * np.abs(ref["kl"]).sum(axis=1))
    leaves, it = [], iter(twins)

    def twin_rsample(self, sample_shape=torch.Size()):
        ref, _, shape = next(it)
        assert tuple(sample_shape) == (ns,) and tuple(self.concentration1.shape) == (B,) + shape[2:]
        leaf = torch.from_numpy(ref["z"].astype(F)).to(t.dev).reshape(shape).requires_grad_(True)
        leaves.append(leaf)
        return leaf
    monkeypatch.setattr(torch.distributions.Beta, "rsample", twin_rsample)
    loss_u, kl_u, ll_u, _ = tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, **common)
    monkeypatch.undo()
    assert len(leaves) == len(skips)
    grads = torch.autograd.grad(ll_u, leaves)
    tol_ll = 2 * tb.U * math.log2(ie[0].numel() * B) * abs(float(ll_u.detach()))
    for g, (_, dz, shape) in zip(grads, twins):
        tol_ll += 2 * float((np.abs(g.double().cpu().numpy().reshape(dz.shape)) * dz).sum())
    d_kl = np.abs(kl_f.double().cpu().numpy() - kl_u.detach().double().cpu().numpy())
    d_ll = abs(float(ll_f) - float(ll_u.detach()))
    d_loss = np.abs(loss_f.double().cpu().numpy() - loss_u.detach().double().cpu().numpy())
    print(f"kl fused {kl_f.tolist()} twin-fed unfused {kl_u.tolist()} |diff| / tol {(d_kl / tol_kl).tolist()}")
    print(f"loglik fused {float(ll_f):.6f} twin-fed unfused {float(ll_u.detach()):.6f} |diff| {d_ll:.3e} tol {tol_ll:.3e}")
    assert (d_kl <= tol_kl).all()
    assert d_ll <= tol_ll
    assert (d_loss <= tol_kl + tol_ll).all()


def test_fused_beta_latents_training_run_is_finite_and_reproducible():
    """Three --fused_beta_latents --fused_beta_head steps: nothing in the step draws from torch's global generator, so two equal-seed
    runs under --reproducible (deterministic convolution algorithms) are bit-equal, losses and parameters, whatever that generator's
    state; the losses are finite.  With --fused_blocks and --dp on top the run stays finite."""
    runs = []
    was = torch.backends.cudnn.deterministic            # (--reproducible switches it on for the process: put back for the tests that follow)
    try:
        for k in range(2):
            t = _small_trainer("--fused_beta_latents --fused_beta_head --reproducible")
            torch.manual_seed(1000 + k)                 # the global generator is not part of the step: another state, the same run
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
            runs.append((losses, [p.detach().clone() for p in t.params]))
        losses, _ = _small_trainer("--fused_beta_latents --fused_beta_head --fused_blocks --dp 0.1 --no_final_eval").train()
        assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    finally:
        torch.backends.cudnn.deterministic = was
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    normal = tr.get_args("--nsa 20 --td 6 -b 3 --normal".split())
    normal.fused_beta_latents = True
    with pytest.raises(ValueError):
        tr.PVAETrainer(normal, _dev())
