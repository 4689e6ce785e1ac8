"""The fused Beta output head on the device (ct_pvae_amd/beta_head.py, csrc/beta_head.hip) against the twins of
tests/np_twin_beta.py: the draws against the numpy Philox, every value and gradient against the float64 composition evaluated AT THE
DEVICE'S ACCEPTED DRAWS under that file's per-sample rule |got - ref| <= 4 R bar, the clamp, the fixed order of the per-object sum,
reproducibility and split invariance, a NaN operand, the trainer with --fused_beta_head."""
import math

import numpy as np
import pytest
import torch
from scipy import special

from ct_pvae_amd import _lib, beta_head, forward_functions
from ct_pvae_amd import trainer as tr
from tests import np_twin_beta as tb
from tests import np_twin_hmc

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
SEED = 0x5EED0123456789
DRAW = 5
# (n, X, Y, first_object): pix = 1, 3, 5 -- ragged quads, objects not 16-byte aligned; 16 x 16; 4100 -- a thread with two quads;
# 128 x 128 with n = 2
SHAPES = {"1x1x1": (1, 1, 1, 0), "3x1x3+2": (3, 1, 3, 2), "3x1x5": (3, 1, 5, 0), "1x16x16": (1, 16, 16, 0), "3x41x100+7": (3, 41, 100, 7),
          "2x128x128": (2, 128, 128, 0)}
_cases = {}


def _dev():
    return torch.device("cuda", 0)


def run_head(alpha, beta, first_object, draw, g_x=None, g_LP=None, seed=SEED, X=1, sr=tb.EPS32):
    """The device's results as a dict of numpy arrays: x, lp [n][pix], LP [n], aux [n][pix][2][4], g_alpha, g_beta [n][pix] (when
    cotangents are given); x and LP through the autograd function, lp and aux through the entry point (whose x and LP must be the
    function's, bit for bit)."""
    n, pix = alpha.shape
    dev = _dev()
    al = torch.from_numpy(alpha).to(dev).reshape(n, 1, X, pix // X).requires_grad_(True)
    be = torch.from_numpy(beta).to(dev).reshape(n, 1, X, pix // X).requires_grad_(True)
    x, LP = beta_head(al, be, seed=seed, draw=draw, first_object=first_object, sqrt_reg=sr)
    assert x.shape == (n, X, pix // X, 1) and LP.shape == (n,) and x.dtype == LP.dtype == torch.float32
    x2 = forward_functions._new_output((n, pix), torch.float32, dev)
    LP2 = forward_functions._new_output((n,), torch.float32, dev)
    lp_elem = forward_functions._new_output((n, pix), torch.float32, dev)
    aux = forward_functions._new_output((n, pix, 2, 4), torch.float32, dev)
    _lib.check(_lib.load().ctpvae_beta_head_fwd_f32(al.data_ptr(), be.data_ptr(), n, pix, first_object, seed, draw, sr, x2.data_ptr(),
                                                    LP2.data_ptr(), lp_elem.data_ptr(), aux.data_ptr(), forward_functions._stream_ptr()),
               "beta_head_fwd")
    assert torch.equal(x2.view(torch.int32), x.reshape(n, pix).view(torch.int32)) or bool(torch.isnan(x2).any())
    out = dict(x=x.detach().reshape(n, pix).cpu().numpy(), LP=LP.detach().cpu().numpy(), lp=lp_elem.cpu().numpy(), aux=aux.cpu().numpy(),
               LP2=LP2.cpu().numpy(), x2=x2.cpu().numpy())
    if g_x is not None:
        loss = (x.reshape(n, pix) * torch.from_numpy(g_x).to(dev)).sum() + (LP * torch.from_numpy(g_LP).to(dev)).sum()
        out["g_alpha"], out["g_beta"] = (g.reshape(n, pix).cpu().numpy() for g in torch.autograd.grad(loss, (al, be)))
    return out


def device_case(shape, kind):
    """One (shape, range): the device's results, and the CPU reference at the device's accepted draws (computed once, shared, left
    unchanged)."""
    key = (shape, kind)
    if key not in _cases:
        n, X, Y, fo = SHAPES[shape]
        alpha, beta = tb.operands(kind, n, X * Y, 17)
        g_x, g_LP = tb.cotangents(n, X * Y, 18)
        dev = run_head(alpha, beta, fo, DRAW, g_x, g_LP, X=X)
        c = tb.case(kind, n, X * Y, 17, draws=(dev["aux"][..., 0], dev["aux"][..., 1]))
        assert np.array_equal(c["alpha"], alpha) and np.array_equal(c["g_x"], g_x)
        c["dev"], c["fo"] = dev, fo
        _cases[key] = c
    return _cases[key]


@pytest.mark.parametrize("kind", list(tb.RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_draws_are_the_numpy_philox_at_the_reported_attempt(shape, kind):
    """aux's ub equals the numpy Philox draw bit for bit at the attempt k the device reports; zn is the device's normcdfinvf of the
    numpy u24(word 0) -- another implementation of ndtri than scipy's, so it is held to 4 ulps of the float64 ndtri of that float32
    uniform (plus 4 U: ndtri's slope at 0.5) instead of to scipy's float32 bits.  k equals the float64 search on all but at most 1e-4
    of the gammas, and every disagreement is a draw whose float64 acceptance margin is inside its own bar."""
    c = device_case(shape, kind)
    n, X, Y, fo = SHAPES[shape]
    w = tb.words(n, X * Y, SEED, DRAW, fo)
    aux = c["dev"]["aux"]
    k = aux[..., 2].astype(np.int64)
    assert ((k >= 0) & (k < tb.ATTEMPTS)).all() and np.array_equal(k.astype(F), aux[..., 2])
    at = np.take_along_axis(w, k[..., None, None], axis=3)[:, :, :, 0]                     # [n][pix][2][4]
    assert np.array_equal(np_twin_hmc.u24(at[..., 2]).view(np.uint32), aux[..., 1].view(np.uint32))
    zn64 = special.ndtri(np_twin_hmc.u24(at[..., 0]).astype(D))
    assert (np.abs(aux[..., 0] - zn64) <= 4 * tb.U * (1 + np.abs(zn64))).all()
    s64 = tb.search(c["alpha"], c["beta"], w, D)
    dis = k != s64["k"]
    print(f"{shape} {kind}: k differs on {int(dis.sum())} of {dis.size} gammas; attempts used: {np.bincount(k.ravel()).tolist()}")
    assert dis.sum() <= max(1e-4 * dis.size, 0)
    first = np.minimum(k, s64["k"])[..., None]
    m = np.take_along_axis(s64["margin"], first, axis=-1)[..., 0]
    b = np.take_along_axis(s64["bar"], first, axis=-1)[..., 0]
    assert (np.abs(m[dis]) <= tb.MARGIN * b[dis]).all()
    # lg of the device against the float64 twin at these draws: the bar of x is built on it
    assert np.isfinite(aux[..., 3]).all()


@pytest.mark.parametrize("kind", list(tb.RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_sample_within_its_bar_of_float64(shape, kind):
    """x, lp, g_alpha, g_beta against the float64 composition evaluated at the device's accepted draws."""
    c = device_case(shape, kind)
    left_out = float(c["skip"].mean())
    print(f"{shape} {kind}: left out near the clamp {int(c['skip'].sum())} of {c['skip'].size}")
    assert left_out <= 0.01
    for k in ("x", "lp", "g_alpha", "g_beta"):
        keep = ~c["skip"] if k.startswith("g_") else np.ones_like(c["skip"])
        e = tb.excess(c["dev"][k], c["want"][k], c["bar"][k])
        worst = float(np.max(e[keep])) if keep.any() else 0.0
        print(f"{shape} {kind} {k}: worst |got - ref| / bar = {worst:.3f}, R = {c['R'][k]:.3f}")
        assert c["R"][k] <= tb.R_MAX
        assert np.isfinite(c["dev"][k]).all(), k                        # (also: no element left at its NaN poison)
        assert worst <= tb.MARGIN * c["R"][k], (k, worst, c["R"][k])


def test_clamp_saturated_samples_and_the_exact_gate():
    """Concentrations of 3e-7 against 1.5: x rounds to 0 in object 0 and to 1 in object 1.  lp then uses sr or 1 - sr (within its bar
    of the float64 twin, whose clamp is the definition's), and the gate is exact: a saturated pixel's gradients have the same BITS
    whatever g_x is (the path through x vanishes, x y = 0), and with G = 0 they are exactly 0.  Then sqrt_reg = 0.25 on the trainer
    range, where the clamp binds on ordinary samples: values and gradients obey the same bars (the twin's gate is the definition's;
    tests/test_beta_head_cpu.py shows that a gate left open misses them)."""
    n, pix = 2, 64
    alpha = np.stack([np.full(pix, -14.0, F), np.full(pix, 1.5, F)])
    beta = np.stack([np.full(pix, 1.5, F), np.full(pix, -14.0, F)])
    g_x, g_LP = tb.cotangents(n, pix, 3)
    d = run_head(alpha, beta, 0, 1, g_x, g_LP)
    assert (d["x"][0] == 0).mean() > 0.9 and (d["x"][1] == 1).mean() > 0.9
    sat = (d["x"] == 0) | (d["x"] == 1)
    c = tb.case(None, n, pix, 2, draws=(d["aux"][..., 0], d["aux"][..., 1]), operands_=(alpha, beta))
    assert np.array_equal(c["g_x"], g_x)
    for k in ("x", "lp", "g_alpha", "g_beta"):
        worst = float(np.max(tb.excess(d[k], c["want"][k], c["bar"][k])[~c["skip"]]))
        print(f"saturated {k}: worst {worst:.3f}, R = {c['R'][k]:.3f}")
        assert worst <= tb.MARGIN * c["R"][k], (k, worst)
    a32 = np.exp(F(-15.0)) + F(tb.EPS32)
    sr, hi = F(tb.EPS32), F(1) - F(tb.EPS32)
    want0 = (a32 - 1) * np.log(sr.astype(D)) + 0.5 * np.log(hi.astype(D)) - (special.gammaln(float(a32)) + special.gammaln(1.5) - special.gammaln(1.5 + float(a32)))
    assert np.allclose(d["lp"][0][d["x"][0] == 0], want0, rtol=1e-5) and np.allclose(d["lp"][1][d["x"][1] == 1], want0, rtol=1e-5)
    d0 = run_head(alpha, beta, 0, 1, np.zeros_like(g_x), g_LP)
    for k in ("g_alpha", "g_beta"):
        assert np.array_equal(d0[k][sat].view(np.uint32), d[k][sat].view(np.uint32)), k
    dz = run_head(alpha, beta, 0, 1, g_x, np.zeros_like(g_LP))
    assert (dz["g_alpha"][sat] == 0).all() and (dz["g_beta"][sat] == 0).all()
    # the clamp binding on ordinary samples
    n, pix, sr = 2, 1024, 0.25
    alpha, beta = tb.operands("trainer", n, pix, 5)
    g_x, g_LP = tb.cotangents(n, pix, 6)
    d = run_head(alpha, beta, 0, 2, g_x, g_LP, sr=sr)
    c = tb.case(None, n, pix, 5, draws=(d["aux"][..., 0], d["aux"][..., 1]), operands_=(alpha, beta), sr=sr)
    bound = ~c["ref"]["passes"]
    assert 0.2 < bound.mean() < 0.9 and c["skip"].mean() <= 0.01
    for k in ("x", "lp", "g_alpha", "g_beta"):
        keep = ~c["skip"] if k.startswith("g_") else np.ones_like(c["skip"])
        worst = float(np.max(tb.excess(d[k], c["want"][k], c["bar"][k])[keep]))
        print(f"sr = 0.25 {k}: worst {worst:.3f}, R = {c['R'][k]:.3f}, clamp binds on {float(bound.mean()):.2f}")
        assert worst <= tb.MARGIN * c["R"][k], (k, worst)
    # where it binds, G does not ride on the path through x: the run with both cotangents is the sum of the run with G alone (the
    # direct term) and the run with g_x alone (g_x x y dlg), within the rounding of the two float32 results
    d0 = run_head(alpha, beta, 0, 2, np.zeros_like(g_x), g_LP, sr=sr)
    only = np.where(bound, g_x, 0).astype(F)
    d1 = run_head(alpha, beta, 0, 2, only, np.zeros_like(g_LP), sr=sr)
    for k in ("g_alpha", "g_beta"):
        s = d0[k].astype(D) + d1[k].astype(D)
        assert (np.abs(d[k] - s)[bound] <= 4 * tb.U * (np.abs(d0[k]) + np.abs(d1[k]))[bound] + 1e-30).all(), k


def ordered_sum(lp):
    """csrc/beta_head.hip's order of additions applied to one object's lp_elem, in float32."""
    pix = lp.shape[0]
    quads = (pix + 3) // 4
    padded = np.zeros(4 * quads, F)
    padded[:pix] = lp
    q = padded.reshape(quads, 4)
    s = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    rounds = (quads + 1023) // 1024
    sq = np.zeros(rounds * 1024, F)
    sq[:quads] = s
    acc = np.zeros(1024, F)
    for r in range(rounds):
        has = np.arange(1024) + 1024 * r < quads
        acc = np.where(has, acc + sq[1024 * r:1024 * (r + 1)], acc).astype(F)
    v = acc.reshape(16, 64)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ m]).astype(F)
    total = v[0, 0]
    for w in range(1, 16):
        total = F(total + v[w, 0])
    return total


@pytest.mark.parametrize("shape", list(SHAPES))
def test_object_sum_is_the_stated_order_bit_for_bit(shape):
    c = device_case(shape, "mixed")
    want = np.array([ordered_sum(row) for row in c["dev"]["lp"]], F)
    assert np.array_equal(want.view(np.uint32), c["dev"]["LP"].view(np.uint32)), (want, c["dev"]["LP"])
    assert np.array_equal(c["dev"]["LP2"].view(np.uint32), c["dev"]["LP"].view(np.uint32))


def test_sum_and_sample_are_reproducible_and_split_invariant():
    """Bit-equal across two runs, and between one call on 3 objects and calls on 1 + 2 objects with first_object (4100 pixels: the
    split's objects sit at the same alignment; 3 x 5: at another)."""
    for shape in ("3x41x100+7", "3x1x5"):
        c = device_case(shape, "mixed")
        fo = c["fo"]
        x, LP = c["dev"]["x"], c["dev"]["LP"]
        again = run_head(c["alpha"], c["beta"], fo, DRAW)
        assert np.array_equal(x.view(np.uint32), again["x"].view(np.uint32)) and np.array_equal(LP.view(np.uint32), again["LP"].view(np.uint32))
        a = run_head(c["alpha"][:1], c["beta"][:1], fo, DRAW)
        b = run_head(np.ascontiguousarray(c["alpha"][1:]), np.ascontiguousarray(c["beta"][1:]), fo + 1, DRAW)
        assert np.array_equal(np.concatenate([a["x"], b["x"]]).view(np.uint32), x.view(np.uint32))
        assert np.array_equal(np.concatenate([a["LP"], b["LP"]]).view(np.uint32), LP.view(np.uint32))
        other = run_head(c["alpha"], c["beta"], fo, DRAW + 1)
        assert not np.array_equal(other["x"], x)
        # the backward redraws what the forward drew: equal bits from two backward runs
        g1 = run_head(c["alpha"], c["beta"], fo, DRAW, c["g_x"], c["g_LP"])
        assert np.array_equal(g1["g_alpha"].view(np.uint32), c["dev"]["g_alpha"].view(np.uint32))
        assert np.array_equal(g1["g_beta"].view(np.uint32), c["dev"]["g_beta"].view(np.uint32))


def test_one_nan_operand_stays_in_its_object():
    """One NaN alpha: that pixel's x and its object's LP are NaN, every other pixel's x and every other object's LP keep their bits,
    the gradients of that pixel are NaN and all others keep theirs; the call returns (the attempt loop leaves after 16 refusals)."""
    c = device_case("3x1x5", "mixed")
    alpha = c["alpha"].copy()
    alpha[1, 2] = np.nan
    d = run_head(alpha, c["beta"], c["fo"], DRAW, c["g_x"], c["g_LP"])
    hit = np.zeros(alpha.shape, bool)
    hit[1, 2] = True
    assert np.isnan(d["x"][hit]).all() and np.isnan(d["LP"][1]) and int(d["aux"][1, 2, 0, 2]) == tb.ATTEMPTS - 1
    assert np.array_equal(d["x"][~hit].view(np.uint32), c["dev"]["x"][~hit].view(np.uint32))
    assert np.array_equal(d["LP"][[0, 2]].view(np.uint32), c["dev"]["LP"][[0, 2]].view(np.uint32))
    assert np.isnan(d["g_alpha"][hit]).all() and np.isnan(d["g_beta"][hit]).all()
    for k in ("g_alpha", "g_beta"):
        assert np.array_equal(d[k][~hit].view(np.uint32), c["dev"][k][~hit].view(np.uint32))


def test_iteration_bound_of_the_implicit_gradient():
    """kDlgMaxTerms = 2048 iterations serve every concentration up to 4e4: at c = 3e4 (about 1650 terms) values and gradients obey
    their bars.  At c = 2e5 the series would need about 4200: the kernel stops at its bound and returns NaN for THAT gamma's gradient,
    not a truncated sum (a draw above c + 1 takes the continued fraction and stays right); x, lp and the other operand's gradient stay
    finite and inside their bars."""
    n, pix = 1, 8
    alpha = np.array([[3e4] * 4 + [2e5] * 4], F)
    beta = np.full((n, pix), 2.0, F)
    g_x, g_LP = tb.cotangents(n, pix, 8)
    d = run_head(alpha, beta, 0, 3, g_x, g_LP)
    c = tb.case(None, n, pix, 7, draws=(d["aux"][..., 0], d["aux"][..., 1]), operands_=(alpha, beta))
    assert np.array_equal(c["g_x"], g_x) and not c["skip"].any()
    ok = np.arange(pix) < 4
    for k in ("x", "lp", "g_alpha", "g_beta"):
        cols = ok if k == "g_alpha" else np.ones(pix, bool)
        worst = float(np.max(tb.excess(d[k], c["want"][k], c["bar"][k])[:, cols]))
        print(f"c = 3e4 / 2e5 {k}: worst {worst:.3f}, R = {c['R'][k]:.3f}")
        assert worst <= tb.MARGIN * c["R"][k], (k, worst)
    # c = 2e5: a draw below c + 1 takes the series (NaN at the bound); one above takes the continued fraction, which converges in a
    # few dozen iterations at any c and must then be right
    far = d["g_alpha"][:, ~ok]
    e = tb.excess(far, c["want"]["g_alpha"][:, ~ok], c["bar"]["g_alpha"][:, ~ok])
    series = np.exp(c["ref"]["lg"][:, ~ok, 0]) <= c["ref"]["a"][:, ~ok] + 1
    assert series.any() and np.isnan(far[series]).all() and np.isfinite(c["want"]["g_alpha"]).all()
    assert (e[~series] <= tb.MARGIN * c["R"]["g_alpha"]).all()


def test_unused_outputs_and_strided_inputs():
    """Only LP used (g_x is None), only x used (g_LP is None): the missing cotangent is zero; a channel half of the decoder's output
    is refused until it is made contiguous."""
    c = device_case("1x16x16", "trainer")
    dev = _dev()
    al = torch.from_numpy(c["alpha"]).to(dev).reshape(1, 1, 16, 16).requires_grad_(True)
    be = torch.from_numpy(c["beta"]).to(dev).reshape(1, 1, 16, 16).requires_grad_(True)
    x, LP = beta_head(al, be, seed=SEED, draw=DRAW)
    gl = torch.from_numpy(c["g_LP"]).to(dev)
    gx = torch.from_numpy(c["g_x"]).to(dev).reshape(1, 16, 16, 1)
    a1, b1 = torch.autograd.grad((LP * gl).sum(), (al, be), retain_graph=True)
    a2, b2 = torch.autograd.grad((x * gx).sum(), (al, be), retain_graph=True)
    a3, b3 = torch.autograd.grad((x * gx).sum() + (LP * gl).sum(), (al, be))
    assert np.array_equal(a3.reshape(1, 256).cpu().numpy().view(np.uint32), c["dev"]["g_alpha"].view(np.uint32))
    # the backward is linear in (g_x, G) up to the gate's term G K, which rides on g_x's path: compare through the twin's bars
    for part1, part2, both, k in ((a1, a2, a3, "g_alpha"), (b1, b2, b3, "g_beta")):
        assert torch.isfinite(both).all()
        err = (part1 + part2 - both).abs().reshape(1, 256).cpu().numpy()
        assert (err <= 2 * tb.MARGIN * c["bar"][k] + 4 * tb.U * np.abs(c["want"][k]))[~c["skip"]].all(), k
    both = torch.randn(3, 2, 5, 7, device=dev)
    with pytest.raises(ValueError):
        beta_head(both[:, :1], both[:, 1:], seed=0, draw=0)
    x, LP = beta_head(both[:, :1].contiguous(), both[:, 1:].contiguous(), seed=0, draw=0)
    assert torch.isfinite(x).all() and torch.isfinite(LP).all()


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def _gauss_lp64(proj, m, x, pnm, eps):
    loc = proj * m
    scale = eps + torch.sqrt(loc / pnm + eps)
    z = (x - loc) / scale
    return -0.5 * z * z - (0.5 * math.log(2 * math.pi) + torch.log(scale))


class _TwinSample(torch.autograd.Function):
    """x of the float64 twin at given draws, as a float32 tensor; the implicit gradient."""
    @staticmethod
    def forward(ctx, a, b, twin):
        ctx.twin = twin
        return torch.from_numpy(twin["x"].astype(F)).to(a.device).reshape(a.shape)

    @staticmethod
    def backward(ctx, g):
        t = ctx.twin
        xy = t["x"] * t["y"]
        d0, d1 = tb.dlg(t["a"], t["lg"][..., 0]), tb.dlg(t["b"], t["lg"][..., 1])
        gn = g.detach().double().cpu().numpy().reshape(xy.shape)
        with np.errstate(all="ignore"):
            ga = np.where((gn == 0) | (xy == 0), 0.0, gn * xy * d0)
            gb = np.where((gn == 0) | (xy == 0), 0.0, -gn * xy * d1)
        return torch.from_numpy(ga).to(g.device).reshape(g.shape), torch.from_numpy(gb).to(g.device).reshape(g.shape), None


class _TwinLogProb(torch.autograd.Function):
    """lp of the float64 twin (its clamp, its y); gradients to a, b and, through the gate, to x."""
    @staticmethod
    def forward(ctx, a, b, x, twin):
        ctx.twin = twin
        return torch.from_numpy(twin["lp"]).to(a.device).reshape(a.shape)

    @staticmethod
    def backward(ctx, g):
        t = ctx.twin
        gn = g.detach().double().cpu().numpy().reshape(t["x"].shape)
        pab = special.digamma(t["a"] + t["b"])
        ga = gn * (np.log(t["xc"]) - special.digamma(t["a"]) + pab)
        gb = gn * (np.log(t["yc"]) - special.digamma(t["b"]) + pab)
        gx = np.where(t["passes"], gn * ((t["a"] - 1) / t["xc"] - (t["b"] - 1) / t["yc"]), 0.0)
        back = lambda v: torch.from_numpy(v).to(g.device).reshape(g.shape)               # noqa: E731
        return back(ga), back(gb), back(gx), None


def test_find_loss_with_the_fused_beta_head_matches_the_twin_fed_unfused_path(monkeypatch):
    """find_loss_vae_unsup(fused_beta_head=(seed, draw, first_object), deterministic=True) against the UNFUSED branch of the same call
    whose torch.distributions.Beta is replaced by the float64 twin of tests/np_twin_beta.py fed the device's own accepted draws
    (aux_out of the entry point): its rsample is the twin's x with the implicit gradient, its log_prob the twin's clamped lp.  Matching
    torch's own Beta.rsample is impossible: it takes its gammas from torch's global generator (other draws) and differentiates with
    another estimator (_dirichlet_grad, not the implicit gradient of each gamma); both facts are pinned on the CPU.
      |loss difference|  <= 4 R * sum (|d loss / d x| bar_x + |d loss / d lp| bar_lp)  + the float32 sums' own rounding
      |grad difference|  <= the per-sample bars of g_alpha / g_beta -- plus the change of the projector's cotangent g_x over bar_x,
                            |lp''| A bar_x carried back by A^T (A: the rotate-and-sum of these angles; lp'': the second derivative of
                            the Gaussian log-probability, float64 autograd) -- pushed through the last convolution's weight gradient."""
    t = _small_trainer("--det")
    B = 3
    seed, draw, fo = 99, 4, 6
    ps, m, ie = t._batch()
    angles_i = torch.from_numpy(np.ascontiguousarray(t.angles.next().astype(np.int32)))
    X = t.x_size
    n, pix = B, X * X
    kept = {}
    real_decode = t.dec.forward

    def decode(latents):
        alpha, beta = real_decode(latents)
        kept["alpha"], kept["beta"] = alpha, beta
        return alpha, beta
    monkeypatch.setattr(t.dec, "forward", decode)
    weight = t.dec.head.ab.weight

    def run(fused):
        for p in t.params:
            p.grad = None
        loss_vec, _, _, recon = tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, num_samples=2,
                                                       theta=t.theta_host, angles_i=angles_i, pad=t.pad, deterministic=True,
                                                       use_normal=False, fused_beta_head=fused)
        loss = loss_vec.mean()
        assert torch.isfinite(loss)
        ga, gb = torch.autograd.grad(loss, (kept["alpha"], kept["beta"]), retain_graph=True)
        loss.backward()
        return loss.detach().double().item(), weight.grad.detach().clone(), ga, gb, kept["alpha"].detach(), kept["beta"].detach(), recon.detach()

    loss_f, gw_f, ga_f, gb_f, alpha, beta, recon_f = run((seed, draw, fo))
    al, be = alpha.reshape(n, pix).cpu().numpy(), beta.reshape(n, pix).cpu().numpy()
    d = run_head(al, be, fo, draw, seed=seed, X=X, sr=float(t.sqrt_reg))
    assert np.array_equal(d["x"].view(np.uint32), recon_f.reshape(n, pix).cpu().numpy().view(np.uint32))
    ref = tb.compose(al, be, (d["aux"][..., 0], d["aux"][..., 1]), D, sr=float(t.sqrt_reg))

    class TwinBeta:
        def __init__(self, a, b):
            self.a, self.b = a.double(), b.double()           # (one float64 copy: the two paths into a add up before the cast back)

        def rsample(self):
            self.x = _TwinSample.apply(self.a, self.b, ref)
            return self.x

        def log_prob(self, xc):
            return _TwinLogProb.apply(self.a, self.b, self.x, ref)

    with monkeypatch.context() as mp:
        mp.setattr(torch.distributions, "Beta", TwinBeta)
        loss_u, gw_u, ga_u, gb_u, alpha_u, beta_u, recon_u = run(None)
    assert torch.equal(alpha, alpha_u) and torch.equal(beta, beta_u)            # deterministic latents: the decoder saw the same input
    assert recon_f.shape == recon_u.shape == (B, 1, X, X)

    # ---- the bars, from the float64 composition with the cotangents the loss hands the head
    G = np.full(n, -1.0)                                                         # d loss / d LP[o]: loss = ... - sum_b LP  (ns = 1)
    x64 = torch.from_numpy(ref["x"]).to(t.dev)
    sel = angles_i.to(t.dev).long()
    from ct_pvae_amd import project_tf_fast
    th_sel = t.theta_host[angles_i.numpy()]
    A = lambda img: project_tf_fast(img.reshape(n, X, X, 1).float(), th_sel, pad=t.pad, dim=2, integrate_vae=True)[..., 0].double()   # noqa: E731
    with torch.no_grad():
        proj = A(x64)
    mm = m[:, sel].double()[..., None]
    meas = ps[:, sel].double()
    pj = proj.clone().requires_grad_(True)
    lp = _gauss_lp64(pj, mm, meas, float(t.pnm), float(t.sqrt_reg))
    d1, = torch.autograd.grad(lp.sum(), pj, create_graph=True)
    d2, = torch.autograd.grad(d1.sum(), pj)
    xg = x64.clone().requires_grad_(True)
    projg = project_tf_fast(xg.reshape(n, X, X, 1).float(), th_sel, pad=t.pad, dim=2, integrate_vae=True)[..., 0]
    g_x, = torch.autograd.grad((projg.double() * (-d1.detach())).sum(), xg)              # d loss / d x, A^T applied by the projector
    g_x = g_x.reshape(n, pix).double().cpu().numpy()
    bar = tb.bars(ref, g_x, G)
    twin = tb.compose(al, be, (d["aux"][..., 0], d["aux"][..., 1]), F, sr=float(t.sqrt_reg))
    want = dict(zip(("g_alpha", "g_beta"), tb.gradients(ref, g_x, G)), x=ref["x"], lp=ref["lp"])
    tw = dict(zip(("g_alpha", "g_beta"), tb.gradients(twin, g_x, G)), x=twin["x"], lp=twin["lp"])
    skip = tb.near_clamp(ref, bar)
    R = {k: tb.twin_ratio(tw[k][~skip] if k.startswith("g_") else tw[k], want[k][~skip] if k.startswith("g_") else want[k],
                          bar[k][~skip] if k.startswith("g_") else bar[k]) for k in want}
    for k, v in R.items():
        assert v <= tb.R_MAX, (k, v)

    # loss
    terms = np.abs(g_x) * bar["x"] * R["x"] + np.abs(G)[:, None] * bar["lp"] * R["lp"]
    n_terms = lp.numel() + n * pix
    sums = 2 * tb.U * math.log2(n_terms) * (float(lp.detach().abs().sum()) + float(np.abs(want["lp"]).sum()))
    tol_loss = 2 * tb.MARGIN * float(terms.sum()) + sums
    print(f"loss fused {loss_f:.6f} twin-fed unfused {loss_u:.6f} |diff| {abs(loss_f - loss_u):.3e} tol {tol_loss:.3e}")
    assert abs(loss_f - loss_u) <= tol_loss

    # gradients of alpha / beta
    with torch.no_grad():
        dproj = A(torch.from_numpy(bar["x"] * R["x"] * tb.MARGIN).to(t.dev))             # A bar_x
    from tests import np_twin_gauss as tg
    pn, mn, xn = proj.cpu().numpy().astype(F), mm[..., 0].cpu().numpy().astype(F), meas.cpu().numpy().astype(F)
    bar_d = tg.bar_dlogp(pn, mn, xn, float(t.pnm), float(t.sqrt_reg))
    R_d = tg.twin_ratio(tg.twin_dlogp(pn, mn, xn, float(t.pnm), float(t.sqrt_reg)), tg.reference_dlogp(pn, mn, xn, float(t.pnm), float(t.sqrt_reg)),
                        bar_d)
    assert R_d <= tg.R_MAX
    wq = (d2.abs() * dproj + torch.from_numpy(tg.MARGIN * R_d * bar_d).to(t.dev)).detach()
    xb = torch.zeros(n, pix, device=t.dev, dtype=torch.float64, requires_grad=True)
    pb = project_tf_fast(xb.reshape(n, X, X, 1).float(), th_sel, pad=t.pad, dim=2, integrate_vae=True)[..., 0]
    dg_x, = torch.autograd.grad((pb.double() * wq).sum(), xb)                            # A^T (|lp''| A bar_x): the change of g_x
    dg_x = dg_x.reshape(n, pix).cpu().numpy()
    ca, cb = tb.gradients(ref, np.ones((n, pix), F), np.zeros(n, F))                     # d x / d alpha, d x / d beta per pixel
    tol_a = 2 * (tb.MARGIN * R["g_alpha"] * bar["g_alpha"] + np.abs(ca) * dg_x)
    tol_b = 2 * (tb.MARGIN * R["g_beta"] * bar["g_beta"] + np.abs(cb) * dg_x)
    ea, eb = np.abs((ga_f - ga_u).reshape(n, pix).cpu().numpy()), np.abs((gb_f - gb_u).reshape(n, pix).cpu().numpy())
    print(f"head gradients: worst |diff| / tol alpha {float((ea / tol_a)[~skip].max()):.3f} beta {float((eb / tol_b)[~skip].max()):.3f}, "
          f"left out {int(skip.sum())}")
    assert skip.mean() <= 0.01 and (ea <= tol_a)[~skip].all() and (eb <= tol_b)[~skip].all()
    # ... pushed through the last convolution: |d g_w| <= wgrad(|input|, tol), with the float32 rounding of that sum riding along
    tol_a[skip] = np.maximum(tol_a[skip], ea[skip])
    tol_b[skip] = np.maximum(tol_b[skip], eb[skip])
    tol_ab = torch.from_numpy(np.stack([tol_a, tol_b], axis=1).reshape(n, 2, X, X)).float().to(t.dev)
    g_ab = torch.cat([ga_u, gb_u], dim=1).abs().float()
    conv = t.dec.head.ab
    caught = {}
    h = conv.register_forward_hook(lambda mod, inp, out: caught.__setitem__("inp", inp[0].detach()))
    tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, num_samples=2, theta=t.theta_host,
                           angles_i=angles_i, pad=t.pad, deterministic=True, use_normal=False, fused_beta_head=(seed, draw, fo))
    h.remove()
    inp = caught["inp"].abs()
    w_abs = torch.zeros_like(weight, requires_grad=True)
    out = torch.nn.functional.conv2d(inp, w_abs, stride=conv.stride, padding=conv.padding)
    assert out.shape[1] == 4                                   # [alpha, beta] of the first convolution, then of the second
    both = torch.cat([tol_ab + 2 * tb.U * math.log2(n * pix) * g_ab] * 2, dim=1)
    tol_w, = torch.autograd.grad((out * both).sum(), w_abs)
    diff = (gw_f - gw_u).abs()
    print(f"last layer: worst |diff| / tol {float((diff / tol_w.clamp_min(1e-30)).max()):.3f}, max |g_w| {float(gw_u.abs().max()):.3e}, "
          f"max |diff| {float(diff.max()):.3e}")
    assert (diff <= tol_w).all()


def test_fused_beta_head_training_run_is_finite_and_reproducible():
    """A few --fused_beta_head steps without --normal (Beta latents from torch's seeded generator, the Beta head from the kernels):
    finite losses; two runs with equal seeds are bit-equal, losses and parameters; the run reaches its final evaluation."""
    runs = []
    was = torch.backends.cudnn.deterministic            # (--reproducible switches it on for the process: put back for the tests that follow)
    try:
        for _ in range(2):
            t = _small_trainer("--fused_beta_head --reproducible")
            assert torch.backends.cudnn.deterministic is True
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
            runs.append((losses, [p.detach().clone() for p in t.params]))
        loss_final, _ = t.final_evaluation(None)
        assert np.isfinite(np.asarray(loss_final)).all()
    finally:
        torch.backends.cudnn.deterministic = was
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    normal = tr.get_args("--nsa 20 --td 6 -b 3 --normal".split())
    normal.fused_beta_head = True
    with pytest.raises(ValueError):
        tr.PVAETrainer(normal, _dev())
