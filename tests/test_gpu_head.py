"""The fused TruncatedNormal output head on the device (ct_pvae_amd/output_head.py, csrc/head.hip) against the float64 composition
of tests/np_twin_head.py fed the same uniforms, under that file's per-sample rule |got - ref| <= 4 R bar; the fixed order of the
per-object sum; the trainer with --fused_head."""
import math

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, forward_functions, head_uniforms, truncated_normal_head
from ct_pvae_amd import trainer as tr
from tests import np_twin_head as th

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
SHAPES = {"3x5x7": (3, 5, 7, 0), "2x64x64": (2, 64, 64, 0), "5x33x31+3": (5, 33, 31, 3), "1x128x128": (1, 128, 128, 0)}
_cases = {}


def _dev():
    return torch.device("cuda", 0)


def sum_chain(pix):
    """Longest chain of additions of LP[o] in the order csrc/head.hip states: quad, the thread's quads, butterfly, the 16 waves."""
    return 3 + math.ceil(math.ceil(pix / 4) / 1024) + 6 + 15


def run_head(alpha, beta, first_object, draw, g_x=None, g_LP=None, u=None, seed=SEED, X=1):
    """The device's (x, LP, lp_elem, g_alpha, g_beta) as numpy arrays [n][pix] / [n]; x and LP through the autograd function, lp_elem
    through the entry point (whose x and LP must be the function's, bit for bit)."""
    n, pix = alpha.shape
    dev = _dev()
    al = torch.from_numpy(alpha).to(dev).reshape(n, 1, X, pix // X).requires_grad_(True)
    be = torch.from_numpy(beta).to(dev).reshape(n, 1, X, pix // X).requires_grad_(True)
    ud = torch.from_numpy(u).to(dev).reshape(n, 1, X, pix // X) if u is not None else None
    x, LP = truncated_normal_head(al, be, seed=seed, draw=draw, first_object=first_object, _u=ud)
    assert x.shape == (n, X, pix // X, 1) and LP.shape == (n,) and x.dtype == LP.dtype == torch.float32
    x2 = forward_functions._new_output((n, pix), torch.float32, dev)
    LP2 = forward_functions._new_output((n,), torch.float32, dev)
    lp_elem = forward_functions._new_output((n, pix), torch.float32, dev)
    _lib.check(_lib.load().ctpvae_tn_head_fwd_f32(al.data_ptr(), be.data_ptr(), n, pix, first_object, seed, draw,
                                                  ud.data_ptr() if ud is not None else None, x2.data_ptr(), LP2.data_ptr(),
                                                  lp_elem.data_ptr(), forward_functions._stream_ptr()), "tn_head_fwd")
    assert torch.equal(x2, x.reshape(n, pix)) and torch.equal(LP2, LP)
    ga = gb = None
    if g_x is not None:
        loss = (x.reshape(n, pix) * torch.from_numpy(g_x).to(dev)).sum() + (LP * torch.from_numpy(g_LP).to(dev)).sum()
        ga, gb = (g.reshape(n, pix).cpu().numpy() for g in torch.autograd.grad(loss, (al, be)))
    return x.detach().reshape(n, pix).cpu().numpy(), LP.detach().cpu().numpy(), lp_elem.cpu().numpy(), ga, gb


def device_case(shape, kind):
    """One (shape, range): the CPU reference (computed once, shared, left unchanged) and the device's results."""
    key = (shape, kind)
    if key not in _cases:
        n, X, Y, fo = SHAPES[shape]
        c = th.case(kind, n, X * Y, SEED, first_object=fo, draw=5)
        c["dev"] = dict(zip(("x", "LP", "lp", "g_alpha", "g_beta"), run_head(c["alpha"], c["beta"], fo, 5, c["g_x"], c["g_LP"], X=X)))
        _cases[key] = c
    return _cases[key]


@pytest.mark.parametrize("kind", list(th.RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_sample_within_its_bar_of_float64(shape, kind):
    """x, lp, g_alpha, g_beta of the kernels' own Philox draws against the float64 composition fed the numpy Philox's u."""
    c = device_case(shape, kind)
    assert c["skip"].mean() <= 0.01
    for k in ("x", "lp", "g_alpha", "g_beta"):
        keep = ~c["skip"] if k.startswith("g_") else np.ones_like(c["skip"])
        e = th.excess(c["dev"][k], c["want"][k], c["bar"][k])
        worst = float(np.max(e[keep])) if keep.any() else 0.0
        print(f"{shape} {kind} {k}: worst |got - ref| / bar = {worst:.3f}, R = {c['R'][k]:.3f}, left out {int((~keep).sum())}")
        assert np.isfinite(c["dev"][k]).all(), k                        # (also: no element left at its NaN poison)
        assert worst <= th.MARGIN * c["R"][k], (k, worst, c["R"][k])


def test_injected_u_reaches_both_clamps_of_p():
    """u = 2^-25, 0.5, 1.0 (and 1 - 2^-24) with Pa ~ 2e-8 (a = -5.5): the first is clamped at 1e-7, the last two at 1 - 1e-7.
    Values obey the same bar; with g_LP = 0 and pr' = 1 (alpha >= 1) nothing but g_x reaches alpha where p is clamped, exactly.  A
    second set with Pa ~ 0.5 (a = -1e-3), where the path through p carries 7 % of g_x just below the upper clamp."""
    n, pix = 2, 64
    u = np.tile(np.array([2.0 ** -25, 0.5, 1.0, 1 - 2.0 ** -24], np.float32), (n, pix // 4))
    for av, bv, clamped in ((2.75, 1 + math.log(0.5), (0, 2, 3)), (1.0, 1000.0, (2, 3))):
        alpha, beta = np.full((n, pix), av, np.float32), np.full((n, pix), bv, np.float32)
        c = th.case(None, n, pix, 5, u=u, operands_=(alpha, beta), skip_p=False)
        ref = th._np(c["ref"])
        for col in range(4):
            is_clamped = bool((ref["p0"][0, col] < th.P_LO) or (ref["p0"][0, col] > th.P_HI))
            assert is_clamped == (col in clamped), (av, col, ref["p0"][0, col])
        x, LP, lp, ga, gb = run_head(alpha, beta, 0, 0, c["g_x"], c["g_LP"], u=u)
        got = dict(x=x, lp=lp, g_alpha=ga, g_beta=gb)
        for k in ("x", "lp", "g_alpha", "g_beta"):
            keep = ~c["skip"] if k.startswith("g_") else np.ones_like(c["skip"])
            worst = float(np.max(th.excess(got[k], c["want"][k], c["bar"][k])[keep]))
            print(f"injected a={-av / math.exp(bv - 1) if bv < 1 else -av / bv:.3g} {k}: worst {worst:.3f}, R = {c['R'][k]:.3f}, left out {int((~keep).sum())}")
            assert worst <= th.MARGIN * c["R"][k], (k, worst)
        gx1 = c["g_x"].copy()
        gx1[0, 2] = 1.0                                   # a unit cotangent in a column clamped at HI: its g_beta IS the device's z
        _, _, _, ga0, gb0 = run_head(alpha, beta, 0, 0, gx1, np.zeros(n, np.float32), u=u)
        cols = np.zeros((n, pix), bool)
        cols[:, [j for j in range(pix) if j % 4 in clamped]] = True
        cols &= ~c["skip"]
        assert cols.any() and np.array_equal(ga0[cols], gx1[cols])
        if bv >= 1:                                       # pr'(beta) = 1: g_scale = g_x z - ga a / scale with ga exactly 0, z one constant
            hi = np.zeros((n, pix), bool)
            hi[:, [j for j in range(pix) if j % 4 in (2, 3)]] = True
            hi &= ~c["skip"]
            z_dev = gb0[0, 2]
            assert abs(float(z_dev) - float(ref["z"][0, 2])) < 1e-4
            assert np.array_equal(gb0[hi], (gx1[hi] * z_dev).astype(np.float32))
        free = np.zeros((n, pix), bool)
        free[:, 1::4] = True
        if av == 1.0:                                     # (at a = -5.5 phi(a) ~ 1e-7: the path through p is below an ulp of g_x)
            assert not np.array_equal(ga0[free], c["g_x"][free])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_object_sum_follows_the_stated_order(shape):
    """LP[o] against the float64 sum of the kernel's own lp_elem: within gamma_n sum |lp_elem|, n the longest chain of additions."""
    c = device_case(shape, "trainer")
    lp = c["dev"]["lp"].astype(np.float64)
    n_add = sum_chain(lp.shape[1])
    gamma = n_add * th.U / (1 - n_add * th.U)
    err, bound = np.abs(c["dev"]["LP"] - lp.sum(axis=1)), gamma * np.abs(lp).sum(axis=1)
    print(f"{shape}: chain {n_add}, worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (err, bound)


def test_sum_and_sample_are_reproducible_and_split_invariant():
    """Bit-equal across two runs, and between one call on 5 objects and calls on 2 + 3 objects with first_object (33 x 31 = 1023
    pixels: the split's objects sit at another alignment in memory than the whole batch's)."""
    c = device_case("5x33x31+3", "wide")
    x, LP = c["dev"]["x"], c["dev"]["LP"]
    x2, LP2, _, _, _ = run_head(c["alpha"], c["beta"], 3, 5)
    assert np.array_equal(x.view(np.uint32), x2.view(np.uint32)) and np.array_equal(LP.view(np.uint32), LP2.view(np.uint32))
    xa, LPa, _, _, _ = run_head(c["alpha"][:2], c["beta"][:2], 3, 5)
    xb, LPb, _, _, _ = run_head(np.ascontiguousarray(c["alpha"][2:]), np.ascontiguousarray(c["beta"][2:]), 5, 5)
    assert np.array_equal(np.concatenate([xa, xb]).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(np.concatenate([LPa, LPb]).view(np.uint32), LP.view(np.uint32))
    # the device draws what the host entry point reports: another draw index gives other samples
    x3, _, _, _, _ = run_head(c["alpha"], c["beta"], 3, 6)
    assert not np.array_equal(x3, x)


def test_unused_outputs_and_strided_inputs():
    """Only LP used (g_x is None), only x used (g_LP is None): the missing cotangent is zero; a channel half of the decoder's output
    is refused until it is made contiguous."""
    c = device_case("3x5x7", "trainer")
    dev = _dev()
    al = torch.from_numpy(c["alpha"]).to(dev).reshape(3, 1, 5, 7).requires_grad_(True)
    be = torch.from_numpy(c["beta"]).to(dev).reshape(3, 1, 5, 7).requires_grad_(True)
    x, LP = truncated_normal_head(al, be, seed=SEED, draw=5)
    gl = torch.from_numpy(c["g_LP"]).to(dev)
    gx = torch.from_numpy(c["g_x"]).to(dev).reshape(3, 5, 7, 1)
    a1, b1 = torch.autograd.grad((LP * gl).sum(), (al, be), retain_graph=True)
    a2, b2 = torch.autograd.grad((x * gx).sum(), (al, be), retain_graph=True)
    a3, b3 = torch.autograd.grad((x * gx).sum() + (LP * gl).sum(), (al, be))
    for part1, part2, both in ((a1, a2, a3), (b1, b2, b3)):
        assert torch.isfinite(both).all()
        assert torch.allclose(part1 + part2, both, rtol=1e-5, atol=1e-6 * float(both.abs().max()))     # (the backward is linear in g)
    both = torch.randn(3, 2, 5, 7, device=dev)
    with pytest.raises(ValueError):
        truncated_normal_head(both[:, :1], both[:, 1:], seed=0, draw=0)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 --normal -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def _gauss_lp64(proj, m, x, pnm, eps):
    loc = proj * m
    scale = eps + torch.sqrt(loc / pnm + eps)
    z = (x - loc) / scale
    return -0.5 * z * z - (0.5 * math.log(2 * math.pi) + torch.log(scale))


def test_find_loss_with_the_fused_head_matches_the_unfused_path(monkeypatch):
    """find_loss_vae_unsup(fused_head=(seed, draw, first_object)) against the unfused path whose rsample is fed head_uniforms(...).
    Both heads are float32 evaluations of one function, each within 4 R bar of float64 per sample, so
      |loss difference|  <= 2 * 4 R * sum (|d loss / d x| bar_x + |d loss / d lp| bar_lp)  + the float32 sums' own rounding
      |grad difference|  <= the same per-sample bars of g_alpha / g_beta -- plus the change of the projector's cotangent g_x over
                            bar_x, |lp''| A bar_x carried back by A^T (A: the rotate-and-sum of these angles, all weights >= 0; lp'':
                            the second derivative of the Gaussian log-probability, from float64 autograd) -- pushed through the last
                            convolution's weight gradient with |input|."""
    t = _small_trainer()
    ns, B = 2, 3
    seed, draw, fo = 99, 4, 6
    ps, m, ie = t._batch()
    angles_i = torch.from_numpy(np.ascontiguousarray(t.angles.next().astype(np.int32)))
    X = t.x_size
    u = torch.from_numpy(head_uniforms(ns * B, X * X, seed=seed, draw=draw, first_object=fo)).to(t.dev).reshape(ns * B, 1, X, X)

    def rsample(self):
        p = (self.cdf_a + u * self.Z).clamp(1e-7, 1 - 1e-7)
        return (self.loc + self.scale * torch.special.ndtri(p)).clamp_min(0.0)

    kept = {}
    real_decode = t.dec.forward

    def decode(latents):
        alpha, beta = real_decode(latents)
        kept["alpha"], kept["beta"] = alpha, beta
        return alpha, beta
    monkeypatch.setattr(t.dec, "forward", decode)
    weight = t.dec.head.ab.weight

    def run(fused):
        torch.manual_seed(7)                                  # the latents' randn: the same in both runs
        for p in t.params:
            p.grad = None
        loss_vec, _, _, recon = tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, num_samples=ns,
                                                       theta=t.theta_host, angles_i=angles_i, pad=t.pad, fused_head=fused)
        loss = loss_vec.mean()
        ga, gb = torch.autograd.grad(loss, (kept["alpha"], kept["beta"]), retain_graph=True)
        loss.backward()
        return loss.detach().double().item(), weight.grad.detach().clone(), ga, gb, kept["alpha"].detach(), kept["beta"].detach(), recon.detach()

    with monkeypatch.context() as mp:
        mp.setattr(tr.TruncatedNormal, "rsample", rsample)
        loss_u, gw_u, ga_u, gb_u, alpha, beta, recon_u = run(None)
    loss_f, gw_f, ga_f, gb_f, alpha_f, beta_f, recon_f = run((seed, draw, fo))
    assert torch.equal(alpha, alpha_f) and torch.equal(beta, beta_f)          # the decoder saw the same latents
    assert recon_f.shape == recon_u.shape == (B, 1, X, X)

    # ---- the bars, from the float64 composition on the decoder's alpha / beta with the cotangents the loss hands the head
    n, pix = ns * B, X * X
    al, be = alpha.reshape(n, pix).cpu().numpy(), beta.reshape(n, pix).cpu().numpy()
    un = u.reshape(n, pix).cpu().numpy()
    ref = th.compose(al, be, un, torch.float64)
    G = np.full(n, -1.0 / ns)                                                  # d loss / d LP[o]: loss = ... - mean_s sum_b LP
    x64 = ref["x"].detach().to(t.dev)
    # d loss / d x through the projector's likelihood, and its second derivative, in float64 from the closed form
    sel = angles_i.to(t.dev).long()
    with torch.no_grad():
        from ct_pvae_amd import project_tf_fast
        A = lambda img: project_tf_fast(img.reshape(n, X, X, 1).float(), t.theta_host[angles_i.numpy()], pad=t.pad, dim=2,   # noqa: E731
                                        integrate_vae=True)[..., 0].double()
        proj = A(x64)
    mm = m.repeat(ns, 1)[:, sel].double()[..., None]
    meas = ps.repeat(ns, 1, 1)[:, sel].double()
    pj = proj.clone().requires_grad_(True)
    lp = _gauss_lp64(pj, mm, meas, float(t.pnm), float(t.sqrt_reg))
    d1, = torch.autograd.grad(lp.sum(), pj, create_graph=True)
    d2, = torch.autograd.grad(d1.sum(), pj)
    xg = ref["x"].detach().clone().to(t.dev).requires_grad_(True)
    projg = project_tf_fast(xg.reshape(n, X, X, 1).float(), t.theta_host[angles_i.numpy()], pad=t.pad, dim=2, integrate_vae=True)[..., 0]
    g_x, = torch.autograd.grad((projg.double() * (-d1.detach() / ns)).sum(), xg)       # d loss / d x, A^T applied by the projector
    g_x = g_x.reshape(n, pix).double().cpu().numpy()
    bar = th.bars(ref, g_x, G)
    twin = th.compose(al, be, un, torch.float32)
    want = dict(zip(("g_alpha", "g_beta"), th.gradients(ref, g_x, G)), x=ref["x"].detach().numpy(), lp=ref["lp"].detach().numpy())
    tw = dict(zip(("g_alpha", "g_beta"), th.gradients(twin, g_x, G)), x=twin["x"].detach().numpy(), lp=twin["lp"].detach().numpy())
    R = {k: th.twin_ratio(tw[k], want[k], bar[k]) for k in want}
    for k, v in R.items():
        assert v <= th.R_MAX, (k, v)

    # loss
    terms = np.abs(g_x) * bar["x"] * R["x"] + np.abs(G)[:, None] * bar["lp"] * R["lp"]
    n_terms = lp.numel() + n * pix
    sums = 2 * th.U * math.log2(n_terms) * (float(lp.detach().abs().sum()) / ns + float(np.abs(want["lp"]).sum()) / ns)
    tol_loss = 2 * th.MARGIN * float(terms.sum()) + sums
    print(f"loss fused {loss_f:.6f} unfused {loss_u:.6f} |diff| {abs(loss_f - loss_u):.3e} tol {tol_loss:.3e}")
    assert abs(loss_f - loss_u) <= tol_loss

    # gradient of the decoder's last layer
    with torch.no_grad():
        dproj = A(torch.from_numpy(bar["x"] * R["x"] * th.MARGIN).to(t.dev))           # A bar_x
    # ... and the float32 evaluation of d lp / d proj itself, on two slightly different ray-sums: np_twin_gauss's bar and rule
    from tests import np_twin_gauss as tg
    pn, mn, xn = proj.cpu().numpy().astype(np.float32), mm[..., 0].cpu().numpy().astype(np.float32), meas.cpu().numpy().astype(np.float32)
    bar_d = tg.bar_dlogp(pn, mn, xn, float(t.pnm), float(t.sqrt_reg))
    R_d = tg.twin_ratio(tg.twin_dlogp(pn, mn, xn, float(t.pnm), float(t.sqrt_reg)), tg.reference_dlogp(pn, mn, xn, float(t.pnm), float(t.sqrt_reg)),
                        bar_d)
    assert R_d <= tg.R_MAX
    wq = ((d2.abs() * dproj + torch.from_numpy(tg.MARGIN * R_d * bar_d).to(t.dev)) / ns).detach()
    xb = torch.zeros(n, pix, device=t.dev, dtype=torch.float64, requires_grad=True)
    pb = project_tf_fast(xb.reshape(n, X, X, 1).float(), t.theta_host[angles_i.numpy()], pad=t.pad, dim=2, integrate_vae=True)[..., 0]
    dg_x, = torch.autograd.grad((pb.double() * wq).sum(), xb)                          # A^T (|lp''| A bar_x): the change of g_x
    dg_x = dg_x.reshape(n, pix).cpu().numpy()
    ca, cb = th.gradients(ref, np.ones((n, pix)), np.zeros(n))                          # d x / d alpha, d x / d beta per pixel
    tol_a = 2 * (th.MARGIN * R["g_alpha"] * bar["g_alpha"] + np.abs(ca) * dg_x)
    tol_b = 2 * (th.MARGIN * R["g_beta"] * bar["g_beta"] + np.abs(cb) * dg_x)
    ea, eb = np.abs((ga_f - ga_u).reshape(n, pix).cpu().numpy()), np.abs((gb_f - gb_u).reshape(n, pix).cpu().numpy())
    skip = th.near_clamp(ref, bar)
    print(f"head gradients: worst |diff| / tol alpha {float((ea / tol_a)[~skip].max()):.3f} beta {float((eb / tol_b)[~skip].max()):.3f}, "
          f"left out {int(skip.sum())}")
    assert skip.mean() <= 0.01 and (ea <= tol_a)[~skip].all() and (eb <= tol_b)[~skip].all()
    # ... pushed through the last convolution: |d g_w| <= wgrad(|input|, tol).  The float32 rounding of that sum itself (n X Y terms
    # per weight, added blockwise by the library: 2 U log2(terms) of sum |terms|; a plain running sum would be U * terms) rides along
    # as a relative widening of |g|.
    tol_a[skip] = np.maximum(tol_a[skip], ea[skip])
    tol_b[skip] = np.maximum(tol_b[skip], eb[skip])
    tol_ab = torch.from_numpy(np.stack([tol_a, tol_b], axis=1).reshape(n, 2, X, X)).float().to(t.dev)
    g_ab = torch.cat([ga_u, gb_u], dim=1).abs()
    conv = t.dec.head.ab
    caught = {}
    h = conv.register_forward_hook(lambda mod, inp, out: caught.__setitem__("inp", inp[0].detach()))
    torch.manual_seed(7)
    tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, num_samples=ns, theta=t.theta_host,
                           angles_i=angles_i, pad=t.pad, fused_head=(seed, draw, fo))
    h.remove()
    inp = caught["inp"].abs()
    # the maxout picks one of the two convolutions per output pixel: an upper bound lets the tolerance reach both
    w_abs = torch.zeros_like(weight, requires_grad=True)
    out = torch.nn.functional.conv2d(inp, w_abs, stride=conv.stride, padding=conv.padding)
    assert out.shape[1] == 4                                   # [alpha, beta] of the first convolution, then of the second
    both = torch.cat([tol_ab + 2 * th.U * math.log2(n * pix) * g_ab] * 2, dim=1)
    tol_w, = torch.autograd.grad((out * both).sum(), w_abs)
    diff = (gw_f - gw_u).abs()
    print(f"last layer: worst |diff| / tol {float((diff / tol_w.clamp_min(1e-30)).max()):.3f}, max |g_w| {float(gw_u.abs().max()):.3e}, "
          f"max |diff| {float(diff.max()):.3e}")
    assert (diff <= tol_w).all()


def test_fused_head_training_run_is_finite_and_reproducible():
    """A few --fused_head steps at the small shape of tests/test_gpu_trainer.py: finite losses; two runs with equal seeds are
    bit-equal, losses and parameters (the head's uniforms are a function of (--head_seed, step, object); the latents' come from
    torch's seeded generator; --reproducible asks torch for deterministic convolution algorithms -- MIOpen's default weight
    gradients differ in their last bits from run to run, with or without the fused head)."""
    runs = []
    was = torch.backends.cudnn.deterministic            # (--reproducible switches it on for the process: put back for the tests that follow)
    try:
        for _ in range(2):
            t = _small_trainer("--fused_head --reproducible")
            assert torch.backends.cudnn.deterministic is True
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
            runs.append((losses, [p.detach().clone() for p in t.params]))
    finally:
        torch.backends.cudnn.deterministic = was
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    beta_head = tr.get_args("--nsa 20 --td 6 -b 3".split())
    beta_head.fused_head = True
    with pytest.raises(ValueError):
        tr.PVAETrainer(beta_head, _dev())
