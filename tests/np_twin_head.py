"""Twins of the TruncatedNormal output head (ct_pvae_amd/csrc/head.hip; the trainer's positive_range / TruncatedNormal.rsample /
.log_prob) and the per-sample acceptance rule the tests hold the kernels to.

    compose(alpha, beta, u, dtype)     the trainer's composition, operation by operation, in torch on the CPU with the uniforms
                                       injected; float64: the definition (its autograd IS the gradient's definition), on the float32
                                       operands promoted to float64, with the float32 constants (eps, the clamp bounds 1e-7f and
                                       (float)(1 - 1e-7)) promoted too; float32: the "float32 twin"
    gradients(c, g_x, g_LP)            autograd of sum(x g_x) + sum_o g_LP[o] sum_pixels lp
    uniforms(n, pix, seed, draw, fo)   the kernels' u from a numpy Philox (np_twin_hmc.philox)
    bars(ref, g_x, g_LP)               a first-order float32 error bar per sample for x, lp, g_alpha, g_beta, U = 2^-24, every term in
                                       float64 from the float64 composition's intermediates

The bar follows the roundings of the named intermediates through the composition:
    loc, scale   relative U (2 + |t - 1|) below t = 1 (the rounding of t - 1 moves exp by that much), 2 U above
    a            |a| (rel loc + rel scale + 2 U)
    Pa           phi(a) da + 2 U ABSOLUTE (0.5 (1 + erf) rounds next to -1);   Z = 1 - Pa:  dPa + U Z
    p            dPa + u dZ + 2 U p;  0 where the clamp binds (the bound is a constant)
    z            D dp + 2 U |z| + U,  D = ndtri'(p) = sqrt(2 pi) e^(z^2 / 2) -- THE term: next to p = 1 it is 1e6 U
    x            dloc + |z| dscale + scale dz + U (|scale z| + |x|)
    zeta         dz + U (|x| + |loc|) / scale + 3 U |zeta|  (x - loc cancels loc's own error, not the rounding of the sum x)
    lp           |zeta| dzeta + U zeta^2 + rel scale + U |log scale| + dZ / Z + U |log Z| + 2 U |lp| + U
and, for the gradients (G = g_LP of the pixel's object, rs = 1 / scale, gzs = G zeta rs; [x], [p]: the clamps pass):
    gx0 = [x] (g_x - gzs)                  [x] (|G| rs dzeta + |gzs| (rel scale + 2 U) + U (|g_x| + |gzs|))
    gp  = [p] gx0 scale D                  [p] (scale D dgx0 + |gp| (rel scale + |z| dz + U (4 + z^2 / 2)))
    br  = gp (1 - u) + G / Z               dgp (1 - u) + 2 U |gp| + |G| dZ / Z^2 + 2 U |G / Z|
    ga  = phi(a) br                        phi (|a| da + U (2 + a^2)) |br| + phi dbr + 2 U |ga|
    gloc   = (gx0 + gzs) - ga rs           U (|g_x| + 4 |gzs|) + dga rs + |ga rs| (rel scale + 2 U) + 2 U |gloc|
                                           (gzs leaves and re-enters as the same float: it cancels, its rounding does not)
    gscale = gx0 z + G (zeta^2 - 1) rs - ga a rs
                                           |g_x| dz + U |g_x z| + |gzs| (dzeta - dz) + 4 U (|gzs z| + |G| zeta^2 rs)
                                           + |G rs| (rel scale + 2 U) + |a| rs dga + |ga| rs da + |ga a rs| (rel scale + 3 U) + 2 U |gscale|
    g_alpha = pr'(alpha) gloc              pr' dgloc + |g_alpha| (rel loc + U);  g_beta alike

The rule (device): for EVERY sample |got - ref| <= MARGIN * R * bar, R = max(1, the float32 twin's own worst excess on the same
operands) and MARGIN = 4, np_twin_gauss's values; R <= R_MAX is asserted on the CPU (tests/test_head_cpu.py).  Samples whose float64
p (before its clamp) or x (before its clamp) lies within its bar of a clamp bound may be left out of the GRADIENT comparison
(near_clamp): the derivative jumps there."""
import math

import numpy as np
import torch

from tests import np_twin_gauss as tg
from tests import np_twin_hmc

TAG = 0x544E48
U = 2.0 ** -24
MARGIN, R_MAX = tg.MARGIN, tg.R_MAX
EPS32 = float(np.finfo(np.float32).eps)
P_LO, P_HI = float(np.float32(1e-7)), float(np.float32(1 - 1e-7))
RANGES = {"trainer": ((-1.0, 2.0), (-3.0, 0.5)), "trunc": ((-6.0, 0.2), (-0.5, 1.7)), "wide": ((-3.0, 2.5), (-4.0, 1.5))}
excess, twin_ratio = tg.excess, tg.twin_ratio


def uniforms(n, pix, seed, draw, first_object=0):
    """float32 [n][pix]: word e & 3 of Philox((lo32(e >> 2), hi32(e >> 2), draw, TAG), seed), e = (first_object + o) * pix + pixel."""
    e = np.array([[(int(first_object) + o) * int(pix) + k for k in range(pix)] for o in range(n)], dtype=np.uint64)
    blk = e >> np.uint64(2)
    w = np_twin_hmc.philox(blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), np.uint64(draw), TAG, int(seed))       # [n][pix][4]
    word = np.take_along_axis(w, (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    return np_twin_hmc.u24(word)


def operands(kind, n, pix, seed):
    """float32 (alpha, beta) [n][pix], uniform on the raw-input range `kind`."""
    (a0, a1), (b0, b1) = RANGES[kind]
    rng = np.random.default_rng(seed)
    return rng.uniform(a0, a1, (n, pix)).astype(np.float32), rng.uniform(b0, b1, (n, pix)).astype(np.float32)


def cotangents(n, pix, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, pix)).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def _positive_range(t, unit_slope):
    x = t - 1
    neg = (x < 0).to(t.dtype)
    v = (torch.exp(torch.clamp(x, -1e10, 10)) + EPS32) * neg + (x + 1) * (1 - neg)
    return t + (v - t).detach() if unit_slope else v      # (defect: the value of pr, the slope 1 everywhere)


def compose(alpha, beta, u, dtype, defect=None):
    """The composition on float32 operands [n][pix] in `dtype`; returns a dict of torch tensors (alpha, beta are leaves that require
    grad).  defect (negative controls): "no_log_z" drops log Z from lp, "unit_slope" makes pr' = 1; the law tests' "z_is_1"
    takes Z as 1 in p = Pa + u Z, "no_truncation" forgets the truncation in the draw altogether (p = u), "flip_lower" takes 1 - u for
    u where p falls on the lower half."""
    assert defect in (None, "no_log_z", "unit_slope", "z_is_1", "no_truncation", "flip_lower")
    al = torch.tensor(np.asarray(alpha, np.float32)).to(dtype).requires_grad_(True)
    be = torch.tensor(np.asarray(beta, np.float32)).to(dtype).requires_grad_(True)
    uu = torch.tensor(np.asarray(u, np.float32)).to(dtype)
    loc, scale = _positive_range(al, defect == "unit_slope"), _positive_range(be, defect == "unit_slope")
    a = (0.0 - loc) / scale
    Pa = 0.5 * (1 + torch.erf(a / math.sqrt(2.0)))
    cdf_b = 0.5 * (1 + torch.erf(((1e10 - loc) / scale) / math.sqrt(2.0)))
    Z = (cdf_b - Pa).clamp_min(1e-30)
    p0 = uu if defect == "no_truncation" else Pa + uu * (1.0 if defect == "z_is_1" else Z)
    if defect == "flip_lower":
        p0 = torch.where(p0 < 0.5, Pa + (1 - uu) * Z, p0)
    p = p0.clamp(P_LO, P_HI)
    z = torch.special.ndtri(p)
    x0 = loc + scale * z
    x = x0.clamp_min(0.0)
    zeta = (x - loc) / scale
    lp = -0.5 * zeta * zeta - 0.5 * math.log(2 * math.pi) - torch.log(scale)
    if defect != "no_log_z":
        lp = lp - torch.log(Z)
    return dict(alpha=al, beta=be, u=uu, loc=loc, scale=scale, a=a, Pa=Pa, Z=Z, p0=p0, p=p, z=z, x0=x0, x=x, zeta=zeta, lp=lp)


def gradients(c, g_x, g_LP):
    """(g_alpha, g_beta) as numpy arrays of the composition's dtype."""
    dt = c["x"].dtype
    gx, gl = torch.tensor(np.asarray(g_x, np.float32)).to(dt), torch.tensor(np.asarray(g_LP, np.float32)).to(dt)
    loss = (c["x"] * gx).sum() + (c["lp"].sum(dim=1) * gl).sum()
    ga, gb = torch.autograd.grad(loss, (c["alpha"], c["beta"]), retain_graph=True)
    return ga.numpy(), gb.numpy()


def _np(c):
    return {k: v.detach().numpy().astype(np.float64) for k, v in c.items()}


def bars(ref, g_x, g_LP):
    """dict x, lp, g_alpha, g_beta of float64 arrays [n][pix] (and the bars of p0 and x0 for near_clamp), from the float64
    composition `ref`."""
    r = _np(ref)
    al, be, u, loc, scale, a, Z, p0, z, x, zeta, lp = (r[k] for k in ("alpha", "beta", "u", "loc", "scale", "a", "Z", "p0", "z", "x",
                                                                      "zeta", "lp"))
    gx = np.asarray(g_x, np.float64)
    G = np.broadcast_to(np.asarray(g_LP, np.float64)[:, None], gx.shape)
    with np.errstate(all="ignore"):
        rel_loc = U * np.where(al < 1, 2 + np.abs(al - 1), 2.0)
        rel_scale = U * np.where(be < 1, 2 + np.abs(be - 1), 2.0)
        dpr_a, dpr_b = np.where(al < 1, np.exp(al - 1), 1.0), np.where(be < 1, np.exp(be - 1), 1.0)
        dloc, dscale = loc * rel_loc, scale * rel_scale
        da = np.abs(a) * (rel_loc + rel_scale + 2 * U)
        phi = np.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
        dPa = phi * da + 2 * U
        dZ = dPa + U * Z
        dp0 = dPa + u * dZ + 2 * U * np.abs(p0)
        mp = ((p0 >= P_LO) & (p0 <= P_HI)).astype(np.float64)
        mx = (r["x0"] >= 0).astype(np.float64)
        D = math.sqrt(2 * math.pi) * np.exp(0.5 * z * z)
        dz = mp * D * dp0 + 2 * U * np.abs(z) + U
        dx = dloc + np.abs(z) * dscale + scale * dz + U * (np.abs(scale * z) + np.abs(x))
        dzeta = dz + U * (np.abs(x) + np.abs(loc)) / scale + 3 * U * np.abs(zeta)
        dlp = (np.abs(zeta) * dzeta + U * zeta * zeta + rel_scale + U * np.abs(np.log(scale)) + dZ / Z + U * np.abs(np.log(Z))
               + 2 * U * np.abs(lp) + U)
        rs = 1.0 / scale
        gzs = G * zeta * rs
        gx0 = mx * (gx - gzs)
        dgx0 = mx * (np.abs(G) * rs * dzeta + np.abs(gzs) * (rel_scale + 2 * U) + U * (np.abs(gx) + np.abs(gzs)))
        gp = mp * gx0 * scale * D
        dgp = mp * (scale * D * dgx0 + np.abs(gp) * (rel_scale + np.abs(z) * dz + U * (4 + 0.5 * z * z)))
        br = gp * (1 - u) + G / Z
        dbr = dgp * (1 - u) + 2 * U * np.abs(gp) + np.abs(G) * dZ / (Z * Z) + 2 * U * np.abs(G / Z)
        ga = phi * br
        dga = phi * (np.abs(a) * da + U * (2 + a * a)) * np.abs(br) + phi * dbr + 2 * U * np.abs(ga)
        gloc = (gx0 + gzs) - ga * rs
        dgloc = U * (np.abs(gx) + 4 * np.abs(gzs)) + dga * rs + np.abs(ga * rs) * (rel_scale + 2 * U) + 2 * U * np.abs(gloc)
        gscale = gx0 * z + G * (zeta * zeta - 1) * rs - ga * a * rs
        dgscale = (np.abs(gx) * dz + U * np.abs(gx * z) + np.abs(gzs) * (dzeta - dz) + 4 * U * (np.abs(gzs * z) + np.abs(G) * zeta * zeta * rs)
                   + np.abs(G * rs) * (rel_scale + 2 * U) + np.abs(a) * rs * dga + np.abs(ga) * rs * da
                   + np.abs(ga * a * rs) * (rel_scale + 3 * U) + 2 * U * np.abs(gscale))
        return dict(x=dx, lp=dlp, g_alpha=dpr_a * dgloc + np.abs(dpr_a * gloc) * (rel_loc + U),
                    g_beta=dpr_b * dgscale + np.abs(dpr_b * gscale) * (rel_scale + U), p0=dp0, x0=dx)


def near_clamp(ref, bar, with_p=True):
    """bool [n][pix]: the float64 p before its clamp (with_p), or x before its clamp, lies within its bar of a clamp bound."""
    r = _np(ref)
    near_x = np.abs(r["x0"]) <= bar["x0"]
    if not with_p:
        return near_x
    return (np.abs(r["p0"] - P_LO) <= bar["p0"]) | (np.abs(r["p0"] - P_HI) <= bar["p0"]) | near_x


def case(kind, n, pix, seed, u=None, first_object=0, draw=0, operands_=None, skip_p=True):
    """Operands (of range `kind`, or operands_ = (alpha, beta)), cotangents, u (the generator's for (seed, draw, first_object) unless
    given), the float64 reference, its gradients and bars, and R per quantity: a dict.  skip_p=False (injected u that sits clearly
    on one side of a p bound, inside the bound's coarse bar): only samples next to the clamp of x are left out of the gradients."""
    alpha, beta = operands(kind, n, pix, seed) if operands_ is None else operands_
    g_x, g_LP = cotangents(n, pix, seed + 1)
    if u is None:
        u = uniforms(n, pix, seed, draw, first_object)
    ref, twin = compose(alpha, beta, u, torch.float64), compose(alpha, beta, u, torch.float32)
    bar = bars(ref, g_x, g_LP)
    want = dict(zip(("g_alpha", "g_beta"), gradients(ref, g_x, g_LP)), x=ref["x"].detach().numpy(), lp=ref["lp"].detach().numpy())
    got = dict(zip(("g_alpha", "g_beta"), gradients(twin, g_x, g_LP)), x=twin["x"].detach().numpy(), lp=twin["lp"].detach().numpy())
    skip = near_clamp(ref, bar, with_p=skip_p)
    R = {}
    for k in ("x", "lp", "g_alpha", "g_beta"):
        keep = ~skip if k.startswith("g_") else np.ones_like(skip)
        R[k] = twin_ratio(got[k][keep], want[k][keep], bar[k][keep])
    return dict(alpha=alpha, beta=beta, u=np.asarray(u, np.float32), g_x=g_x, g_LP=g_LP, ref=ref, want=want, twin=got, bar=bar, skip=skip, R=R)


def kernel_form(alpha, beta, u, g_x, g_LP):
    """csrc/head.hip's own expressions (its header: the two erfc, the quantile from the complement on the upper half, the backward's
    closed form) in numpy float32, operation by operation -- scipy's erfc / ndtri in float32 in place of the device's.  Returns the
    dict x, lp, g_alpha, g_beta.  What the CPU can say about the kernels' algebra; the device itself: tests/test_gpu_head.py."""
    from scipy.special import erfc, ndtri
    F = np.float32
    al, be, u, gx = (np.asarray(v, F) for v in (alpha, beta, u, g_x))
    G = np.broadcast_to(np.asarray(g_LP, F)[:, None], al.shape)
    with np.errstate(all="ignore"):
        ea, eb = np.exp(al - F(1)), np.exp(be - F(1))
        loc, scale = np.where(al >= 1, al, ea + F(EPS32)), np.where(be >= 1, be, eb + F(EPS32))
        dloc, dscale = np.where(al >= 1, F(1), ea), np.where(be >= 1, F(1), eb)
        a = -loc / scale
        t = a * F(math.sqrt(0.5))
        Pa, Z = F(0.5) * erfc(-t), np.maximum(F(0.5) * erfc(t), F(1e-30))
        omu = F(1) - u
        p0, q0 = Pa + u * Z, Z * omu
        upper = p0 > F(0.5)
        q_lo = F(1) - F(P_HI)
        pass_p = np.where(upper, q0 >= q_lo, p0 >= F(P_LO))
        zt = ndtri(np.where(upper, np.maximum(q0, q_lo), np.maximum(p0, F(P_LO))).astype(F)).astype(F)
        z = np.where(upper, -zt, zt)
        x0 = loc + scale * z
        x = np.maximum(x0, F(0))
        zeta = (x - loc) / scale
        lp = ((F(-0.5) * (zeta * zeta) - F(0.5 * math.log(2 * math.pi))) - np.log(scale)) - np.log(Z)
        D = F(math.sqrt(2 * math.pi)) * np.exp(F(0.5) * (z * z))
        rs = F(1) / scale
        gzs = G * zeta * rs
        gx0 = np.where(x0 >= 0, gx - gzs, F(0))
        gp = np.where(pass_p, gx0 * scale * D, F(0))
        phi = F(1 / math.sqrt(2 * math.pi)) * np.exp(F(-0.5) * (a * a))
        gA = phi * (gp * omu + G / Z)
        gloc = (gx0 + gzs) - gA * rs
        gscale = (gx0 * z + G * (zeta * zeta - F(1)) * rs) - gA * a * rs
    out = dict(x=x, lp=lp, g_alpha=gloc * dloc, g_beta=gscale * dscale)
    assert all(v.dtype == F for v in out.values())
    return out
