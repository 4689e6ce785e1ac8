"""Twins of the fused Beta latent block (ct_pvae_amd/csrc/beta_latent.hip; the trainer's positive_range / Beta.rsample / kl_divergence
against Beta(0.5, 0.5), with TensorFlow's implicit reparameterisation gradient), built on tests/np_twin_beta.py: the sampler (search),
the gamma part of compose, dlg and the bars of x, y and lg are that file's, unchanged.  This file adds

    words(n, length, seed, draw, level, s, fo)   uint32 [n][length][2][16][4]: the Philox blocks under the LATENTS' fourth counter word
                                                 0x51000000 | level << 16 | s << 5 | gamma << 4 | attempt
    search_lazy(loc, ls, seed, draw, level, s, dtype, fo, defect)
                                                 the accepted (k, zn, ub) from the blocks a gamma reaches alone (the law tests), with
                                                 two wrong packings of the counter word as negative controls
    kl(a, b)                                     float64 KL(Beta(a, b) || Beta(1/2, 1/2)), scipy's betaln and digamma:
                                                 ln pi - lbeta(a, b) + (a - 1/2) psi(a) + (b - 1/2) psi(b) + (1 - a - b) psi(a + b)
    kl_grad(a, b, trigamma)                      its closed-form gradient ((a - 1/2) psi'(a) + m psi'(a + b), (b - 1/2) psi'(b) + m psi'(a + b)),
                                                 m = 1 - a - b (the digamma terms cancel exactly)
    trigamma_kernel(x)                           beta_head.h's beta_trigamma restated: the recurrence to x >= 10, then the series
    lgamma_digamma_kernel(x), kl_kernel(a, b)    beta_head.h's beta_lgamma_digamma restated operation by operation, and the KL term as
                                                 the kernel evaluates it with it (the float32 twin's kl)
    compose(loc, ls, draws, dtype)               per sample s the composition of np_twin_beta at GIVEN accepted draws [ns][n][len][2], and
                                                 kl; float64: the definition on the float32 operands promoted; float32: the kernel's form
                                                 (fp32 a, b, lg, z, y; kl in float64 on the fp32 a, b rounded once)
    gradients(c, g_z, g_KL)                      (g_loc, g_ls): float64 arithmetic on the composition's intermediates, ascending s, the KL
                                                 term last, times pr', rounded once for the float32 twin
    bars(ref, g_z, g_KL)                         first-order float32 bars of z, kl, g_loc, g_ls (U = 2^-24)
    ordered_sum(kl_row)                          quad_io.h's fixed order of the per-object sum, in float32

The bars.  a = pr(loc), b = pr(log_scale) carry np_twin_beta's relative error rel_c (U (2 + |t - 1|) below t = 1, exact above); the
kernel evaluates kl and its gradient in FLOAT64 on those fp32 a, b, so what remains is the operands' error through the first
derivatives, the final rounding and a named float64 term:
    kl           a rel_a |(a - 1/2) psi'(a) + m psi'(a + b)| + b rel_b |(b - 1/2) psi'(b) + m psi'(a + b)|          (d kl / da, d kl / db)
                 + U |kl|                                                                                        (the final rounding)
                 + kl_float64_bound: the counted float64 roundings of the kernel's own lgamma / digamma (lgamma_digamma_bounds: their
                   Stirling terms are of size 20 even where lgamma itself vanishes) through the combination, + 8 * 2^-53 of the six terms
    h_a = (a - 1/2) psi'(a) + m psi'(a + b)    (the KL part of g_a is G h_a; h_b alike)
                 a rel_a (|psi'(a)| + |(a - 1/2) psi''(a)| + |psi'(a + b)| + |m psi''(a + b)|) + b rel_b (|psi'(a + b)| + |m psi''(a + b)|)
                 -- the partial derivatives term by term, absolute values added (an upper bound of the first-order error)
                 + 2^-53 * 64 (|(a - 1/2) psi'(a)| + |m psi'(a + b)|)
    g_loc        sum over s of np_twin_beta's bar of the path g_z[s] z y dlg_0 (its g_alpha bar at g_LP = 0: the errors of z, y, lg and of
                 dlg's operands, pr' and the rounding included) + pr'(loc) |G| (h_a's bar) + |pr' G h_a| (U (2 + |t - 1|) + U)
    g_ls         alike with b, dlg_1, h_b.
The rule (device) is np_twin_beta's: every sample within MARGIN * R * bar, MARGIN = 4, R = max(1, the float32 twin's own worst excess on
the same operands), asserted <= R_MAX on the CPU (tests/test_beta_latent_cpu.py)."""
import numpy as np
from scipy import special

from tests import np_twin_beta as tb
from tests import np_twin_hmc

TAG = 0x51000000
ATTEMPTS = tb.ATTEMPTS
MAX_NS = 2048
U = tb.U
MARGIN, R_MAX = tb.MARGIN, tb.R_MAX
RANGES = tb.RANGES
F, D = np.float32, np.float64
LN_PI = float(np.log(np.pi))
FP64 = 2.0 ** -53 * 64
EPS64 = 2.0 ** -53


def word3(level, s, gamma, attempt):
    return TAG | (int(level) << 16) | (int(s) << 5) | (int(gamma) << 4) | int(attempt)


def words(n, length, seed, draw, level, s, first_object=0, gammas=(0, 1), attempts=range(ATTEMPTS)):
    """uint32 [n][length][len(gammas)][len(attempts)][4]: Philox((lo32(e), hi32(e), draw, word3(level, s, j, k)), seed),
    e = (first_object + b) * length + i."""
    e = (np.uint64(first_object) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(length) + np.arange(length, dtype=np.uint64)[None, :]
    tags = np.array([[word3(level, s, j, k) for k in attempts] for j in gammas], dtype=np.uint64)
    lo, hi = (e & np.uint64(0xFFFFFFFF))[..., None, None], (e >> np.uint64(32))[..., None, None]
    return np_twin_hmc.philox(lo, hi, np.uint64(draw), tags[None, None], int(seed))


SEARCH_DEFECTS = (None, "s_dropped", "gamma_overlaps_attempt")


def search_lazy(loc, ls, seed, draw, level, s, dtype, first_object=0, defect=None):
    """np_twin_beta.search_lazy under the latents' counter word: attempt 0 of every gamma, then attempt k of those still refused only.
    dict k, zn, ub [n][len][2].  defect (negative controls of the law tests, wrong packings of the word): "s_dropped" leaves the sample
    index out (every sample draws sample 0's numbers), "gamma_overlaps_attempt" puts gamma on the attempt's lowest bit (gamma 1's first attempt
    is gamma 0's second, and its second repeats its first)."""
    assert defect in SEARCH_DEFECTS
    dt = dtype
    n, length = np.shape(loc)
    c = np.stack([tb._pr(loc, dt)[0], tb._pr(ls, dt)[0]], axis=-1)
    d, sc = (np.broadcast_to(v, c.shape).ravel() for v in tb._consts(c, dt))
    e = (np.uint64(first_object) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(length) + np.arange(length, dtype=np.uint64)[None, :]
    e, j = np.broadcast_to(e[..., None], c.shape).ravel(), np.broadcast_to(np.arange(2, dtype=np.uint64), c.shape).ravel()
    s_word = 0 if defect == "s_dropped" else int(s)
    g_shift = 0 if defect == "gamma_overlaps_attempt" else 4
    base = np.uint64(TAG | (int(level) << 16) | (s_word << 5))
    k = np.full(e.size, ATTEMPTS - 1, np.int64)
    zn_out, ub_out = np.zeros(e.size, F), np.zeros(e.size, F)
    live = np.arange(e.size)
    for att in range(ATTEMPTS):
        el, tag = e[live], base | (j[live] << np.uint64(g_shift)) | np.uint64(att)
        w = np_twin_hmc.philox(el & np.uint64(0xFFFFFFFF), el >> np.uint64(32), np.uint64(draw), tag, int(seed))
        zn32 = special.ndtri(np_twin_hmc.u24(w[..., 0]).astype(F)).astype(F)
        zn, ua, dl, sl = zn32.astype(dt), np_twin_hmc.u24(w[..., 1]).astype(dt), d[live], sc[live]
        with np.errstate(all="ignore"):
            wv = dt(1) + sl * zn
            v = (wv * wv) * wv
            rhs = ((dt(0.5) * (zn * zn) + dl) - dl * v) + dl * np.log(v)
            ok = (wv > 0) & (np.log(ua) < rhs)
        zn_out[live], ub_out[live] = zn32, np_twin_hmc.u24(w[..., 2])
        k[live[ok]] = att
        live = live[~ok]
        if live.size == 0:
            break
    return dict(k=k.reshape(c.shape), zn=zn_out.reshape(c.shape), ub=ub_out.reshape(c.shape))


# ---- the KL term ------------------------------------------------------------------------------------------------------------------
def trigamma_kernel(x):
    """beta_head.h's beta_trigamma in float64: psi'(x) = psi'(x + 1) + 1 / x^2 up to x >= 10 (at most 10 steps), then the series."""
    x = np.array(x, D, copy=True)
    r = np.zeros_like(x)
    for _ in range(10):
        low = x < 10.0
        with np.errstate(all="ignore"):
            r = np.where(low, r + 1.0 / (x * x), r)
        x = np.where(low, x + 1.0, x)
    inv = 1.0 / x
    i2 = inv * inv
    series = i2 * (1.0 / 6 - i2 * (1.0 / 30 - i2 * (1.0 / 42 - i2 * (1.0 / 30 - i2 * (5.0 / 66 - i2 * (691.0 / 2730 - i2 * (7.0 / 6)))))))
    return r + (inv + (0.5 * i2 + inv * series))


def lgamma_digamma_kernel(x):
    """beta_head.h's beta_lgamma_digamma in float64, operation by operation: ten steps of the recurrences taken while x < 10 (the factors
    multiplied into p, the reciprocals kept as the fraction q / p, q <- q x + p), then Stirling's series and the digamma's on the
    shifted x, sharing log x and 1 / x.  Returns (lgamma, digamma)."""
    x = np.array(x, D, copy=True)
    p, q = np.ones_like(x), np.zeros_like(x)
    with np.errstate(all="ignore"):
        for _ in range(10):
            low = x < 10.0
            q = np.where(low, q * x + p, q)
            p = np.where(low, p * x, p)
            x = np.where(low, x + 1.0, x)
        inv = 1.0 / x
        i2, lx = inv * inv, np.log(x)
        stirling = inv * (1.0 / 12 - i2 * (1.0 / 360 - i2 * (1.0 / 1260 - i2 * (1.0 / 1680 - i2 * (1.0 / 1188 - i2 * (691.0 / 360360 - i2 * (1.0 / 156 - i2 * (3617.0 / 122400))))))))
        series = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 * (1.0 / 12)))))))
        lg = ((((x - 0.5) * lx - x) + 0.91893853320467274178) + stirling) - np.log(p)
        psi = ((lx - 0.5 * inv) - series) - q / p
    return lg, psi


def lgamma_digamma_bounds(x):
    """Absolute float64 error bounds (lgamma, digamma) of lgamma_digamma_kernel against the exact functions, from counting its
    roundings (EPS64 = 2^-53), with xs >= 10 the shifted argument and p the product of the factors:
      digamma  the shift q / p: two roundings of q and one of p in each of ten steps and the division, 31 in all: 32 EPS64 (q / p) --
               1 / x for small x, THE term there; ln xs, 1 / 2xs and the series: 8 EPS64 (|ln xs| + 1)
      lgamma   (xs - 1/2) ln xs and xs: 8 EPS64 of each; ln p: p's ten roundings are 10 EPS64 absolute in ln p, the logarithm's own
               2 EPS64 |ln p|, the two sums 2 EPS64: 12 EPS64 + 2 EPS64 |ln p|
    plus EPS64 of the value itself (the rounding of whatever float64 reference it is compared with)."""
    x = np.asarray(x, D)
    with np.errstate(all="ignore"):
        xs = x + np.clip(np.ceil(10.0 - x), 0, 10)
        lnp = special.gammaln(xs) - special.gammaln(x)
        shift = special.digamma(xs) - special.digamma(x)
        b_lg = EPS64 * (8 * (np.abs((xs - 0.5) * np.log(xs)) + xs) + 2 * np.abs(lnp) + 12) + EPS64 * np.abs(special.gammaln(x))
        b_psi = EPS64 * (32 * shift + 8 * (np.abs(np.log(xs)) + 1.0)) + EPS64 * np.abs(special.digamma(x))
    return b_lg, b_psi


def kl_float64_bound(a, b):
    """The float64 term of the kl bar: the bounds above through the KL term's combination -- the three lgammas, the digammas times
    their factors -- plus 8 EPS64 of the six terms' absolute sum for the combination's own roundings."""
    a, b = np.asarray(a, D), np.asarray(b, D)
    m, ab = (1.0 - a) - b, a + b
    (la, pa), (lb, pb), (lab, pab) = (lgamma_digamma_bounds(x) for x in (a, b, ab))
    with np.errstate(all="ignore"):
        terms = (np.abs(special.gammaln(a)) + np.abs(special.gammaln(b)) + np.abs(special.gammaln(ab)) + np.abs((a - 0.5) * special.digamma(a))
                 + np.abs((b - 0.5) * special.digamma(b)) + np.abs(m * special.digamma(ab)) + LN_PI)
        return (la + lb + lab) + (np.abs(a - 0.5) * pa + np.abs(b - 0.5) * pb + np.abs(m) * pab) + 8 * EPS64 * terms


def kl_kernel(a, b):
    """The kernel's form of the KL term (beta_latent.hip's beta_latent_kl): float64, lgamma and digamma from lgamma_digamma_kernel."""
    a, b = np.asarray(a, D), np.asarray(b, D)
    (la, pa), (lb, pb), (lab, pab) = lgamma_digamma_kernel(a), lgamma_digamma_kernel(b), lgamma_digamma_kernel(a + b)
    return ((LN_PI - ((la + lb) - lab)) + ((a - 0.5) * pa + (b - 0.5) * pb)) + ((1.0 - a) - b) * pab


def kl(a, b):
    a, b = np.asarray(a, D), np.asarray(b, D)
    return ((LN_PI - special.betaln(a, b)) + ((a - 0.5) * special.digamma(a) + (b - 0.5) * special.digamma(b))) + ((1.0 - a) - b) * special.digamma(a + b)


def kl_grad(a, b, trigamma=None):
    tg = (lambda x: special.polygamma(1, x)) if trigamma is None else trigamma
    a, b = np.asarray(a, D), np.asarray(b, D)
    m, tab = (1.0 - a) - b, tg(a + b)
    return (a - 0.5) * tg(a) + m * tab, (b - 0.5) * tg(b) + m * tab


def operands(kind, n, length, seed):
    """float32 (loc, log_scale) [n][length], uniform on the raw-operand range `kind` of np_twin_beta."""
    return tb.operands(kind, n, length, seed)


def cotangents(ns, n, length, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ns, n, length)).astype(F), rng.standard_normal(n).astype(F)


def compose(loc, ls, draws, dtype):
    """draws = (zn, ub), each float32 [ns][n][len][2].  dict: s -- the list over the samples of np_twin_beta.compose's dicts (z is their
    x) --, a, b, dc [n][len](x 2), t, and kl of `dtype`."""
    zn, ub = draws
    per = [tb.compose(loc, ls, (zn[s], ub[s]), dtype) for s in range(np.shape(zn)[0])]
    a, b = per[0]["a"], per[0]["b"]
    with np.errstate(all="ignore"):
        # float64: the definition (scipy); float32: the kernel's own float64 form on the fp32 a, b, rounded once
        k = kl(a, b) if dtype is D else kl_kernel(a, b).astype(F)
    return dict(s=per, a=a, b=b, dc=per[0]["dc"], t=per[0]["t"], kl=k, z=np.stack([p["x"] for p in per]))


def gradients(c, g_z, g_KL, dlg_=None):
    """(g_loc, g_ls) [n][len] of the composition's dtype for the cotangents g_z [ns][n][len] (None: zero) and g_KL [n] (None: zero).
    dlg_: the list over s of (d0, d1) computed before."""
    dt = c["kl"].dtype.type
    a, b = c["a"].astype(D), c["b"].astype(D)
    n, length = a.shape
    pa, pb = np.zeros((n, length)), np.zeros((n, length))
    with np.errstate(all="ignore"):
        if g_z is not None:
            for s, p in enumerate(c["s"]):
                gz = np.asarray(g_z[s], F).astype(D)
                zy = p["x"].astype(D) * p["y"].astype(D)
                dead = (gz == 0.0) | (zy == 0.0)
                lg = p["lg"].astype(D)
                d0, d1 = (tb.dlg(a, lg[..., 0]), tb.dlg(b, lg[..., 1])) if dlg_ is None else dlg_[s]
                pa = np.where(dead, pa, pa + (gz * zy) * d0)
                pb = np.where(dead, pb, pb - (gz * zy) * d1)
        if g_KL is not None:
            G = np.broadcast_to(np.asarray(g_KL, F).astype(D)[:, None], a.shape)
            ha, hb = kl_grad(a, b, trigamma_kernel if dt is F else None)
            pa = np.where(G != 0, pa + G * ha, pa)
            pb = np.where(G != 0, pb + G * hb, pb)
        return (pa * c["dc"][..., 0].astype(D)).astype(dt), (pb * c["dc"][..., 1].astype(D)).astype(dt)


def z_bar(p):
    """np_twin_beta.bars' bar of x for one sample's float64 composition p, restated term by term (that function also evaluates dlg five
    times per gamma for the gradients' bars, which a caller that wants values alone does not need); tests/test_beta_latent_cpu.py holds
    the two to equal bits."""
    t, c, d, s, zn, w, logd, logv, boost, lg, x, y = (p[k] for k in ("t", "c", "d", "s", "zn", "w", "logd", "logv", "boost", "lg", "x", "y"))
    with np.errstate(all="ignore"):
        rel_c = np.where(t < 1, U * (2 + np.abs(t - 1)), 0.0)
        cb = np.where(c < 1, c + 1, c)
        dd = c * rel_c + U * (np.where(c < 1, cb, 0.0) + d)
        rel_s = dd / (2 * d) + 3 * U
        dw = np.abs(s * zn) * (rel_s + U) + U * np.abs(w)
        rel_v = np.where(w <= 0, 0.0, 3 * dw / np.abs(w) + 2 * U)
        dlg_ = (dd / d + 2 * U * np.abs(logd)) + (rel_v + 2 * U * np.abs(logv)) + np.abs(boost) * (rel_c + 3 * U) + U * (np.abs(logd + logv) + np.abs(lg))
        Dl = dlg_[..., 0] + dlg_[..., 1] + U * np.abs(lg[..., 1] - lg[..., 0])
        return x * y * (np.expm1(np.minimum(Dl, 50.0)) + 2 * U) + 2 * U * x + tb.TINY


def bars(ref, g_z, g_KL, values_only=False):
    """dict z [ns][n][len], kl, g_loc, g_ls [n][len] of float64 arrays, from the float64 composition (the module docstring names the
    terms).  values_only: z and kl alone (z's bar from z_bar; g_loc and g_ls are then not returned)."""
    a, b, t, dc = ref["a"], ref["b"], ref["t"], ref["dc"]
    n, length = a.shape
    ns = len(ref["s"])
    gz = np.zeros((ns, n, length)) if g_z is None else np.asarray(g_z, D)
    G = np.broadcast_to((np.zeros(n) if g_KL is None else np.asarray(g_KL, D))[:, None], a.shape)
    with np.errstate(all="ignore"):
        rel_t = U * (2 + np.abs(t - 1))
        rel_c = np.where(t < 1, rel_t, 0.0)
        ea, eb = a * rel_c[..., 0], b * rel_c[..., 1]                  # the absolute errors of the fp32 a, b
        m, ab = (1.0 - a) - b, a + b
        p1a, p1b, p1ab = (special.polygamma(1, x) for x in (a, b, ab))
        p2a, p2b, p2ab = (special.polygamma(2, x) for x in (a, b, ab))
        ha, hb = kl_grad(a, b)
        k = ref["kl"]
        dkl = ea * np.abs(ha) + eb * np.abs(hb) + U * np.abs(k) + kl_float64_bound(a, b)
        cross = np.abs(p1ab) + np.abs(m * p2ab)
        dha = ea * (np.abs(p1a) + np.abs((a - 0.5) * p2a) + cross) + eb * cross + FP64 * (np.abs((a - 0.5) * p1a) + np.abs(m * p1ab))
        dhb = eb * (np.abs(p1b) + np.abs((b - 0.5) * p2b) + cross) + ea * cross + FP64 * (np.abs((b - 0.5) * p1b) + np.abs(m * p1ab))
        out = dict(kl=dkl, z=[])
        gl = dc[..., 0] * np.abs(G) * dha + np.abs(dc[..., 0] * G * ha) * (rel_t[..., 0] + U)
        gs = dc[..., 1] * np.abs(G) * dhb + np.abs(dc[..., 1] * G * hb) * (rel_t[..., 1] + U)
        if values_only:
            out["z"] = np.stack([z_bar(p) for p in ref["s"]])
            return out
        for s, p in enumerate(ref["s"]):
            pb_ = tb.bars(p, gz[s], np.zeros(n))
            out["z"].append(pb_["x"])
            gl, gs = gl + pb_["g_alpha"], gs + pb_["g_beta"]
        out["z"] = np.stack(out["z"])
        out.update(g_loc=gl, g_ls=gs)
    return out


def ordered_sum(row):
    """quad_io.h's order of additions applied to one object's kl_elem, in float32."""
    length = row.shape[0]
    quads = (length + 3) // 4
    padded = np.zeros(4 * quads, F)
    padded[:length] = row
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
    for mask in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ mask]).astype(F)
    total = v[0, 0]
    for w in range(1, 16):
        total = F(total + v[w, 0])
    return total


def case(kind, n, length, ns, seed, draws=None, first_object=0, draw=0, level=0, operands_=None, g_z=True, g_KL=True):
    """Operands (of range `kind`, or operands_ = (loc, ls)), cotangents (g_z / g_KL False: that cotangent is absent), accepted draws
    (the float32 search's on the numpy Philox words unless given), the float64 reference, the float32 twin, bars and R per quantity."""
    loc, ls = operands(kind, n, length, seed) if operands_ is None else operands_
    gz, gk = cotangents(ns, n, length, seed + 1)
    gz, gk = (gz if g_z else None), (gk if g_KL else None)
    if draws is None:
        sch = [tb.search(loc, ls, words(n, length, seed, draw, level, s, first_object), F) for s in range(ns)]
        draws = (np.stack([r["zn"] for r in sch]), np.stack([r["ub"] for r in sch]))
    ref, twin = compose(loc, ls, draws, D), compose(loc, ls, draws, F)
    bar = bars(ref, gz, gk)
    want = dict(zip(("g_loc", "g_ls"), gradients(ref, gz, gk)), z=ref["z"], kl=ref["kl"])
    got = dict(zip(("g_loc", "g_ls"), gradients(twin, gz, gk)), z=twin["z"], kl=twin["kl"])
    R = {k: tb.twin_ratio(got[k], want[k], bar[k]) for k in want}
    return dict(loc=loc, ls=ls, draws=draws, g_z=gz, g_KL=gk, ref=ref, want=want, twin=got, bar=bar, R=R)
