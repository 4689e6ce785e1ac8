"""Twins of the Beta output head (ct_pvae_amd/csrc/beta_head.hip, beta_head.h; the trainer's positive_range / Beta.rsample / clamp /
.log_prob, with TensorFlow's implicit reparameterisation gradient) and the per-sample acceptance rule the tests hold the kernels to.

    words(n, pix, seed, draw, fo)        uint32 [n][pix][2][16][4]: the Philox block of every (pixel, gamma, attempt), numpy
    search(alpha, beta, words, dtype)    the Marsaglia-Tsang attempt loop restated: the accepted attempt k, its (zn, ub), the float
                                         acceptance margin of every attempt and a float32 bar of that margin
    search_lazy(alpha, beta, seed, draw, dtype)
                                         the same k, zn, ub from the Philox blocks of the attempts a gamma reaches alone (2^20 pixels:
                                         the law tests, tests/test_beta_head_law_cpu.py), with the law tests' wrong samplers
    compose(alpha, beta, draws, dtype)   the composition of beta_head.hip's header at GIVEN accepted draws (zn, ub) [n][pix][2];
                                         float64: the definition, on the float32 operands and constants promoted; float32: the twin
                                         in the kernel's form (fp32 forward; the backward in float64 on the fp32 intermediates, as the
                                         kernel does it -- see below)
    gradients(c, g_x, g_LP)              (g_alpha, g_beta) of sum(x g_x) + sum_o g_LP[o] sum_pixels lp, the closed form with the
                                         implicit gradient dlg of each gamma
    dlg(c, lg)                           float64 d log g / d c at fixed uniform of the implicit form: the series for g <= c + 1, the
                                         continued fraction above (the kernel's two forms, run to convergence); validated against mpmath
                                         (tests/test_beta_head_cpu.py)
    bars(ref, g_x, g_LP)                 a first-order float32 error bar per sample for x, lp, g_alpha, g_beta, U = 2^-24

dlg in the kernel and in the float32 twin is FLOAT64: its two halves (log g - digamma) S and dS/dc are each sqrt(c) times the result and
digamma(a) - digamma(a + b) cancels for a >> b; an honest fp32 bar for that is tens of ulps and grows with c.  In float64 the arithmetic's
own rounding (2^-53 times the number of terms) is a named, negligible term and what remains is the fp32 rounding of the operands.

The bar follows the roundings of the named intermediates (per gamma, c = a or b, t its raw operand):
    c            relative U (2 + |t - 1|) below t = 1, exact above (pr(t) = t)
    d            c rel_c + U ([c < 1] cb + d)                (the sum c + 1 and the difference cb - 1/3, whose 1/3 is rounded too)
    s            relative dd / 2d + 3 U
    w            |s zn| (rel_s + U) + U |w|;   v = w^3: relative 3 dw / |w| + 2 U  (v = 1 exactly where w <= 0)
    log v, log d rel_v + 2 U |log v|;  dd / d + 2 U |log d|
    boost        |log(ub) / c| (rel_c + 3 U)                 (-1e7 at c = 1e-7: THE term of the small range)
    lg           the three above + U (|log d + log v| + |lg|)
    x, y         x y (expm1(D) + 2 U) + 2 U x (2 U y) + 2^-126,  D = dlg_0 + dlg_1 + U |lg_1 - lg_0|   -- "U |lg|" of the log-space
                 difference; expm1 because D is not small where |lg| ~ 1e7: a sigmoid moved by D changes by at most x y (e^D - 1);
                 2 U for expf, 2 U x for the sum and the reciprocal, 2^-126 for fp32's underflow (exp overflows from 88.7 on)
    xc, yc       dx, dy where the clamp passes, 0 where it binds (the bounds are constants)
    lp           |a - 1| (dxc / xc + 2 U |log xc|) + |log xc| (a rel_a + U |a - 1|) + U |T1|,  T2 alike with b, yc
                 + |psi(a) - psi(a + b)| a rel_a + |psi(b) - psi(a + b)| b rel_b + U (a + b) |psi(a + b)|       (lbeta's operands)
                 + 4 U (|lgamma a| + |lgamma b| + |lgamma(a + b)|) + 2 U (|lgamma a + lgamma b| + |lbeta|) + 2 U (|T1 + T2| + |lp|)
and, for the gradients (G = g_LP of the pixel's object; float64 arithmetic, so only operand errors and the final rounding):
    dlg_j        |d dlg / d lg| dlg_j + |d dlg / d c| c rel_c  (both partials by central differences of the float64 dlg)
                 + 2^-53 * 64 (1 + 9 sqrt(c)) |dlg|            (rounding times the number of series terms; no asymptotic form is used)
    K = (a - 1) / xc - (b - 1) / yc      a rel_a / xc + |a - 1| dxc / xc^2 + the same with b, yc
    gx0 = g_x + [pass] G K               [pass] |G| dK
    path_a = gx0 x y dlg_0               x y |dlg_0| dgx0 + |gx0 dlg_0| (y dx + x dy) + |gx0| x y ddlg_0
    direct_a = G (log xc - psi(a) + psi(a + b))     |G| (dxc / xc + psi'(a) a rel_a + psi'(a + b) (a rel_a + b rel_b))
    g_alpha = pr'(alpha) (path_a + direct_a)        pr' (the two above) + |g_alpha| (U (2 + |t - 1|) + U)

The rule (device): for EVERY sample |got - ref| <= MARGIN * R * bar, R = max(1, the float32 twin's own worst excess on the same
operands) and MARGIN = 4, np_twin_gauss's values; R <= R_MAX is asserted on the CPU (tests/test_beta_head_cpu.py).  Samples whose
float64 x lies within its bar of sr, or y within its bar of 1 - hi, are left out of the GRADIENT comparison where the derivative's jump
across the gate exceeds the gradient's bar (near_clamp)."""
import numpy as np
from scipy import special

from tests import np_twin_gauss as tg
from tests import np_twin_hmc

TAG = 0x42000000
ATTEMPTS = 16
KERNEL_MAX_TERMS = 2048
U = 2.0 ** -24
MARGIN, R_MAX = tg.MARGIN, tg.R_MAX
EPS32 = float(np.finfo(np.float32).eps)
RANGES = {"trainer": (-1.0, 2.0), "small": (-16.0, 0.0), "large": (1.0, 40.0), "mixed": (-3.0, 6.0)}
excess, twin_ratio = tg.excess, tg.twin_ratio
F, D = np.float32, np.float64
TINY = float(np.finfo(np.float32).tiny)


def words(n, pix, seed, draw, first_object=0, gammas=(0, 1), attempts=range(ATTEMPTS)):
    """uint32 [n][pix][len(gammas)][len(attempts)][4]: Philox((lo32(e), hi32(e), draw, TAG | j << 8 | k), seed),
    e = (first_object + o) * pix + pixel."""
    e = np.array([[(int(first_object) + o) * int(pix) + k for k in range(pix)] for o in range(n)], dtype=np.uint64)
    tags = np.array([[TAG | (j << 8) | k for k in attempts] for j in gammas], dtype=np.uint64)
    lo, hi = (e & np.uint64(0xFFFFFFFF))[..., None, None], (e >> np.uint64(32))[..., None, None]
    return np_twin_hmc.philox(lo, hi, np.uint64(draw), tags[None, None], int(seed))


def operands(kind, n, pix, seed):
    """float32 (alpha, beta) [n][pix], uniform on the raw-operand range `kind`."""
    lo, hi = RANGES[kind]
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, pix)).astype(F), rng.uniform(lo, hi, (n, pix)).astype(F)


def cotangents(n, pix, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, pix)).astype(F), rng.standard_normal(n).astype(F)


def _pr(t, dt):
    """positive_range and its slope, tn_head.h's form."""
    t = np.asarray(t, F).astype(dt)
    with np.errstate(over="ignore"):
        e = np.exp(t - dt(1))
    return np.where(t >= 1, t, e + dt(EPS32)), np.where(t >= 1, dt(1), e)


def _consts(c, dt, defect=None):
    cb = np.where(c < 1, c + dt(1), c)
    third = dt(F(1) / F(3)) if dt is F else dt(1) / dt(3)
    d = cb if defect == "d_is_cb" else cb - third
    return d, dt(1) / np.sqrt(dt(9) * d)


def search(alpha, beta, w, dtype):
    """The attempt loop on the words w [n][pix][2][16][4] in `dtype` (scipy's ndtri on the float32 u24 in place of the device's).  dict:
    k int [n][pix][2] (15 after 16 refusals), zn, ub float32 of attempt k, margin [n][pix][2][16] = rhs - log(ua) per attempt
    (accept iff w > 0 and margin > 0; -inf where w <= 0), bar: the float32 bar of that margin (U-scaled roundings of its terms, plus
    4 ulps of zn for the two ndtri implementations)."""
    dt = dtype
    c = np.stack([_pr(alpha, dt)[0], _pr(beta, dt)[0]], axis=-1)[..., None]             # [n][pix][2][1]
    d, s = _consts(c, dt)
    zn32 = special.ndtri(np_twin_hmc.u24(w[..., 0]).astype(F)).astype(F)
    zn, ua = zn32.astype(dt), np_twin_hmc.u24(w[..., 1]).astype(dt)
    with np.errstate(all="ignore"):
        wv = dt(1) + s * zn
        v = (wv * wv) * wv
        lv, lu = np.log(v), np.log(ua)
        rhs = ((dt(0.5) * (zn * zn) + d) - d * v) + d * lv
        ok = (wv > 0) & (lu < rhs)
        margin = np.where(wv > 0, rhs - lu, -np.inf).astype(D)
        dm_dzn = zn - 3 * d * s * wv * wv + 3 * d * s / wv
        bar = U * (2 * np.abs(lu) + 2 * zn * zn + 4 * d + d * v * (6 + 6 * np.abs(s * zn / wv)) + np.abs(d * lv) * 4
                   + d * 6 * np.abs(s * zn / wv) + 4 * np.abs(zn * dm_dzn))
    k = np.where(ok.any(axis=-1), ok.argmax(axis=-1), ATTEMPTS - 1)
    take = lambda a: np.take_along_axis(a, k[..., None], axis=-1)[..., 0]                 # noqa: E731
    return dict(k=k, zn=take(zn32), ub=take(np_twin_hmc.u24(w[..., 2])), margin=margin, bar=np.where(np.isfinite(bar), bar, np.inf).astype(D))


SEARCH_DEFECTS = (None, "no_squeeze", "no_half_zn2", "d_is_cb")


def search_lazy(alpha, beta, seed, draw, dtype, first_object=0, defect=None, cache=None):
    """search() without the words of attempts nobody reaches: attempt 0 of every gamma, then attempt k of those still refused only
    (their Philox blocks alone).  dict k, zn, ub [n][pix][2] -- equal to search's on the words of (seed, draw, first_object).
    defect (negative controls of the law tests; compose takes the matching one where lg changes too): "no_squeeze" accepts the first
    attempt with w > 0, "no_half_zn2" drops 0.5 zn^2 from the squeeze, "d_is_cb" takes d = cb.  cache: a dict that keeps attempt 0's
    words between calls on ONE (shape, seed, draw, first_object) -- the two dtypes and the defects draw the same."""
    assert defect in SEARCH_DEFECTS
    dt = dtype
    n, pix = np.shape(alpha)
    c = np.stack([_pr(alpha, dt)[0], _pr(beta, dt)[0]], axis=-1)                           # [n][pix][2]
    d, s = (np.broadcast_to(v, c.shape).ravel() for v in _consts(c, dt, defect))
    e = ((np.uint64(first_object) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(pix) + np.arange(pix, dtype=np.uint64)[None, :])
    e, j = np.broadcast_to(e[..., None], c.shape).ravel(), np.broadcast_to(np.arange(2, dtype=np.uint64), c.shape).ravel()
    k = np.full(e.size, ATTEMPTS - 1, np.int64)
    zn_out, ub_out = np.zeros(e.size, F), np.zeros(e.size, F)
    live = np.arange(e.size)
    for att in range(ATTEMPTS):
        el, tag = e[live], np.uint64(TAG) | (j[live] << np.uint64(8)) | np.uint64(att)
        if att == 0 and cache is not None and "w0" in cache:
            w = cache["w0"]
        else:
            w = np_twin_hmc.philox(el & np.uint64(0xFFFFFFFF), el >> np.uint64(32), np.uint64(draw), tag, int(seed))
        if att == 0 and cache is not None:
            cache["w0"] = w
        zn32 =special.ndtri(np_twin_hmc.u24(w[..., 0]).astype(F)).astype(F)
        zn, ua, dl, sl = zn32.astype(dt), np_twin_hmc.u24(w[..., 1]).astype(dt), d[live], s[live]
        with np.errstate(all="ignore"):
            wv = dt(1) + sl * zn
            v = (wv * wv) * wv
            half = dt(0) if defect == "no_half_zn2" else dt(0.5) * (zn * zn)
            rhs = ((half + dl) - dl * v) + dl * np.log(v)
            ok = (wv > 0) & ((np.log(ua) < rhs) | (defect == "no_squeeze"))
        zn_out[live], ub_out[live] = zn32, np_twin_hmc.u24(w[..., 2])                       # (the last attempt's where all refuse)
        k[live[ok]] = att
        live = live[~ok]
        if live.size == 0:
            break
    shape = c.shape
    return dict(k=k.reshape(shape), zn=zn_out.reshape(shape), ub=ub_out.reshape(shape))


# ---- float64 special functions ----------------------------------------------------------------------------------------------------
def digamma_kernel(x):
    """beta_head.h's digamma in float64: the recurrence to x >= 10 (at most 10 steps), then the asymptotic series."""
    x = np.array(x, D, copy=True)
    r = np.zeros_like(x)
    for _ in range(10):
        low = x < 10.0
        with np.errstate(all="ignore"):
            r = np.where(low, r - 1.0 / x, r)
        x = np.where(low, x + 1.0, x)
    inv = 1.0 / x
    i2 = inv * inv
    series = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 * (1.0 / 12)))))))
    return r + ((np.log(x) - 0.5 * inv) - series)


def dlg(c, lg, max_terms=200000, count=None):
    """d lg / d c at fixed uniform of the implicit form, float64, the kernel's two forms (beta_head.h) run to convergence (NaN where a
    sum has not converged after max_terms iterations; the kernel's hard bound is KERNEL_MAX_TERMS, enough for c <= 4e4).  count: a list
    that receives the largest number of iterations used."""
    c, lg = np.broadcast_arrays(np.asarray(c, D), np.asarray(lg, D))
    shape = c.shape
    c, lg = c.ravel().copy(), lg.ravel().copy()
    out = np.full(c.shape, np.nan)
    with np.errstate(all="ignore"):
        g = np.exp(lg)
        ser = ~(g > c + 1.0)
        used = 0
        if ser.any():
            cs, gs, ls = c[ser], g[ser], lg[ser]
            t, S, H, dS = np.ones_like(cs), np.ones_like(cs), np.zeros_like(cs), np.zeros_like(cs)
            live = np.isfinite(cs) & np.isfinite(gs)
            for n in range(1, max_terms + 1):
                r = 1.0 / (cs + n)
                t = np.where(live, t * gs * r, t)
                H = H + r
                S = np.where(live, S + t, S)
                dS = np.where(live, dS - t * H, dS)
                live &= ~(t * (cs + n) < 1e-17 * S)
                used = max(used, n)
                if not live.any():
                    break
            out[ser] = np.where(live, np.nan, -((ls - digamma_kernel(cs + 1.0)) * S + dS) / cs)      # not converged at the bound: NaN
        cfm = ~ser
        if cfm.any():
            cs, gs, ls = c[cfm], g[cfm], lg[cfm]
            A1, A0, B1, B0 = np.ones_like(cs), np.zeros_like(cs), np.zeros_like(cs), np.ones_like(cs)
            dA1, dA0, dB1, dB0 = (np.zeros_like(cs) for _ in range(4))
            cf, dcf = np.zeros_like(cs), np.zeros_like(cs)
            live = np.isfinite(cs) & np.isfinite(gs)
            for i in range(1, max_terms + 1):
                bi = gs + (2 * i - 1) - cs
                ai = np.ones_like(cs) if i == 1 else -(i - 1.0) * ((i - 1) - cs)
                dai = 0.0 if i == 1 else float(i - 1)
                A, B = bi * A0 + ai * A1, bi * B0 + ai * B1
                dA, dB = (bi * dA0 - A0) + (ai * dA1 + dai * A1), (bi * dB0 - B0) + (ai * dB1 + dai * B1)
                A1, B1, dA1, dB1 = A0, B0, dA0, dB0
                A0, B0, dA0, dB0 = A, B, dA, dB
                big = np.where(np.abs(B0) > 1e100, 1e-100, 1.0)
                A1, A0, B1, B0, dA1, dA0, dB1, dB0 = (v * big for v in (A1, A0, B1, B0, dA1, dA0, dB1, dB0))
                ib = 1.0 / B0
                ncf = A0 * ib
                ndcf = (dA0 - ncf * dB0) * ib
                done = (np.abs(ncf - cf) <= 1e-16 * np.abs(ncf)) & (np.abs(ndcf - dcf) <= 1e-14 * np.abs(ndcf) + 1e-300)
                cf, dcf = np.where(live, ncf, cf), np.where(live, ndcf, dcf)
                live &= ~done
                used = max(used, i)
                if not live.any():
                    break
            out[cfm] = np.where(live, np.nan, (ls - digamma_kernel(cs)) * cf + dcf)
    if count is not None:
        count.append(used)
    return out.reshape(shape)


_dlg_like = dlg


# ---- the composition --------------------------------------------------------------------------------------------------------------
def compose(alpha, beta, draws, dtype, sr=EPS32, lg=None, defect=None):
    """The composition at accepted draws (zn, ub), each float32 [n][pix][2], in `dtype`: a dict of numpy arrays of that dtype
    (gamma-wise quantities [n][pix][2]: index 0 is a's gamma, 1 is b's).  lg [n][pix][2] (tests): the gammas' logarithms given
    instead of computed from the draws.  defect (negative controls): "one_minus_x" takes y as 1 - x; the law tests' "d_is_cb" takes
    d = cb, "no_boost" leaves the boost out, "boost_cb" divides it by cb = c + 1."""
    assert defect in (None, "one_minus_x", "d_is_cb", "no_boost", "boost_cb")
    lg_given = lg
    dt = dtype
    zn, ub = (np.asarray(v, F).astype(dt) for v in draws)
    t = np.stack([np.asarray(alpha, F), np.asarray(beta, F)], axis=-1)
    c, dc = _pr(t, dt)
    d, s = _consts(c, dt, defect)
    sr, hi = dt(F(sr)), dt(F(1) - F(sr))
    with np.errstate(all="ignore"):
        w = dt(1) + s * zn
        v = np.where(w <= 0, dt(1), (w * w) * w)
        logd, logv = np.log(d), np.log(v)
        boost = np.where(c < 1, np.log(ub) / (c + dt(1) if defect == "boost_cb" else c), dt(0))
        if defect == "no_boost":
            boost = np.zeros_like(boost)
        lg = (logd + logv) + boost if lg_given is None else np.asarray(lg_given).astype(dt)
        x = dt(1) / (dt(1) + np.exp(lg[..., 1] - lg[..., 0]))
        y = dt(1) / (dt(1) + np.exp(lg[..., 0] - lg[..., 1])) if defect != "one_minus_x" else dt(1) - x
        lo_y = dt(1) - hi                                            # x > hi is tested as y < 1 - hi, the kernel's form
        passes = (x >= sr) & (y >= lo_y)
        xc = np.where(x < sr, sr, np.where(y < lo_y, hi, x))
        yc = np.where(x < sr, hi, np.where(y < lo_y, lo_y, y))
        a, b = c[..., 0], c[..., 1]
        lga, lgb, lgab = (special.gammaln(q).astype(dt) for q in (a, b, a + b))
        T1, T2 = (a - dt(1)) * np.log(xc), (b - dt(1)) * np.log(yc)
        lbeta = (lga + lgb) - lgab
        lp = (T1 + T2) - lbeta
    out = dict(t=t, c=c, dc=dc, d=d, s=s, zn=zn, ub=ub, w=w, v=v, logd=logd, logv=logv, boost=boost, lg=lg, x=x, y=y, passes=passes,
               xc=xc, yc=yc, a=a, b=b, lga=lga, lgb=lgb, lgab=lgab, T1=T1, T2=T2, lbeta=lbeta, lp=lp, sr=sr, hi=hi, lo_y=lo_y)
    assert all(v.dtype == dt for k, v in out.items() if k not in ("t", "passes", "sr", "hi", "lo_y")), [k for k, v in out.items() if getattr(v, "dtype", dt) != dt]
    return out


def gradients(c, g_x, g_LP, defect=None, dlg_=None, defect_scale=1.0):
    """(g_alpha, g_beta) of the composition's dtype: float64 arithmetic on the composition's intermediates (promoted), the closed form
    of beta_head.hip's header; rounded to float32 once when the composition is the float32 twin.  defect (negative controls):
    "dlg_1e-4" scales dlg by 1 + 1e-4 * defect_scale, "no_gate" lets lp's path through x pass the clamp.  dlg_ = (d0, d1): the
    float64 dlg of the two gammas computed before (several cotangents on one composition)."""
    assert defect in (None, "dlg_1e-4", "no_gate")
    dt = c["x"].dtype.type
    a, b, x, y, xc, yc = (c[k].astype(D) for k in ("a", "b", "x", "y", "xc", "yc"))
    lg = c["lg"].astype(D)
    gx = np.asarray(g_x, F).astype(D)
    G = np.broadcast_to(np.asarray(g_LP, F).astype(D)[:, None], gx.shape)
    with np.errstate(all="ignore"):
        gx0 = np.where(c["passes"] | (defect == "no_gate"), gx + G * ((a - 1.0) / xc - (b - 1.0) / yc), gx)
        xy = x * y
        dead = (gx0 == 0.0) | (xy == 0.0)
        d0, d1 = (_dlg_like(a, lg[..., 0]), _dlg_like(b, lg[..., 1])) if dlg_ is None else dlg_
        if defect == "dlg_1e-4":
            d0, d1 = d0 * (1 + 1e-4 * defect_scale), d1 * (1 + 1e-4 * defect_scale)
        pa = np.where(dead, 0.0, gx0 * xy * d0)
        pb = np.where(dead, 0.0, -(gx0 * xy * d1))
        pab = digamma_kernel(a + b)
        da = np.where(G != 0, G * ((np.log(xc) - digamma_kernel(a)) + pab), 0.0)
        db = np.where(G != 0, G * ((np.log(yc) - digamma_kernel(b)) + pab), 0.0)
        ga, gb = (pa + da) * c["dc"][..., 0].astype(D), (pb + db) * c["dc"][..., 1].astype(D)
    return ga.astype(dt), gb.astype(dt)


def bars(ref, g_x, g_LP):
    """dict x, lp, g_alpha, g_beta of float64 arrays [n][pix], from the float64 composition `ref` (the module docstring names the terms)."""
    r = ref
    t, c, d, s, zn, w, v, logd, logv, boost, lg = (r[k] for k in ("t", "c", "d", "s", "zn", "w", "v", "logd", "logv", "boost", "lg"))
    a, b, x, y, xc, yc, passes = (r[k] for k in ("a", "b", "x", "y", "xc", "yc", "passes"))
    gx = np.asarray(g_x, D)
    G = np.broadcast_to(np.asarray(g_LP, D)[:, None], gx.shape)
    with np.errstate(all="ignore"):
        rel_t = U * (2 + np.abs(t - 1))
        rel_c = np.where(t < 1, rel_t, 0.0)
        cb = np.where(c < 1, c + 1, c)
        dd = c * rel_c + U * (np.where(c < 1, cb, 0.0) + d)
        rel_s = dd / (2 * d) + 3 * U
        dw = np.abs(s * zn) * (rel_s + U) + U * np.abs(w)
        rel_v = np.where(w <= 0, 0.0, 3 * dw / np.abs(w) + 2 * U)
        dlogv = rel_v + 2 * U * np.abs(logv)
        dlogd = dd / d + 2 * U * np.abs(logd)
        dboost = np.abs(boost) * (rel_c + 3 * U)
        dlg_ = dlogd + dlogv + dboost + U * (np.abs(logd + logv) + np.abs(lg))
        Dl = dlg_[..., 0] + dlg_[..., 1] + U * np.abs(lg[..., 1] - lg[..., 0])
        E = np.expm1(np.minimum(Dl, 50.0))
        dx, dy = x * y * (E + 2 * U) + 2 * U * x + TINY, x * y * (E + 2 * U) + 2 * U * y + TINY
        dxc, dyc = np.where(passes, dx, 0.0), np.where(passes, dy, 0.0)
        rel_a, rel_b = rel_c[..., 0], rel_c[..., 1]
        lxc, lyc = np.log(xc), np.log(yc)
        pa_, pb_, pab_ = special.digamma(a), special.digamma(b), special.digamma(a + b)
        dlp = (np.abs(a - 1) * (dxc / xc + 2 * U * np.abs(lxc)) + np.abs(lxc) * (a * rel_a + U * np.abs(a - 1)) + U * np.abs(r["T1"])
               + np.abs(b - 1) * (dyc / yc + 2 * U * np.abs(lyc)) + np.abs(lyc) * (b * rel_b + U * np.abs(b - 1)) + U * np.abs(r["T2"])
               + np.abs(pa_ - pab_) * a * rel_a + np.abs(pb_ - pab_) * b * rel_b + U * (a + b) * np.abs(pab_)
               + 4 * U * (np.abs(r["lga"]) + np.abs(r["lgb"]) + np.abs(r["lgab"])) + 2 * U * (np.abs(r["lga"] + r["lgb"]) + np.abs(r["lbeta"]))
               + 2 * U * (np.abs(r["T1"] + r["T2"]) + np.abs(r["lp"])))
        # dlg and its partials (central differences of the float64 form)
        h_l, h_c = 1e-6 * np.maximum(1.0, np.abs(lg)), 1e-6 * c
        dl = _dlg_like(c, lg)
        p_l = (_dlg_like(c, lg + h_l) - _dlg_like(c, lg - h_l)) / (2 * h_l)
        p_c = (_dlg_like(c + h_c, lg) - _dlg_like(c - h_c, lg)) / (2 * h_c)
        ddl = np.abs(p_l) * dlg_ + np.abs(p_c) * c * rel_c + 2.0 ** -53 * 64 * (1 + 9 * np.sqrt(c)) * np.abs(dl)
        K = (a - 1) / xc - (b - 1) / yc
        dK = a * rel_a / xc + np.abs(a - 1) * dxc / (xc * xc) + b * rel_b / yc + np.abs(b - 1) * dyc / (yc * yc)
        gx0 = np.where(passes, gx + G * K, gx)
        dgx0 = np.where(passes, np.abs(G) * dK, 0.0)
        xy = x * y
        out = {}
        for j, name, rel_j, xcj, dxcj in ((0, "g_alpha", rel_a, xc, dxc), (1, "g_beta", rel_b, yc, dyc)):
            dpath = xy * np.abs(dl[..., j]) * dgx0 + np.abs(gx0 * dl[..., j]) * (y * dx + x * dy) + np.abs(gx0) * xy * ddl[..., j]
            dpath = np.where((gx0 == 0) | (xy == 0), 0.0, dpath)
            cj = c[..., j]
            ddirect = np.abs(G) * (dxcj / xcj + special.polygamma(1, cj) * cj * rel_j + special.polygamma(1, a + b) * (a * rel_a + b * rel_b))
            path = np.where((gx0 == 0) | (xy == 0), 0.0, gx0 * xy * dl[..., j]) * (1 if j == 0 else -1)
            direct = G * ((np.log(xcj) - special.digamma(cj)) + pab_)
            gj = r["dc"][..., j] * (path + direct)
            out[name] = r["dc"][..., j] * (dpath + ddirect) + np.abs(gj) * (rel_t[..., j] + U)
            out["jump_a" if j == 0 else "jump_b"] = np.abs(G * K * xy * dl[..., j] * r["dc"][..., j])
        out.update(x=dx, y=dy, lp=dlp)
        return out


def near_clamp(ref, bar):
    """bool [n][pix]: the float64 x lies within its bar of sr, or y within its bar of 1 - hi (the upper bound in the form the gate
    tests it), AND the gate matters: the jump of a gradient across it, |G K x y dlg_j pr'|, exceeds that gradient's bar."""
    near = (np.abs(ref["x"] - ref["sr"]) <= bar["x"]) | (np.abs(ref["y"] - ref["lo_y"]) <= bar["y"])
    return near & ((bar["jump_a"] > bar["g_alpha"]) | (bar["jump_b"] > bar["g_beta"]))


def case(kind, n, pix, seed, draws=None, first_object=0, draw=0, operands_=None, sr=EPS32):
    """Operands (of range `kind`, or operands_ = (alpha, beta)), cotangents, accepted draws (the float32 search's on the numpy Philox
    words of (seed, draw, first_object) unless given), the float64 reference, its gradients and bars, and R per quantity: a dict."""
    alpha, beta = operands(kind, n, pix, seed) if operands_ is None else operands_
    g_x, g_LP = cotangents(n, pix, seed + 1)
    if draws is None:
        sch = search(alpha, beta, words(n, pix, seed, draw, first_object), F)
        draws = (sch["zn"], sch["ub"])
    ref, twin = compose(alpha, beta, draws, D, sr), compose(alpha, beta, draws, F, sr)
    bar = bars(ref, g_x, g_LP)
    want = dict(zip(("g_alpha", "g_beta"), gradients(ref, g_x, g_LP)), x=ref["x"], lp=ref["lp"])
    got = dict(zip(("g_alpha", "g_beta"), gradients(twin, g_x, g_LP)), x=twin["x"], lp=twin["lp"])
    skip = near_clamp(ref, bar)
    R = {}
    for k in ("x", "lp", "g_alpha", "g_beta"):
        keep = ~skip if k.startswith("g_") else np.ones_like(skip)
        R[k] = twin_ratio(got[k][keep], want[k][keep], bar[k][keep])
    return dict(alpha=alpha, beta=beta, draws=draws, g_x=g_x, g_LP=g_LP, ref=ref, want=want, twin=got, bar=bar, skip=skip, R=R)
