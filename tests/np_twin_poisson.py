"""numpy restatements of the exact Poisson log-probability (noise="poisson", csrc/loglik_math.h).

    twin_logp / twin_dlogp   the expression the kernels evaluate, operation by operation, in float32 (no FMA contraction: the
                             library is built with -ffp-contract=off).  They differ from the device only in the implementations
                             of log / log1p / lgamma (numpy's and scipy's against ocml's, a few ulp each).
    naive_logp               the textbook form k log(lam) - lgamma(k + 1) - lam in float32: what NOT to evaluate.
    reference_logp / _dlogp  float64: TFP 0.14's Poisson._log_prob, multiply_no_nan(log lam, k) - lgamma(k + 1) - lam, with
                             scipy.special.gammaln, on the float32 operands promoted to float64.

    bar_logp / bar_dlogp     a first-order float32 error bar per sample, U = 2^-24, every term in float64 on the float32 operands
                             promoted to float64 (lam = proj m pnm, k = x pnm, u = (lam - k) / k).  The terms, each with the
                             rounding it stands for:
                               lp, k > 0    2 |k - lam|                      the two roundings of lam = (proj m) pnm, carried by
                                                                             d lp / d lam = (k - lam) / lam
                                            k |log lam - digamma(k + 1)|     the rounding of k = x pnm, carried by d lp / d k
                                            2 k (|log1p(u)| + |u|)           the cancellation in k (l1p - u): l1p and u rounded,
                                                                             their difference taken, the product with k
                                            2 rho(k)                         the Stirling remainder r(k): below 8 lgammaf(k + 1),
                                                                             k logf(k) and k as they stand (rho = |lgamma(k + 1)| +
                                                                             |k log k| + k), from 8 on 0.5 log(2 pi k) and the
                                                                             series (rho = |0.5 log(2 pi k)| + 1 / 12k)
                                            |lp| + 1                         the rounding of the result and of the last difference,
                                                                             and one ulp of a term of order 1 (the few-ulp
                                                                             logf / log1pf / lgammaf next to a result near 0)
                               lp, k == 0   2 |lam|                          the two roundings of lam; lp = -lam
                               dlp, k != 0  m pnm (|k| / |lam| + 2)          the roundings of k and (twice) of lam through
                                                                             (k - lam) / lam = k / lam - 1, and of m pnm
                                            6 |dlp|                          the difference, the quotient, the product, the
                                                                             product with an upstream gradient, twice over
                               dlp, k == 0  m pnm                            the rounding of m pnm; dlp = -m pnm
                             A term that is not finite counts as 0: such a sample's reference is not finite either, and those
                             are compared in kind.
    operands                 near / far / zero / tiny of np_twin_gauss, and three kinds aimed at the seams of poisson_logp.

The per-sample rule is np_twin_gauss's: |got - ref| <= MARGIN * R * bar for EVERY sample, R = max(1, the twin's own worst excess
on the same operands) <= R_MAX; where the bar is 0 (mask == 0 with k == 0; an upstream gradient of 0) the value is exactly 0;
samples whose reference is not finite agree in kind.  excess / worst_excess (as `worst_excess_bar` here: the older atol / rtol
`worst_excess` keeps its name) / twin_ratio / MARGIN / R_MAX are that module's, not copies.

All take proj [B][A][P], mask [B][A], x [B][A][P] and a scalar pnm."""
import numpy as np
from scipy.special import digamma, gammaln

from tests import np_twin_gauss as tg

F = np.float32
HALF_LOG_2PI = F(0.91893853320467274178)
STIRLING_MIN = F(8.0)
C1, C2, C3 = F(0.083333333333333333), F(0.0027777777777777778), F(0.00079365079365079365)


def _f32(proj, mask, x, pnm):
    proj, x = np.asarray(proj, F), np.asarray(x, F)
    m = np.broadcast_to(np.asarray(mask, F)[..., None], proj.shape)
    return proj, m, x, F(pnm)


def twin_logp(proj, mask, x, pnm, c2=C2, always_log1p=False):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        lam = (proj * m) * pnm
        k = x * pnm
        kk = np.where(k > 0, k, F(1.0))                     # (lanes with k <= 0 take the edge branch below)
        u = (lam - kk) / kk
        ik = F(1.0) / kk
        ik2 = ik * ik
        series = ik * (C1 - ik2 * (c2 - ik2 * C3))
        r_big = (HALF_LOG_2PI + F(0.5) * np.log(kk)) + series
        r_small = gammaln(kk + F(1.0)).astype(F) - (kk * np.log(kk) - kk)
        r = np.where(kk >= STIRLING_MIN, r_big, r_small)
        l1p = np.log1p(u) if always_log1p else np.where(u < F(-0.5), np.log(lam / kk), np.log1p(u))
        lp = kk * (l1p - u) - r
        edge = np.where(k == 0, -lam, np.where(k < 0, F(-np.inf), k))
        edge = np.where(lam >= 0, edge, F(np.nan))
        out = np.where(k > 0, lp, edge)
    assert out.dtype == F
    return out


def twin_dlogp(proj, mask, x, pnm, without_mask=False, general_at_zero=False):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        mp = np.broadcast_to(pnm, m.shape) if without_mask else m * pnm
        lam = (proj * m) * pnm
        k = x * pnm
        general = mp * ((k - lam) / lam)
        out = general if general_at_zero else np.where(k == 0, -mp, general)
    return out.astype(F)


def twin_logp_without_c2(proj, mask, x, pnm):
    """A WRONG log-probability (negative control): the Stirling series without its second term, 1 / (360 k^3) -- 5e-6 at k = 8."""
    return twin_logp(proj, mask, x, pnm, c2=F(0.0))


def twin_logp_always_log1p(proj, mask, x, pnm):
    """A WRONG log-probability (negative control): log1pf(u) also where u < -0.5, with no logf(lam / k) branch."""
    return twin_logp(proj, mask, x, pnm, always_log1p=True)


def twin_dlogp_without_mask(proj, mask, x, pnm):
    """A WRONG derivative (negative control): the factor pnm where mask * pnm belongs."""
    return twin_dlogp(proj, mask, x, pnm, without_mask=True)


def twin_dlogp_general_at_zero(proj, mask, x, pnm):
    """A WRONG derivative (negative control): no k == 0 case, so lam == 0 with k == 0 gives NaN where -mask * pnm belongs."""
    return twin_dlogp(proj, mask, x, pnm, general_at_zero=True)


def naive_logp(proj, mask, x, pnm):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        lam = (proj * m) * pnm
        k = x * pnm
        out = np.where(k == 0, F(0.0), k * np.log(lam)) - gammaln(k + F(1.0)).astype(F) - lam
    return out.astype(F)


def reference_logp(proj, mask, x, pnm):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    proj, m, x, pnm = proj.astype(np.float64), m.astype(np.float64), x.astype(np.float64), np.float64(pnm)
    with np.errstate(all="ignore"):
        lam = proj * m * pnm
        k = x * pnm
        safe_k = np.maximum(k, 0.0)
        y = np.where(k == 0, 0.0, k * np.log(lam)) - gammaln(1.0 + safe_k)          # multiply_no_nan(log_rate, x) - lgamma(1 + x)
        y = np.where(k == safe_k, y, -np.inf)                                       # outside the support
        return y - lam + np.where(lam < 0, np.nan, 0.0)                             # - exp(log_rate); a negative rate's log is NaN


def reference_dlogp(proj, mask, x, pnm):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    proj, m, x, pnm = proj.astype(np.float64), m.astype(np.float64), x.astype(np.float64), np.float64(pnm)
    with np.errstate(all="ignore"):
        lam = proj * m * pnm
        k = x * pnm
        return np.where(k == 0, -m * pnm, m * pnm * (k - lam) / lam)


def errors(got, want):
    """(max abs error over samples whose reference is finite, indices agree on the non-finite ones)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    same_rest = bool(np.array_equal(got[~fin], want[~fin], equal_nan=True))
    return (float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0), same_rest


# The acceptance bar of the GPU tests: |got - want| <= atol + rtol * |want| per sample, both taken from the TWIN's error on the same
# operands, times MARGIN.  Samples whose |want| is below BIG set atol (their error is absolute: cancellation, lgamma), the others
# (k = 0 at a large rate: want = -lam, up to 1e5) set rtol (their error is the rounding of the result itself; floor: half an ulp).
MARGIN = 4.0
BIG = 1.0e3


def bar_from_twin(proj, mask, x, pnm):
    want = reference_logp(proj, mask, x, pnm)
    twin = twin_logp(proj, mask, x, pnm).astype(np.float64)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):                     # (-inf against -inf)
        err = np.abs(twin - want)
    small, big = fin & (np.abs(want) < BIG), fin & (np.abs(want) >= BIG)
    e_abs = float(err[small].max()) if small.any() else 0.0
    e_rel = float((err[big] / np.abs(want[big])).max()) if big.any() else 0.0
    e_rel = max(e_rel, 2.0 ** -24)
    if small.any():                                         # floor: half an ulp of the largest such value
        e_abs = max(e_abs, 2.0 ** -24 * float(np.abs(want[small]).max()))
    return want, MARGIN * e_abs, MARGIN * e_rel, e_abs, e_rel


def worst_excess(got, want, atol, rtol):
    """max over finite-reference samples of |got - want| / (atol + rtol |want|) (<= 1 passes), the max abs error, and whether the
    non-finite samples agree exactly."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    ratio = err / (atol + rtol * np.abs(want[fin]))
    same_rest = bool(np.array_equal(got[~fin], want[~fin], equal_nan=True))
    return (float(ratio.max()) if fin.any() else 0.0), (float(err.max()) if fin.any() else 0.0), same_rest


# ---- the per-sample rule (np_twin_gauss's: |got - ref| <= MARGIN * R * bar) ----------------------------------------------------------
U = tg.U
R_MAX = tg.R_MAX
assert MARGIN == tg.MARGIN
excess, worst_excess_bar, twin_ratio = tg.excess, tg.worst_excess, tg.twin_ratio


def _f64(proj, mask, x, pnm):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    return proj.astype(np.float64), m.astype(np.float64), x.astype(np.float64), np.float64(pnm)


def _finite_or_0(t):
    return np.where(np.isfinite(t), t, 0.0)


def bar_logp(proj, mask, x, pnm):
    """The float32 error bar of lp per sample (the terms: this module's docstring)."""
    proj, m, x, pnm = _f64(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        lam = proj * m * pnm
        k = x * pnm
        kk = np.where(k > 0, k, 1.0)
        u = (lam - kk) / kk
        lp = reference_logp(proj, mask, x, pnm)
        rho = np.where(kk >= float(STIRLING_MIN), np.abs(0.5 * np.log(2.0 * np.pi * kk)) + 1.0 / (12.0 * kk),
                       np.abs(gammaln(kk + 1.0)) + np.abs(kk * np.log(kk)) + kk)
        terms = (2.0 * np.abs(kk - lam), kk * np.abs(np.log(lam) - digamma(kk + 1.0)), 2.0 * kk * (np.abs(np.log1p(u)) + np.abs(u)),
                 2.0 * rho, np.abs(lp) + 1.0)
        general = U * sum(_finite_or_0(t) for t in terms)
        return np.where(k > 0, general, np.where(k == 0, U * 2.0 * _finite_or_0(np.abs(lam)), 0.0))


def bar_dlogp(proj, mask, x, pnm):
    """The float32 error bar of d lp / d proj per sample (the terms: this module's docstring)."""
    proj, m, x, pnm = _f64(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        lam = proj * m * pnm
        k = x * pnm
        mp = m * pnm
        dlp = reference_dlogp(proj, mask, x, pnm)
        general = U * (_finite_or_0(mp * (np.abs(k) / np.abs(lam) + 2.0)) + 6.0 * _finite_or_0(np.abs(dlp)))
        return np.where(k == 0, U * mp, general)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
MASKS = tg.MASKS
SEAM_KINDS = ("seam_k", "seam_u", "small_k")
KINDS = tg.KINDS + SEAM_KINDS


def operands(kind, shape, pnm, seed):
    """float32 proj [B][A][P], mask [B][A], x [B][A][P].  near / far / zero / tiny: np_twin_gauss.operands (masks from MASKS, 0
    included).  The three kinds below draw k and lam, take masks from the non-zero MASKS and return x = float32(k / pnm) and
    proj = float32(lam / (mask pnm)):
        seam_k   k = 8 (1 +- 10^U(-7.5, -1)), lam = k exp(N(0, 0.5)): both sides of kPoissonStirlingMin, down to the float32 values
                 next to 8, and sample 0 with float32 k == 8 exactly
        seam_u   k = 10^U(-1, 6), lam = 0.5 k (1 +- 10^U(-7.5, -1)): both sides of u = -0.5, where logf(lam / k) hands over to log1pf(u)
        small_k  k = 10^U(-4, log10 8) (never an integer), lam = 10^U(-4, 2): lgammaf's range, with u on either side of -0.5"""
    if kind in tg.KINDS:
        return tg.operands(kind, shape, pnm, seed)
    if kind not in SEAM_KINDS:
        raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")
    B, A, P = shape
    rng = np.random.default_rng(seed)
    mask = rng.choice(np.asarray(MASKS[1:], F), size=(B, A)).astype(F)
    sign = rng.choice(np.float64([-1.0, 1.0]), size=shape)
    near = 1.0 + sign * 10.0 ** rng.uniform(-7.5, -1.0, shape)
    if kind == "seam_k":
        k = 8.0 * near
        lam = k * np.exp(rng.normal(0.0, 0.5, shape))
    elif kind == "seam_u":
        k = 10.0 ** rng.uniform(-1.0, 6.0, shape)
        lam = 0.5 * k * near
    else:
        k = 10.0 ** rng.uniform(-4.0, np.log10(8.0), shape)
        k = np.where(k == np.round(k), k * (1.0 - 2.0 ** -20), k)
        lam = 10.0 ** rng.uniform(-4.0, 2.0, shape)
    p32 = F(pnm)
    x = (k / np.float64(p32)).astype(F)
    if kind == "small_k":                                    # (x * pnm rounds in float32: keep every k below the seam)
        while (x * p32 >= STIRLING_MIN).any():
            x = np.where(x * p32 >= STIRLING_MIN, np.nextafter(x, F(0.0)), x)
    if kind == "seam_k":                                     # sample 0: float32 k == 8 exactly
        cands = [F(8.0 / np.float64(p32))]
        for toward in (F(0.0), F(np.inf)):                   # (the quotient's neighbours, should its product round off 8)
            c = cands[0]
            for _ in range(4):
                c = np.nextafter(c, toward)
                cands.append(c)
        hit = [c for c in cands if c * p32 == STIRLING_MIN]
        assert hit, f"no float32 x with x * {pnm:g} == 8"
        x.reshape(-1)[0] = hit[0]
    proj = (lam / (mask[..., None].astype(np.float64) * np.float64(p32))).astype(F)
    return proj, mask, x
