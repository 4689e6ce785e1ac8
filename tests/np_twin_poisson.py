"""numpy restatements of the exact Poisson log-probability (noise="poisson", csrc/loglik_math.h).

    twin_logp / twin_dlogp   the expression the kernels evaluate, operation by operation, in float32 (no FMA contraction: the
                             library is built with -ffp-contract=off).  They differ from the device only in the implementations
                             of log / log1p / lgamma (numpy's and scipy's against ocml's, a few ulp each).
    naive_logp               the textbook form k log(lam) - lgamma(k + 1) - lam in float32: what NOT to evaluate.
    reference_logp / _dlogp  float64: TFP 0.14's Poisson._log_prob, multiply_no_nan(log lam, k) - lgamma(k + 1) - lam, with
                             scipy.special.gammaln, on the float32 operands promoted to float64.

All take proj [B][A][P], mask [B][A], x [B][A][P] and a scalar pnm."""
import numpy as np
from scipy.special import gammaln

F = np.float32
HALF_LOG_2PI = F(0.91893853320467274178)
STIRLING_MIN = F(8.0)
C1, C2, C3 = F(0.083333333333333333), F(0.0027777777777777778), F(0.00079365079365079365)


def _f32(proj, mask, x, pnm):
    proj, x = np.asarray(proj, F), np.asarray(x, F)
    m = np.broadcast_to(np.asarray(mask, F)[..., None], proj.shape)
    return proj, m, x, F(pnm)


def twin_logp(proj, mask, x, pnm):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        lam = (proj * m) * pnm
        k = x * pnm
        kk = np.where(k > 0, k, F(1.0))                     # (lanes with k <= 0 take the edge branch below)
        u = (lam - kk) / kk
        ik = F(1.0) / kk
        ik2 = ik * ik
        series = ik * (C1 - ik2 * (C2 - ik2 * C3))
        r_big = (HALF_LOG_2PI + F(0.5) * np.log(kk)) + series
        r_small = gammaln(kk + F(1.0)).astype(F) - (kk * np.log(kk) - kk)
        r = np.where(kk >= STIRLING_MIN, r_big, r_small)
        l1p = np.where(u < F(-0.5), np.log(lam / kk), np.log1p(u))
        lp = kk * (l1p - u) - r
        edge = np.where(k == 0, -lam, np.where(k < 0, F(-np.inf), k))
        edge = np.where(lam >= 0, edge, F(np.nan))
        out = np.where(k > 0, lp, edge)
    assert out.dtype == F
    return out


def twin_dlogp(proj, mask, x, pnm):
    proj, m, x, pnm = _f32(proj, mask, x, pnm)
    with np.errstate(all="ignore"):
        mp = m * pnm
        lam = (proj * m) * pnm
        k = x * pnm
        out = np.where(k == 0, -mp, mp * ((k - lam) / lam))
    return out.astype(F)


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
