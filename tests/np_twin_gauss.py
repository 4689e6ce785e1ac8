"""numpy restatements of the Gaussian-approximated Poisson log-probability (the default noise model, csrc/loglik_math.h) and of
its derivatives, and the per-sample acceptance rule the tests hold the kernels to.

    reference_logp / _dlogp / _dpnm   float64, on the float32 operands (eps and pnm included) promoted to float64:
                                          loc = proj m, root = sqrt(loc / pnm + eps), scale = eps + root, z = (x - loc) / scale
                                          lp   = -z^2 / 2 - (log(2 pi) / 2 + log scale)
                                          dlp  = t1 + t2,  t1 = m z / scale,  t2 = m (z^2 - 1) / scale * du / pnm,  du = 0.5 / root
                                          dpnm = (z^2 - 1) / scale * du * (-loc / pnm^2)
    twin_logp / _dlogp / _dpnm        the expressions of loglik_math.h operation by operation in float32 (no FMA contraction: the
                                      library is built with -ffp-contract=off).  div_by() is the IEEE quotient, so the log-probability
                                      differs from the device only in logf; the derivative's reciprocals are true float32 divisions
                                      here, refined (1 / scale) and raw (1 / root: v_rcp_f32, 1 ulp) approximations on the device.
    bar_logp / _dlogp / _dpnm         a first-order float32 error bar per sample, u = 2^-24, every term in float64.  The (|x| + |loc|)
                                      terms are the sensitivity to the float32 rounding of loc and of the two quotients: with x next to
                                      loc the float32 value moves by far more than u (|t1| + |t2|), and no float32 evaluation meets a
                                      bar without them.

The rule (device): for EVERY sample |got - ref| <= MARGIN * R * bar, R = max(1, worst_excess(twin, ref, bar)) on the same operands
-- measured against the reference, never against the device -- and MARGIN = 4, np_twin_poisson's value.  R <= R_MAX is asserted on
the CPU (tests/test_gauss_loglik_cpu.py), so the twin cannot quietly widen the bar.  Where the bar is 0 (mask == 0 for dlp, loc == 0
for dpnm) the value must be exactly 0; samples whose reference is not finite must agree in kind (NaN with NaN, the same infinity).

All take proj [B][A][P], mask [B][A], x [B][A][P], a scalar pnm and a scalar eps."""
import numpy as np

F = np.float32
D = np.float64
HALF_LOG_2PI = F(0.91893853320467274178)
U = 2.0 ** -24
MARGIN = 4.0
R_MAX = 16.0
FLT_EPSILON = float(np.finfo(np.float32).eps)
MASKS = (0.0, 1.0 / 180.0, 1.0 / 20.0, 0.5, 1.0)
KINDS = ("near", "far", "zero", "tiny")


def _f32(proj, mask, x, pnm, eps):
    proj, x = np.asarray(proj, F), np.asarray(x, F)
    m = np.broadcast_to(np.asarray(mask, F)[..., None], proj.shape)
    return proj, m, x, F(pnm), F(eps)


def _f64(proj, mask, x, pnm, eps):
    proj, m, x, pnm, eps = _f32(proj, mask, x, pnm, eps)
    return proj.astype(D), m.astype(D), x.astype(D), D(pnm), D(eps)


# ---- float32 twin ------------------------------------------------------------------------------------------------------------
def _twin_terms(proj, m, pnm, eps):
    loc = proj * m
    root = np.sqrt(loc / pnm + eps)
    scale = eps + root
    return loc, root, scale


def twin_logp(proj, mask, x, pnm, eps):
    proj, m, x, pnm, eps = _f32(proj, mask, x, pnm, eps)
    with np.errstate(all="ignore"):
        loc, root, scale = _twin_terms(proj, m, pnm, eps)
        z = x / scale - loc / scale
        out = F(-0.5) * (z * z) - (HALF_LOG_2PI + np.log(scale))
    assert out.dtype == F
    return out


def _twin_derivatives(proj, mask, x, pnm, eps, drop_dscale=False, rs_once=False):
    proj, m, x, pnm, eps = _f32(proj, mask, x, pnm, eps)
    with np.errstate(all="ignore"):
        loc, root, scale = _twin_terms(proj, m, pnm, eps)
        inv_pnm = F(1.0) / pnm
        rs = F(1.0) / scale
        z = (x - loc) * rs
        dscale = (z * z - F(1.0)) * rs
        dscale_du = F(0.5) * (F(1.0) / root)
        dpnm = dscale * dscale_du * (-loc * (inv_pnm * inv_pnm))
        first = z if rs_once else z * rs
        dlp = (first if drop_dscale else first + dscale * dscale_du * inv_pnm) * m
    assert dlp.dtype == F and dpnm.dtype == F
    return dlp, dpnm


def twin_dlogp(proj, mask, x, pnm, eps):
    return _twin_derivatives(proj, mask, x, pnm, eps)[0]


def twin_dpnm(proj, mask, x, pnm, eps):
    return _twin_derivatives(proj, mask, x, pnm, eps)[1]


def twin_dlogp_without_dscale(proj, mask, x, pnm, eps):
    """A WRONG derivative (negative control): the d logp / d scale term is lost."""
    return _twin_derivatives(proj, mask, x, pnm, eps, drop_dscale=True)[0]


def twin_dlogp_rs_once(proj, mask, x, pnm, eps):
    """A WRONG derivative (negative control): (x - loc) / scale where (x - loc) / scale^2 belongs."""
    return _twin_derivatives(proj, mask, x, pnm, eps, rs_once=True)[0]


# ---- float64 reference and the bars ------------------------------------------------------------------------------------------
def _ref_terms(proj, mask, x, pnm, eps):
    proj, m, x, pnm, eps = _f64(proj, mask, x, pnm, eps)
    loc = proj * m
    root = np.sqrt(loc / pnm + eps)
    scale = eps + root
    z = (x - loc) / scale
    du = 0.5 / root
    return m, x, pnm, loc, scale, z, du


def reference_logp(proj, mask, x, pnm, eps):
    with np.errstate(all="ignore"):
        m, x, pnm, loc, scale, z, du = _ref_terms(proj, mask, x, pnm, eps)
        return -0.5 * z * z - (0.5 * np.log(2.0 * np.pi) + np.log(scale))


def reference_dlogp(proj, mask, x, pnm, eps):
    with np.errstate(all="ignore"):
        m, x, pnm, loc, scale, z, du = _ref_terms(proj, mask, x, pnm, eps)
        return m * z / scale + m * (z * z - 1.0) / scale * du / pnm


def reference_dpnm(proj, mask, x, pnm, eps):
    with np.errstate(all="ignore"):
        m, x, pnm, loc, scale, z, du = _ref_terms(proj, mask, x, pnm, eps)
        return (z * z - 1.0) / scale * du * (-loc / (pnm * pnm))


def bar_logp(proj, mask, x, pnm, eps):
    with np.errstate(all="ignore"):
        m, x, pnm, loc, scale, z, du = _ref_terms(proj, mask, x, pnm, eps)
        lp = -0.5 * z * z - (0.5 * np.log(2.0 * np.pi) + np.log(scale))
        return U * ((np.abs(x) + np.abs(loc)) / scale * np.abs(z) + np.abs(lp) + 1.0)


def bar_dlogp(proj, mask, x, pnm, eps):
    with np.errstate(all="ignore"):
        m, x, pnm, loc, scale, z, du = _ref_terms(proj, mask, x, pnm, eps)
        t1 = m * z / scale
        return U * (np.abs(t1) + m * (z * z + 1.0) / scale * du / pnm
                    + (np.abs(x) + np.abs(loc)) * (m / scale ** 2 + np.abs(2.0 * z * m * du / (pnm * scale ** 2))))


def bar_dpnm(proj, mask, x, pnm, eps):
    with np.errstate(all="ignore"):
        m, x, pnm, loc, scale, z, du = _ref_terms(proj, mask, x, pnm, eps)
        return U * ((z * z + 1.0) / scale * du * np.abs(loc) / pnm ** 2      # (|loc|: a negative ray-sum is an edge sample)
                    + (np.abs(x) + np.abs(loc)) * np.abs(2.0 * z * du * loc / (pnm ** 2 * scale ** 2)))


def excess(got, want, bar):
    """|got - want| / bar per sample; where bar == 0 the value must be exact (0 if so, inf if not).  NaN where the reference is not
    finite (those samples are compared in kind)."""
    got, want, bar = np.asarray(got, D), np.asarray(want, D), np.asarray(bar, D)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        out = np.where(bar > 0, err / bar, np.where(got == want, 0.0, np.inf))
    out = np.where(np.isnan(out), np.inf, out)                  # a NaN where the reference is finite misses every bar
    return np.where(np.isfinite(want), out, np.nan)


def worst_excess(got, want, bar):
    """(max over the samples whose reference is finite of |got - want| / bar, whether the other samples agree in kind: NaN with NaN,
    and the same infinity)."""
    got, want = np.asarray(got, D), np.asarray(want, D)
    fin = np.isfinite(want)
    e = excess(got, want, bar)[fin]
    same_rest = bool(np.array_equal(got[~fin], want[~fin], equal_nan=True))
    return (float(e.max()) if e.size else 0.0), same_rest


def twin_ratio(twin, want, bar):
    """R of the rule: the twin's own worst excess on these operands, at least 1."""
    r, same = worst_excess(twin, want, bar)
    assert same, "the float32 twin and the float64 reference disagree on which samples are finite"
    return max(1.0, r)


# ---- operands ----------------------------------------------------------------------------------------------------------------
def operands(kind, shape, pnm, seed):
    """float32 proj [B][A][P], mask [B][A] drawn from MASKS, x [B][A][P].
    near: proj in [0, 60), x = Poisson(loc pnm) / pnm -- a converged reconstruction; far: the same proj, x uniform in [0, 3) --
    the first training steps; zero: as near, every second proj exactly 0 -- the rays outside the object; tiny: proj = 10^U(-8, 0)."""
    B, A, P = shape
    rng = np.random.default_rng(seed)
    mask = rng.choice(np.asarray(MASKS, F), size=(B, A)).astype(F)
    if kind == "tiny":
        proj = (10.0 ** rng.uniform(-8.0, 0.0, shape)).astype(F)
    elif kind in ("near", "far", "zero"):
        proj = (rng.random(shape) * 60.0).astype(F)
        if kind == "zero":
            proj.reshape(-1)[::2] = 0.0
    else:
        raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")
    if kind == "far":
        x = (rng.random(shape) * 3.0).astype(F)
    else:
        loc = (proj * mask[..., None]).astype(D)
        x = (rng.poisson(loc * D(F(pnm))) / D(F(pnm))).astype(F)
    return proj, mask, x
