"""What the law tests of the samplers share (tests/test_beta_head_law_cpu.py, test_head_law_cpu.py and the device files beside them):
the probability integral transforms of the laws the heads claim to sample, from scipy's CDFs and closed forms alone -- not from the
twins -- and the ONE threshold of every Kolmogorov assertion.

    ks_uniform(u)                 two-sided Kolmogorov distance of a sample from U(0, 1), float64
    dkw(N, alpha=1e-6)            sqrt(log(2 / alpha) / (2 N)): the Dvoretzky-Kiefer-Wolfowitz bound (Massart's constant).  Derived, not
                                  tuned: a correct sampler exceeds it with probability at most alpha per statistic, at every N
    corr_bound(N)                 5.5 / sqrt(N) for the sample correlation of two independent PIT vectors (standard error 1 / sqrt(N):
                                  5.5 standard errors, 4e-8 two-sided)
    pit_log_gamma(c, lg)          P(c, exp(lg)), the regularised lower incomplete gamma, for the LOGARITHM of a Gamma(c, 1) sample
    pit_beta(a, b, x, y)          the Beta(a, b) CDF at x, from the upper tail's side where x >= 0.5 (y is the sampler's own 1 - x)
    pit_truncnorm(loc, scale, x)  the CDF of N(loc, scale^2) truncated to [0, inf)
    pit_normal(z)                 Phi(z)

Every PIT takes per-sample parameters: the PITs of samples with DIFFERENT parameters are all U(0, 1), so their pool is too, and one
statistic tests a whole operand range."""
import math

import numpy as np
from scipy import special

D = np.float64


def ks_uniform(u):
    """sup_t |F_N(t) - t| of the sample u (any shape), float64."""
    u = np.sort(np.asarray(u, D).ravel())
    n = u.size
    assert n > 0 and np.isfinite(u).all() and u[0] >= 0.0 and u[-1] <= 1.0
    i = np.arange(1, n + 1, dtype=D)
    return float(max(np.max(i / n - u), np.max(u - (i - 1) / n)))


def dkw(N, alpha=1e-6):
    return math.sqrt(math.log(2.0 / alpha) / (2.0 * N))


def corr_bound(N):
    return 5.5 / math.sqrt(N)


def corr(p, q):
    """Sample correlation of two PIT vectors, float64."""
    p, q = np.asarray(p, D).ravel(), np.asarray(q, D).ravel()
    p, q = p - p.mean(), q - q.mean()
    return float((p * q).sum() / math.sqrt((p * p).sum() * (q * q).sum()))


def pit_log_gamma(c, lg):
    """P(c, exp(lg)).  Where exp(lg) underflows (lg < -700: concentrations of 1e-3 and below put lg near -1 / c times an exponential
    variate) the series' leading term exp(c lg - lgamma(c + 1)); its relative error is below g c / (c + 1) < exp(lg)."""
    c, lg = np.broadcast_arrays(np.asarray(c, D), np.asarray(lg, D))
    with np.errstate(under="ignore"):
        lead = np.exp(c * lg - special.gammaln(c + 1.0))
        return np.where(lg < -700.0, lead, special.gammainc(c, np.exp(np.maximum(lg, -700.0))))


def pit_beta(a, b, x, y):
    """I_x(a, b) (scipy.stats.beta.cdf(x, a, b) is this function) where x < 0.5, 1 - I_y(b, a) otherwise."""
    a, b, x, y = np.broadcast_arrays(*(np.asarray(v, D) for v in (a, b, x, y)))
    return np.where(x < 0.5, special.betainc(a, b, x), 1.0 - special.betainc(b, a, y))


def pit_truncnorm(loc, scale, x):
    """(Phi((x - loc) / scale) - Phi(-loc / scale)) / (1 - Phi(-loc / scale)); with loc > 0 the denominator is at least 0.5."""
    loc, scale, x = np.broadcast_arrays(*(np.asarray(v, D) for v in (loc, scale, x)))
    pa = special.ndtr(-loc / scale)
    return (special.ndtr((x - loc) / scale) - pa) / (1.0 - pa)


def pit_normal(z):
    return special.ndtr(np.asarray(z, D))
