"""numpy twin of every store of the ray-driven projector pair (csrc/siddon.hip): what each forward form and each back-projector
instantiation must write, given the CPU oracle's ray-sums (oracle._project_grid / siddon_project) and back-projections
(oracle.siddon_backproject) -- those two are held to exact float64 chords in tests/test_oracle.py.

Stores that are a few correctly rounded float32 operations are written here in np.float32 in the order siddon.hip writes them (the
library is built with -ffp-contract=off and its '/' is the IEEE quotient, so the BITS are expected):

    forward  (siddon_fwd_store, siddon_ratio_store)            back-projector (siddon_bwd_gather_kernel's EPI)
      sirt_update   (meas - sim) / w where w != 0, else 0        sirt_add   x + bp / colsum where colsum != 0, else x         (EPI 1)
      ratio         meas / sim where sim != 0, else 0            scaled     scale[s] * bp, or bp                             (EPI 3)
      tv_dual       (p + w (sim - meas)) / (1 + w)               multiply   x * (bp / colsum) where colsum != 0, else x      (EPI 4)

Whole iterations (EPI 2: the TV primal step, EPI 5: the penalized update, and the two-launch iterations of every algorithm) are
what exists: oracle.sirt, oracle.tv_standin, tests/np_twin_mlem.py, tests/np_twin_pml.py (`recon`).  The likelihood stores are
oracle.loglik and the float64 references and bars of tests/np_twin_gauss.py / tests/np_twin_poisson.py (`gauss`, `poisson`).

Arrays: sim / meas / p / ratio [oy][rows][dx], w [rows][dx], x / bp [oy][gx][gy], colsum [gx][gy], scale [oy]."""
import numpy as np

from oracle import radon_oracle as orc
from tests import np_twin_gauss as tg
from tests import np_twin_mlem as tm
from tests import np_twin_pml as tp
from tests import np_twin_poisson as tpo

F = np.float32


def _f(*arrays):
    out = [np.asarray(a, F) for a in arrays]
    return out if len(out) > 1 else out[0]


# ---- the projector pair (the oracle's) -------------------------------------------------------------------------------------------
def raysums(x, theta, dx):
    """A x on a dx-wide detector with center dx / 2: [oy][gx][gy] -> [oy][dt][dx]."""
    return orc._project_grid(x, np.ascontiguousarray(theta, F), int(dx))


def backproject(data, theta, gx, gy):
    """A^T data in libtomo's order of terms: [oy][dt][dx] -> [oy][gx][gy]."""
    return orc.siddon_backproject(data, np.ascontiguousarray(theta, F), gx, gy)


# ---- forward stores --------------------------------------------------------------------------------------------------------------
def sirt_update(sim, meas, w):
    sim, meas, w = _f(sim, meas, w)
    with np.errstate(all="ignore"):
        out = np.where(w != 0, (meas - sim) / w, F(0.0))
    assert out.dtype == F
    return out


def ratio(sim, meas):
    sim, meas = _f(sim, meas)
    with np.errstate(all="ignore"):
        out = np.where(sim != 0, meas / sim, F(0.0))
    assert out.dtype == F
    return out


def tv_dual(p, sim, meas, w):
    p, sim, meas, w = _f(p, sim, meas, w)
    out = (p + w * (sim - meas)) / (F(1.0) + w)
    assert out.dtype == F
    return out


# ---- back-projector stores -------------------------------------------------------------------------------------------------------
def sirt_add(x, bp, colsum):
    x, bp, colsum = _f(x, bp, colsum)
    with np.errstate(all="ignore"):
        out = np.where(colsum != 0, x + bp / colsum, x)
    assert out.dtype == F
    return out


def multiply(x, bp, colsum):
    x, bp, colsum = _f(x, bp, colsum)
    with np.errstate(all="ignore"):
        out = np.where(colsum != 0, x * (bp / colsum), x)
    assert out.dtype == F
    return out


def scaled(bp, scale=None):
    bp = _f(bp)
    if scale is None:
        return bp
    s = _f(scale).reshape(-1)
    out = (s[:, None, None] if s.size > 1 else s[0]) * bp
    assert out.dtype == F
    return out


# ---- whole iterations ------------------------------------------------------------------------------------------------------------
ALGORITHMS = ("sirt", "tv", "mlem", "osem", "pml_quad", "ospml_hybrid")


def recon(algorithm, data, theta, num_iter, gx, gy, num_block=1, ind_block=None, reg_par=None):
    """recon(data, theta, sinogram_order=True, algorithm=..., num_iter=..., num_gridx=gx, num_gridy=gy) from the default start
    (1e-6 everywhere): data [oy][dt][dx] -> [oy][gx][gy].  reg_par as the product takes it (None: ones)."""
    data, theta = np.ascontiguousarray(data, F), np.ascontiguousarray(theta, F)
    par = np.ones(2) if reg_par is None else np.asarray(reg_par, np.float64).reshape(-1)
    if algorithm == "sirt":
        return orc.sirt(data, theta, num_iter, gx, gy)
    if algorithm == "tv":
        return orc.tv_standin(data, theta, num_iter, lam=float(par[0]), ngridx=gx, ngridy=gy)
    if algorithm in ("mlem", "osem"):
        return tm.mlem(data, theta, num_iter, ngridx=gx, ngridy=gy, num_block=num_block if algorithm == "osem" else 1,
                       ind_block=ind_block if algorithm == "osem" else None)
    if algorithm in ("pml_quad", "pml_hybrid", "ospml_quad", "ospml_hybrid"):
        blocked = algorithm.startswith("os")
        hybrid = algorithm.endswith("hybrid")
        return tp.pml(data, theta, num_iter, beta=float(par[0]), delta=float(par[1]) if hybrid else 1.0, hybrid=hybrid, ngridx=gx,
                      ngridy=gy, num_block=num_block if blocked else 1, ind_block=ind_block if blocked else None)
    raise ValueError(f"no twin for algorithm {algorithm!r}")


# ---- likelihood stores -----------------------------------------------------------------------------------------------------------
def gauss(sim, mask, x, pnm, eps):
    """The Gaussian store on ray-sums `sim`: the oracle's float32 log-probability, and np_twin_gauss's float64 references with the
    bars of its rule, MARGIN * R * bar with R the float32 twin's own worst excess (at least 1): a dict of lp_oracle, lp_ref, lp_bar,
    dlp_ref, dlp_bar."""
    a = (sim, mask, x, pnm, eps)
    lp_ref, lp_bar = tg.reference_logp(*a), tg.bar_logp(*a)
    dlp_ref, dlp_bar = tg.reference_dlogp(*a), tg.bar_dlogp(*a)
    return {"lp_oracle": orc.loglik(sim, mask, x, pnm, eps),
            "lp_ref": lp_ref, "lp_bar": tg.MARGIN * tg.twin_ratio(tg.twin_logp(*a), lp_ref, lp_bar) * lp_bar,
            "dlp_ref": dlp_ref, "dlp_bar": tg.MARGIN * tg.twin_ratio(tg.twin_dlogp(*a), dlp_ref, dlp_bar) * dlp_bar}


def gauss_excess(got, ref, bar):
    """(worst |got - ref| / bar over the samples with a finite reference: <= 1 passes; whether the other samples agree in kind)."""
    return tg.worst_excess(got, ref, bar)


def poisson(sim, mask, x, pnm):
    """The Poisson store on ray-sums `sim`: np_twin_poisson's float64 reference with bar_from_twin's bars: (want, atol, rtol)."""
    want, atol, rtol, _, _ = tpo.bar_from_twin(sim, mask, x, pnm)
    return want, atol, rtol


def poisson_excess(got, want, atol, rtol):
    """(worst |got - want| / (atol + rtol |want|): <= 1 passes; whether the non-finite samples agree exactly)."""
    r, _, same = tpo.worst_excess(got, want, atol, rtol)
    return r, same


# ---- operands of the matrix tests (tests/test_siddon_matrix_cpu.py, tests/test_gpu_siddon_matrix.py) ----------------------------
GRIDS = ((12, 70), (33, 47), (100, 258), (160, 258))     # ragged gather tiles; odd (degenerate rays); one slice in LDS; none
SUBSET = (16, 2, 2, 9, 0, 15, 7)                          # an angle subset: out of order, with a repeat
ZERO_ANGLE = 3                                            # the angle whose data are all zero (the gather's live-angle skip)


def angles():
    """17 float32 angles -- more than one LDS chunk of 15 in the gather: along the grid lines both ways and back, the diagonal and
    its float32 neighbour, a rational slope, ten seeded draws over more than a turn either way."""
    fixed = [0.0, np.pi / 2, np.pi / 4, np.pi, -np.pi / 2, np.arctan(0.5), np.nextafter(F(np.pi / 4), F(1.0))]
    return np.concatenate([np.asarray(fixed, F), np.random.default_rng(17).uniform(-7.0, 7.0, 10).astype(F)])


def detector(grid):
    """The detector of the recon-level cells: 200 bins (even), 59 (odd) on the odd grid."""
    return 59 if grid[0] % 2 else 200


def images(oy, grid, seed, positive=False):
    """[oy][gx][gy] float32, both signs unless `positive`; slice 1 (where there is one) is all zero."""
    rng = np.random.default_rng(seed)
    x = rng.random((oy,) + tuple(grid), dtype=F) + F(0.05) if positive else rng.standard_normal((oy,) + tuple(grid)).astype(F)
    if oy > 1:
        x[1] = 0.0
    return x


def sinograms(oy, dt, dx, seed, positive=False):
    """[oy][dt][dx] float32 as `images`; row ZERO_ANGLE (where there is one) of every slice and all of slice 1 are zero."""
    rng = np.random.default_rng(seed)
    y = rng.random((oy, dt, dx), dtype=F) * F(3.0) if positive else rng.standard_normal((oy, dt, dx)).astype(F)
    if dt > ZERO_ANGLE:
        y[:, ZERO_ANGLE] = 0.0
    if oy > 1:
        y[1] = 0.0
    return y


def weights(shape, seed):
    """Positive float32 weights (rn2 / sigma [dt][dx], colsum [gx][gy]) of which every seventh is exactly 0."""
    w = (np.random.default_rng(seed).random(shape, dtype=F) + F(0.25))
    w.reshape(-1)[::7] = 0.0
    return w
