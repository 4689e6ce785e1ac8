"""numpy restatement of the HMC sampler of ct_pvae_amd/csrc/hmc.hip (its header states the target), generic in dtype and vectorised
over chains.  [3P-recalled: TFP 0.14's TransformedTransitionKernel(HamiltonianMonteCarlo, IteratedSigmoidCentered) under
SimpleStepSizeAdaptation -- restated from memory; tests/test_hmc_cpu.py pins the derivative against torch.autograd.]

The projector is two dense 0 / 1 matrices taken ONCE from the CPU oracle (rotate_fwd on unit images, rotate_bwd_tfcompat on unit
cotangents): the forward is linear in the object, so the nearest taps are the oracle's, not re-derived here.  float32: every
operation in float32 (the kernel's expressions; numpy's log / exp / cos and numpy's order of sums instead of the device's).
float64: the same formulas on the same float32 inputs and the same draws, with the textbook Poisson log-probability."""
import numpy as np
from scipy.special import gammaln

from tests import np_twin_poisson as tp

TAG = 0x484D43
TINY = np.finfo(np.float32).tiny


# ---- Philox4x32-10, vectorised (checked against the oracle's on first use) -----------------------------------------
def _philox(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


_checked = False


def philox(c0, c1, c2, c3, seed):
    global _checked
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    if not _checked:
        from oracle import radon_oracle
        for ctr in ((0, 0, 0, 0), (7, 3, 0xFFFFFFFF, TAG), (123456, 99, 15, TAG)):
            assert np.array_equal(_philox(*ctr, k0, k1), radon_oracle.philox4x32_10(ctr, (k0, k1)))
        _checked = True
    return _philox(c0, c1, c2, c3, k0, k1)


def u24(w):
    """((w >> 8) + 0.5f) * 2^-24, in float32 as the kernel takes it."""
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def draws(seed, chain_ids, t, K, dtype):
    """(momenta [C][K-1], log u [C]) of step t: Box-Muller on word pairs (0, 1), (2, 3) of block k // 4; u of block 0xFFFFFFFF."""
    chain_ids = np.asarray(chain_ids, np.uint64)
    nb = (K - 1 + 3) // 4
    w = philox(np.uint64(t), chain_ids[:, None], np.arange(nb, dtype=np.uint64)[None, :], TAG, seed)       # [C][nb][4]
    u = u24(w).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(u[..., 0::2]))                                                          # [C][nb][2]
    ang = dtype(np.float32(2.0 * np.pi)) * u[..., 1::2]
    n = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1).reshape(len(chain_ids), nb * 4)[:, :K - 1]
    wu = philox(np.uint64(t), chain_ids, 0xFFFFFFFF, TAG, seed)[:, 0]
    return n.astype(dtype), np.log(u24(wu).astype(dtype))


# ---- the model ---------------------------------------------------------------------------------------------------
def projector_matrices(oracle, theta, N):
    """(F [A N][K], B [K][A N]) of the nearest rotate-and-sum on the unpadded N x N canvas and of its tf_compat backward."""
    geom = oracle.Geometry(N, N, False)
    T8 = oracle.rotate_transforms(theta, N, N)
    K, A = N * N, T8.shape[0]
    F = oracle.rotate_fwd(np.eye(K, dtype=np.float32).reshape(K, N, N), geom, T8).reshape(K, A * N).T
    B = oracle.rotate_bwd_tfcompat(np.eye(A * N, dtype=np.float32).reshape(A * N, A, N), geom, oracle.invert_transforms(T8)).reshape(A * N, K).T
    return np.ascontiguousarray(F, np.float64), np.ascontiguousarray(B, np.float64)


def prior_tables(weights, alpha):
    """(logw [M], alpha [M][K], lbeta [M]) in float32, computed in float64 and rounded once (what hmc_sample uploads)."""
    alpha = np.atleast_2d(np.asarray(alpha, np.float64))
    alpha = alpha.astype(np.float32).astype(np.float64)
    lbeta = gammaln(alpha).sum(-1) - gammaln(alpha.sum(-1))
    return np.log(np.asarray(weights, np.float64)).astype(np.float32), alpha.astype(np.float32), lbeta.astype(np.float32)


class Model:
    def __init__(self, oracle, theta, N, mask, meas, pnm, weights, alpha, chains_per_object=1):
        self.N, self.K = N, N * N
        self.F, self.B = projector_matrices(oracle, theta, N)
        self.A = self.F.shape[0] // N
        mask, meas = np.asarray(mask, np.float32).reshape(-1, self.A), np.asarray(meas, np.float32).reshape(-1, self.A, N)
        self.mask, self.meas = np.repeat(mask, chains_per_object, 0), np.repeat(meas, chains_per_object, 0)     # per chain
        self.pnm = np.float32(pnm)
        self.logw, self.alpha, self.lbeta = prior_tables(weights, alpha)

    def _lik(self, proj, dtype):
        if dtype == np.float32:
            return tp.twin_logp(proj, self.mask, self.meas, self.pnm), tp.twin_dlogp(proj, self.mask, self.meas, self.pnm)
        m, x, pnm = self.mask.astype(dtype)[..., None], self.meas.astype(dtype), dtype(self.pnm)
        with np.errstate(all="ignore"):
            lam, k = proj * m * pnm, x * pnm
            lp = np.where(k == 0, 0.0, k * np.log(lam)) - gammaln(k + 1.0) - lam
            return lp, np.where(k == 0, -m * pnm, m * pnm * (k - lam) / lam)

    def bijector(self, x):
        """x [C][K-1] -> dict of z, 1 - z, log z, log(1 - z), log r [C][K], log O, O [C][K]."""
        dt, K = x.dtype.type, self.K
        c = np.log(np.arange(K - 1, 0, -1).astype(dt))
        t = x - c
        with np.errstate(all="ignore"):
            e = np.exp(-np.abs(t))
            lg = np.log1p(e)
            inv = dt(1.0) / (dt(1.0) + e)
            z, omz = np.where(t >= 0, inv, e * inv), np.where(t >= 0, e * inv, inv)
            lz, l1mz = -(np.maximum(-t, dt(0.0)) + lg), -(np.maximum(t, dt(0.0)) + lg)
            zero = np.zeros((x.shape[0], 1), dt)
            logr = np.concatenate([zero, np.cumsum(l1mz, axis=1, dtype=dt)], axis=1)
            logO = np.concatenate([lz, zero], axis=1) + logr
            return dict(z=z, omz=omz, lz=lz, l1mz=l1mz, logr=logr, logO=logO, O=np.exp(logO))

    def inverse(self, O, dtype):
        """The inverse bijector as the kernel's init takes it: x_k = (log O_k - log sum_{j>k} O_j) + log(K-1-k)."""
        O = np.asarray(O, np.float32).astype(dtype)
        above = np.cumsum(O[:, ::-1], axis=1, dtype=dtype)[:, ::-1][:, 1:]
        return ((np.log(O[:, :-1]) - np.log(above)) + np.log(np.arange(self.K - 1, 0, -1).astype(dtype))).astype(dtype)

    def target(self, x, with_w=False):
        """(T [C], dT/dx [C][K-1], O [C][K]) in x's dtype; with_w: and w [C][K] = O dT/dO, 0 where the clamp binds."""
        dt, K = x.dtype.type, self.K
        b = self.bijector(x)
        with np.errstate(all="ignore"):
            bind = b["O"] < dt(TINY)
            Oc, logOc = np.where(bind, dt(TINY), b["O"]), np.where(bind, np.log(dt(TINY)), b["logO"])
            proj = (Oc @ self.F.T.astype(dt)).reshape(-1, self.A, self.N)
            lp, g = self._lik(proj, dt)
            G = g.astype(dt).reshape(-1, self.A * self.N) @ self.B.T.astype(dt)
            am1 = self.alpha.astype(dt) - dt(1.0)                                                   # [M][K]
            am = (self.logw.astype(dt) + (logOc[:, None, :] * am1[None]).sum(-1, dtype=dt)) - self.lbeta.astype(dt)
            mx = am.max(-1, keepdims=True)
            pe = np.exp(am - mx)
            den = pe.sum(-1, keepdims=True, dtype=dt)
            prior = (mx + np.log(den))[:, 0]
            w = np.where(bind, dt(0.0), Oc * G + (pe / den) @ am1)
            above = np.cumsum(w[:, ::-1], axis=1, dtype=dt)[:, ::-1][:, 1:]                           # sum_{k>j} w_k, j < K-1
            kmj = (K - np.arange(K - 1)).astype(dt)
            grad = (w[:, :-1] * b["omz"] - b["z"] * above) + (dt(1.0) - kmj * b["z"])
            fldj = ((b["lz"] + b["l1mz"]) + b["logr"][:, :-1]).sum(-1, dtype=dt)
            T = (prior + lp.astype(dt).sum((1, 2), dtype=dt)) + fldj
        assert T.dtype == dt and grad.dtype == dt
        return (T, grad, b["O"], w) if with_w else (T, grad, b["O"])


LOG_TARGET = np.float32(np.log(0.75))


def adapt(eps, lar):
    """One step of the step-size rule, float32 on float32 (the kernel's two operations)."""
    eps, lar = np.asarray(eps, np.float32), np.asarray(lar, np.float32)
    with np.errstate(invalid="ignore"):
        up = (lar == lar) & (np.minimum(lar, np.float32(0.0)) > LOG_TARGET)
    return np.where(up, eps * np.float32(1.01), eps / np.float32(1.01)).astype(np.float32)


def run(model, x, eps, chain_ids, seed, n_steps, L, num_adaptation_steps=0, t0=0):
    """n_steps transitions from x [C][K-1] with step sizes eps [C] (float32 values).  Returns a dict of per-step arrays: samples
    [n][C][K], proposal [n][C][K], lar, acc, target, logu [n][C], and the final eps [C] and x."""
    dt = x.dtype.type
    eps = np.asarray(eps, np.float32).copy()
    T, g, O = model.target(x)
    out = dict(samples=[], proposal=[], lar=[], acc=[], target=[], logu=[])
    for t in range(t0, t0 + n_steps):
        mom, logu = draws(seed, chain_ids, t, model.K, dt)
        e = eps.astype(dt)[:, None]
        half = dt(0.5) * e
        kin0 = dt(0.5) * (mom * mom).sum(-1, dtype=dt)
        mom = mom + half * g
        xn = x
        for l in range(L):
            xn = xn + e * mom
            Tn, gn, On = model.target(xn)
            mom = mom + (half if l == L - 1 else e) * gn
        kin1 = dt(0.5) * (mom * mom).sum(-1, dtype=dt)
        with np.errstate(invalid="ignore"):
            lar = (Tn - kin1) - (T - kin0)
            acc = logu < lar
        a = acc[:, None]
        x, g, O, T = np.where(a, xn, x), np.where(a, gn, g), np.where(a, On, O), np.where(acc, Tn, T)
        if t < num_adaptation_steps:
            eps = adapt(eps, lar.astype(np.float32))
        for key, v in (("samples", O), ("proposal", On), ("lar", lar), ("acc", acc), ("target", T), ("logu", logu)):
            out[key].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out["eps"], out["x"] = eps, x
    return out


# ---- the tests' problems and their acceptance rule ---------------------------------------------------------------
# name -> (N, A).  n4, n6, n7: K - 1 = 15 ends the active lanes exactly on a 16-lane DPP row; K = 36 and 49 end them inside rows 2
# and 3, where the scans' row_bcast:15 / row_bcast:31 steps decide the result.
SHAPES = {"toy": (2, 2), "n3": (3, 5), "n5": (5, 7), "n8": (8, 20), "n4": (4, 16), "n6": (6, 11), "n7": (7, 9)}
# chosen so that twin32 against twin64 stays under the caps
SEEDS = {"toy": 11, "n3": 12, "n5": 13, "n8": 14, "n4": 16, "n6": 17, "n7": 18}
# Step sizes of the comparisons: the toy's is the reference's 6.5e-2.  On the larger objects (a sharper posterior: more rays at
# pnm = 1e3) that size makes the leapfrog integrator diverge from the random starts (log accept ratios down to -4e5, 67 % of the
# chains of n5 left out after 20 steps in twin32 against twin64 alone): a bar taken from the largest value then says nothing.
# 1e-2 keeps the trajectories stable (|lar| < 300, acceptance 40-75 %), which is where a sampler is used.
STEP = {"toy": 6.5e-2, "n3": 1e-2, "n5": 1e-2, "n8": 1e-2, "n4": 1e-2, "n6": 1e-2, "n7": 1e-2}
# The documented extremes at once, outside SHAPES (the issue's cases): 8 x 8 pixels, 256 angles (32 passes over the sinogram, the
# largest LDS request), 4 mixture components, and 32 leapfrog steps per transition.
EXTREME = {"max": (8, 256)}
EXTREME_L = 32
SEEDS["max"], STEP["max"] = 15, 2e-3


def problem(oracle, name, seed=0):
    """theta, mask [1][A], meas [1][A][N], pnm, prior: Poisson measurements (the oracle's sampler) of a random simplex object's
    sinogram at pnm = 1e3; the second angle is masked out (mask = 0, measurement = 0)."""
    N, A = SHAPES[name] if name in SHAPES else EXTREME[name]
    rng = np.random.default_rng(1000 + seed + 17 * N + A // 256)
    theta = np.array([0.0, np.pi / 2], np.float32) if name == "toy" else (0.3 + 0.6 * np.arange(A)).astype(np.float32)
    obj = rng.dirichlet(np.full(N * N, 2.0)).astype(np.float32).reshape(1, N, N)
    sino = oracle.rotate_fwd(obj, oracle.Geometry(N, N, False), oracle.rotate_transforms(theta, N, N))
    mask = np.where(np.arange(A) % 2 == 0, 1.0, 0.5).astype(np.float32)[None]
    if A > 2:
        mask[0, 1] = 0.0
    meas = oracle.poisson_measure(sino, mask, 1e3, 5 + seed)
    if name == "toy":
        prior = (np.array([0.3, 0.7]), np.array([[0.35580334, 0.94963009, 0.60227688, 0.43061459],
                                                 [0.00390356, 0.44335424, 0.83152378, 0.52733124]]))
    elif name in EXTREME:
        prior = (np.array([0.1, 0.2, 0.3, 0.4]), rng.uniform(0.5, 2.0, (4, N * N)))
    else:
        prior = (np.array([0.4, 0.6]), rng.uniform(0.5, 2.0, (2, N * N)))
    return dict(N=N, A=A, theta=theta, mask=mask, meas=meas, pnm=1e3, prior=prior, obj=obj)


def random_starts(name, C, seed=0):
    N = (SHAPES[name] if name in SHAPES else EXTREME[name])[0]
    return np.random.default_rng(2000 + seed).dirichlet(np.full(N * N, 3.0), C).astype(np.float32)


def bar(t32, t64, sel):
    """max(1e-5 scale, 8 max |twin32 - twin64|) over the selected chains (np_twin_poisson.bar_from_twin's way: the bar comes from
    the restatement's own float32 error on the same inputs; 8 covers the device's logf / expf / cosf and its order of sums)."""
    if not sel.any():
        return 0.0
    a, b = np.asarray(t32, np.float64)[sel], np.asarray(t64, np.float64)[sel]
    return max(1e-5 * float(np.abs(b).max()), 8.0 * float(np.abs(a - b).max()))


def check_against_twin(t32, t64, got=None):
    """Step by step along a trajectory: a chain is compared while none of its earlier decisions was LEFT OUT, i.e. closer to the
    accept threshold than the bar of the log accept ratio (|lar64 - log u| < bar).  Compared: log_accept_ratio on every such
    chain; the decision, the sample (the proposal where accepted) and target_log_prob on those whose decision of this step is not
    left out either.  Returns (fraction of chains left out by the end, worst error / bar seen per quantity); asserts when `got`
    (dict of samples [n][C][K], lar, acc, target [n][C]) is given."""
    n, C = t64["lar"].shape
    alive = np.ones(C, bool)
    worst = dict(lar=0.0, samples=0.0, target=0.0)
    for s in range(n):
        b_lar = bar(t32["lar"][s], t64["lar"][s], alive)
        with np.errstate(invalid="ignore"):
            near = ~(np.abs(t64["lar"][s].astype(np.float64) - t64["logu"][s]) >= b_lar)       # (a NaN ratio is left out too)
        keep = alive & ~near
        assert np.array_equal(t32["acc"][s][keep], t64["acc"][s][keep])
        b_smp = bar(t32["samples"][s], t64["samples"][s], keep)
        b_tgt = bar(t32["target"][s], t64["target"][s], keep)
        if got is not None:
            e = np.abs(got["lar"][s].astype(np.float64) - t64["lar"][s])[alive]
            worst["lar"] = max(worst["lar"], float(e.max() / b_lar) if alive.any() else 0.0)
            assert np.all(e <= b_lar), (s, "log_accept_ratio", float(e.max()), b_lar)
            if keep.any():
                assert np.array_equal(got["acc"][s][keep], t64["acc"][s][keep]), (s, "is_accepted")
                e = np.abs(got["samples"][s].astype(np.float64) - t64["samples"][s])[keep]
                worst["samples"] = max(worst["samples"], float(e.max() / b_smp))
                assert np.all(e <= b_smp), (s, "sample", float(e.max()), b_smp)
                e = np.abs(got["target"][s].astype(np.float64) - t64["target"][s])[keep]
                worst["target"] = max(worst["target"], float(e.max() / b_tgt))
                assert np.all(e <= b_tgt), (s, "target_log_prob", float(e.max()), b_tgt)
        alive = keep
    return 1.0 - alive.mean(), worst


def twin_runs(oracle, name, C, n_steps, seed, L=5):
    """The float32 and float64 restatements of hmc_sample(meas, mask, ..., initial_state=random_starts, num_adaptation_steps=0) on
    the problem `name`: (problem, starts, twin32, twin64)."""
    pb = problem(oracle, name)
    model = Model(oracle, pb["theta"], pb["N"], pb["mask"], pb["meas"], pb["pnm"], *pb["prior"], chains_per_object=C)
    starts = random_starts(name, C)
    eps = np.full(C, STEP[name], np.float32)
    runs = [run(model, model.inverse(starts, dt), eps, np.arange(C), seed, n_steps, L) for dt in (np.float32, np.float64)]
    return pb, starts, runs[0], runs[1]


# ---- the evaluator alone: T and dT/dx of the chain state that ctpvae_hmc_init_f32 stores ---------------------------
TIE_ANGLES = np.array([0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, -np.pi / 2, 0.3, 1.1])
TARGET_PNM = 1e3
BAND = (1e-39, 1e-37)      # O around FLT_MIN = 1.18e-38: float32 and float64 may decide the clamp differently there


def target_cases():
    """(N, A, M, seed): every N; one angle, a few, more than the tie angles, and ceil(64 / N) angles -- A N = 64 exactly (one full
    pass: N = 2, 4, 8) or 65 .. 70 (a second pass with 1 .. 6 live entries: N = 5, 3, 6, 7); every M = 1 .. 4 occurs."""
    for N in range(2, 9):
        for A in sorted({1, 3, 11, -(-64 // N)}):
            yield N, A, 1 + (N + A) % 4, 100 * N + A


def target_case(oracle, N, A, M, seed, C=64):
    """(model, theta, mask [1][A], meas [1][A][N], prior, starts [C][K]).  The angles include the rounding ties of the tap tables
    (multiples of pi / 4); chains 0 .. C/2 - 1 start with one denormal pixel (1e-44 .. 1e-40, far below FLT_MIN, where the clamp
    O' = max(O, FLT_MIN) binds), chains C/2 .. C - 1 inside the simplex."""
    K = N * N
    rng = np.random.default_rng(seed)
    theta = np.resize(TIE_ANGLES, A).astype(np.float32)
    obj = rng.dirichlet(np.full(K, 2.0)).astype(np.float32).reshape(1, N, N)
    sino = oracle.rotate_fwd(obj, oracle.Geometry(N, N, False), oracle.rotate_transforms(theta, N, N))
    mask = np.where(np.arange(A) % 2 == 0, 1.0, 0.5).astype(np.float32)[None]
    if A > 2:
        mask[0, 1] = 0.0
    meas = oracle.poisson_measure(sino, mask, TARGET_PNM, 5)
    prior = (np.full(M, 1.0 / M), rng.uniform(0.5, 2.0, (M, K)))
    starts = rng.dirichlet(np.full(K, 3.0), C).astype(np.float32)
    for c in range(C // 2):
        starts[c, rng.integers(K)] = np.float32(10.0 ** -rng.uniform(40, 44))
    model = Model(oracle, theta, N, mask, meas, TARGET_PNM, *prior, chains_per_object=C)
    return model, theta, mask, meas, prior, starts


def _chain_bar(v32, v64):
    """bar()'s rule per chain: max(1e-5 max_k |v64[c]|, 8 max_k |v32[c] - v64[c]|), [C]."""
    v32, v64 = np.asarray(v32, np.float64).reshape(len(v64), -1), np.asarray(v64, np.float64).reshape(len(v64), -1)
    with np.errstate(invalid="ignore"):
        return np.maximum(1e-5 * np.abs(v64).max(-1), 8.0 * np.abs(v32 - v64).max(-1))


def check_target(model, starts, x_dev, g_dev=None, T_dev=None):
    """The evaluator at the device's own point: x_dev [C][K-1] float32 (the device's inverse bijector of `starts`), g_dev [C][K-1]
    and T_dev [C] what it stored for it.  Reference: Model.target(x_dev) in float64; bars: bar()'s factor 8 over the float32
    restatement and its 1e-5 floor, PER CHAIN (boundary and interior chains differ by orders of magnitude).  x_dev itself is held
    to Model.inverse(starts) on every chain in the same way.  A chain is left out of the T and dT/dx comparison when the float32
    restatement is not finite there, when max |g64| >= 1e30 (a ray whose only taps are bound pixels: the float32 formula itself
    overflows, in the reference too), or when some O64 lies in BAND.  T alone, which does not overflow there (log of FLT_MIN pnm
    is finite), is ALSO compared on the left-out chains whose float32 T is finite and that are outside BAND: those are the only
    chains on which the VALUE the clamp puts into the projection shows (elsewhere a bound pixel shares every ray with larger
    ones).  Returns (chains left out, compared chains with a bound pixel, chains in BAND, worst error / bar per quantity); asserts
    when g_dev and T_dev are given."""
    x_dev = np.asarray(x_dev)
    assert x_dev.dtype == np.float32
    with np.errstate(all="ignore"):
        T64, g64, O64 = model.target(x_dev.astype(np.float64))
        T32, g32, _ = model.target(x_dev)
        if starts is None:                                                                      # the default start: x = 0
            x64, x32 = np.zeros(x_dev.shape), np.zeros(x_dev.shape, np.float32)
        else:
            x64, x32 = model.inverse(starts, np.float64), model.inverse(starts, np.float32)
        band = ((O64 >= BAND[0]) & (O64 <= BAND[1])).any(-1)
        out = ~(np.isfinite(g32).all(-1) & np.isfinite(T32)) | ~(np.abs(g64).max(-1) < 1e30) | band
    keep = ~out
    keep_T = keep | (np.isfinite(T32) & ~band)
    bound = int(((O64 < TINY).any(-1) & keep).sum())
    worst = dict(x=0.0, g=0.0, T=0.0)
    if g_dev is not None:
        with np.errstate(all="ignore"):
            b_x, b_g, b_T = _chain_bar(x32, x64), _chain_bar(g32, g64), _chain_bar(T32, T64)
            e_x = np.abs(x_dev.astype(np.float64) - x64).max(-1)
            e_g = np.abs(np.asarray(g_dev, np.float64) - g64).max(-1)
            e_T = np.abs(np.asarray(T_dev, np.float64) - T64)
        for name, e, b, sel in (("x", e_x, b_x, np.ones_like(keep)), ("g", e_g, b_g, keep), ("T", e_T, b_T, keep_T)):
            if sel.any():
                with np.errstate(all="ignore"):
                    ratio = np.where(e[sel] == 0.0, 0.0, e[sel] / b[sel])
                bad = ~(e[sel] <= b[sel])                                                      # (a NaN fails)
                worst[name] = float(ratio.max())
                c = int(np.flatnonzero(sel)[np.argmax(bad)])
                assert not bad.any(), (name, "chain", c, float(e[c]), float(b[c]), int(bad.sum()))
    return int(out.sum()), bound, int(band.sum()), worst
