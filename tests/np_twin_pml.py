"""numpy restatement of recon(algorithm='pml_quad' | 'pml_hybrid' | 'ospml_quad' | 'ospml_hybrid') (ct_pvae_amd/recon.py _pml;
libtomo pml_quad.c / pml_hybrid.c / ospml_quad.c / ospml_hybrid.c [3P-recalled: TomoPy 1.11.0], the recollection checked by
re-deriving the update as De Pierro's separable surrogate of  loglik(x) - beta * penalty(x)), composed from the oracle's projector
pair as tests/np_twin_mlem.py is.  Per iteration and block b, on the grid [gx][gy] with c = (i, j):

    sim   = A_b x ;  ratio = data_b / sim where sim != 0 else 0          (float32, mlem's guarded ratio)
    u     = A_b^T ratio                                                  (float32, libtomo's order of terms)
    E     = -(x[c] * u[c])
    F = 0 ; P = 0 ; for q in NEIGHBOURS, skipping neighbours outside the grid:
            r   = x[c] - x[k_q]
            gam = 1 (quad)   or   1 / (1 + fabs(r / delta)) (hybrid)
            t   = ((2 * beta) * w_q) * gam                               (quad: (2 * beta) * w_q)
            F  += t ;  P -= t * (x[c] + x[k_q])
    G     = P + sum_dist_b[c]                                            sum_dist_b = A_b^T 1
    S     = sqrt(G * G - (8 * E) * F)
    x_new = (-2 * E) / (G + S)      where G > 0                          rule="stable": the build's, free of cancellation
          = (-G + S) / (4 * F)      where G <= 0 and F != 0              rule="libtomo": this form everywhere F != 0
          = x                       where G <= 0 and F == 0              (beta == 0 and no ray of the block crosses the pixel)

All neighbour reads come from the iterate the block started with.  Weights: direct neighbours a, diagonal ones a / sqrt(2), a = 1 /
(n_direct + n_diag / sqrt(2)) over the neighbours that exist -- libtomo's three tables as float32 literals (W_TABLES).  `dtype` is
the type of x and of the arithmetic from E on; the projector pair and the ratio are float32 in both (x is rounded for them), and
beta, delta and the weights are float32 values in both, so a float64 run differs from a float32 one by the rounding of the update
alone."""
import numpy as np

from oracle import radon_oracle as orc
from tests.np_twin_mlem import blocks_of

F = np.float32

NEIGHBOURS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
# neighbours that exist -> (direct, diagonal): interior, edge, corner
W_TABLES = {8: (F(0.1464466094), F(0.1035533906)), 5: (F(0.2265409197), F(0.1601886205)), 3: (F(0.3693980625), F(0.2612038750))}


def weights(gx, gy):
    """w [8][gx][gy] float32 in NEIGHBOURS' order, 0 where the neighbour lies outside the grid (gx, gy >= 2)."""
    if gx < 2 or gy < 2:
        raise ValueError("the penalty needs a grid of at least 2 x 2")
    i, j = np.meshgrid(np.arange(gx), np.arange(gy), indexing="ij")
    exists = np.stack([(i + di >= 0) & (i + di < gx) & (j + dj >= 0) & (j + dj < gy) for di, dj in NEIGHBOURS])
    n = exists.sum(0)
    w = np.zeros((8, gx, gy), F)
    for q, (di, dj) in enumerate(NEIGHBOURS):
        for cnt, tab in W_TABLES.items():
            w[q][exists[q] & (n == cnt)] = tab[0 if di == 0 or dj == 0 else 1]
    return w


def neighbour(x, di, dj):
    """x[..., i + di, j + dj], 0 outside."""
    gx, gy = x.shape[-2:]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)])
    return xp[..., 1 + di:1 + di + gx, 1 + dj:1 + dj + gy]


def update(x, u, sum_dist, beta, delta=1.0, hybrid=False, rule="stable", dtype=F, w=None):
    """The store: x, u [oy][gx][gy], sum_dist [gx][gy] -> x_new, every operation in `dtype` in the order of the module docstring."""
    T = dtype
    x, u, sum_dist = np.asarray(x, T), np.asarray(u, T), np.asarray(sum_dist, T)
    w = weights(*x.shape[-2:]) if w is None else w
    two_beta, dl = T(2) * T(F(beta)), T(F(delta))
    with np.errstate(all="ignore"):
        E = -(x * u)
        Fs, P = np.zeros_like(x), np.zeros_like(x)
        for q, (di, dj) in enumerate(NEIGHBOURS):
            xk, wq = neighbour(x, di, dj), w[q].astype(T)
            t = two_beta * wq                                  # 0 where the neighbour is outside: F and P keep their bits
            if hybrid:
                t = t * (T(1) / (T(1) + np.abs((x - xk) / dl)))
            t = np.broadcast_to(t, x.shape)
            Fs = Fs + t
            P = P - t * (x + xk)
        G = P + sum_dist
        S = np.sqrt(G * G - (T(8) * E) * Fs)
        lib = np.where(Fs != 0, (-G + S) / (T(4) * Fs), x)
        out = lib if rule == "libtomo" else np.where(G > 0, (T(-2) * E) / (G + S), lib)
    assert out.dtype == T
    return out


def pml(data, theta, num_iter=1, beta=1.0, delta=1.0, hybrid=False, init=1e-6, ngridx=None, ngridy=None, num_block=1, ind_block=None,
        rule="stable", dtype=F, each=None):
    """data [oy][dt][dx] -> [oy][gx][gy] in `dtype`.  each(it, x): called with every finished iterate (it = 1 .. num_iter)."""
    data, theta = np.ascontiguousarray(data, F), np.ascontiguousarray(theta, F)
    oy, dt, dx = data.shape
    gx, gy = int(ngridx or dx), int(ngridy or dx)
    x = np.full((oy, gx, gy), init, dtype) if np.isscalar(init) else np.ascontiguousarray(init, dtype).copy()
    w = weights(gx, gy)
    geo = []
    for blk in blocks_of(dt, num_block, ind_block):
        th = np.ascontiguousarray(theta[blk])
        geo.append((th, np.ascontiguousarray(data[:, blk]), orc.siddon_backproject(np.ones((1, blk.size, dx), F), th, gx, gy)[0]))
    for it in range(1, int(num_iter) + 1):
        for th, meas, sum_dist in geo:
            sim = orc._project_grid(x.astype(F), th, dx)
            with np.errstate(all="ignore"):
                ratio = np.where(sim != 0, meas / sim, F(0.0)).astype(F)
            x = update(x, orc.siddon_backproject(ratio, th, gx, gy), sum_dist, beta, delta, hybrid, rule, dtype, w)
        if each is not None:
            each(it, x)
    return x


def penalty(x):
    """1/2 sum_c sum_q w_q (x[c] - x[k_q])^2 over the neighbours that exist, in float64."""
    x = np.asarray(x, np.float64)
    w = weights(*x.shape[-2:]).astype(np.float64)
    return 0.5 * float(sum((w[q] * (x - neighbour(x, di, dj)) ** 2).sum() for q, (di, dj) in enumerate(NEIGHBOURS)))
