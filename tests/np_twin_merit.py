"""float64 numpy restatement of csrc/merit.hip: (MSE, SSIM, PSNR) of an image pair with direct window sums, every sum in the order the
file's header states (ST(v, w): thread u adds v[u], v[u + w], ... ascending from 0, then log2(w) halving steps).  Elements that do not
exist are added as 0.0 here and skipped on the device: x + 0.0 == x for every x (the sign of a zero apart, which no comparison sees)."""
import numpy as np

TILE = 32           # kMeritTile
CHUNK = 4096        # kMeritChunk
THREADS = 256       # kMeritThreads
FINISH_THREADS = 64


def win_size(X, Y):
    m = min(X, Y)
    return 7 if m >= 7 else (m if m % 2 else m - 1)


def shape(X, Y):
    """(win, Xo, Yo, tile rows, tile columns, chunks)."""
    win = win_size(X, Y)
    Xo, Yo = X - win + 1, Y - win + 1
    return win, Xo, Yo, -(-Xo // TILE), -(-Yo // TILE), -(-(X * Y) // CHUNK)


def workspace_bytes(n, X, Y):
    _, _, _, tr, tc, chunks = shape(X, Y)
    return n * (3 * chunks + tr * tc) * 8


def st(v, w):
    """ST(v, w) of csrc/merit.hip."""
    v = np.asarray(v, np.float64).ravel()
    rows = -(-v.size // w)
    pad = np.zeros(rows * w, np.float64)
    pad[:v.size] = v
    p = np.zeros(w, np.float64)
    for row in pad.reshape(rows, w):
        p = p + row
    while p.size > 1:
        h = p.size // 2
        p = p[:h] + p[h:]
    return p[0]


def _window_sums(q, win, Xo, Yo):
    """W(q) at every position: each row's sum with its columns ascending, then the rows ascending."""
    row = q[:, 0:Yo].copy()
    for j in range(1, win):
        row = row + q[:, j:j + Yo]
    w = row[0:Xo].copy()
    for a in range(1, win):
        w = w + row[a:a + Xo]
    return w


def s_map(ref, test):
    """(S at every window position [Xo][Yo], R)."""
    r, t = np.asarray(ref, np.float64), np.asarray(test, np.float64)
    X, Y = r.shape
    win, Xo, Yo = shape(X, Y)[:3]
    R = r.max() - r.min()            # numpy's max / min keep a NaN
    NP = float(win * win)
    cov_norm = NP / (NP - 1.0)
    ux, uy = _window_sums(r, win, Xo, Yo) / NP, _window_sums(t, win, Xo, Yo) / NP
    uxx, uyy, uxy = _window_sums(r * r, win, Xo, Yo) / NP, _window_sums(t * t, win, Xo, Yo) / NP, _window_sums(r * t, win, Xo, Yo) / NP
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    a1, a2 = 0.01 * R, 0.03 * R
    c1, c2 = a1 * a1, a2 * a2
    num = ((2.0 * ux) * uy + c1) * ((2.0 * vxy) + c2)
    den = ((ux * ux + uy * uy) + c1) * ((vx + vy) + c2)
    return num / den, R


def merits(ref, test):
    """(mse, ssim, psnr) of one pair as the device computes them."""
    r, t = np.asarray(ref, np.float64), np.asarray(test, np.float64)
    if r.ndim != 2 or r.shape != t.shape or min(r.shape) < 3:
        raise ValueError(f"need two images of one shape, at least 3 x 3 (got {r.shape}, {t.shape})")
    X, Y = r.shape
    _, Xo, Yo, tr, tc, chunks = shape(X, Y)
    with np.errstate(all="ignore"):
        d = (r - t).ravel()
        d2 = d * d
        sq = st([st(d2[c * CHUNK:(c + 1) * CHUNK], THREADS) for c in range(chunks)], FINISH_THREADS)
        S, R = s_map(r, t)
        tiles = []
        for a in range(tr):
            for b in range(tc):
                tile = np.zeros((TILE, TILE), np.float64)
                blk = S[a * TILE:(a + 1) * TILE, b * TILE:(b + 1) * TILE]
                tile[:blk.shape[0], :blk.shape[1]] = blk
                tiles.append(st(tile, THREADS))
        ss = st(tiles, FINISH_THREADS)
        mse = sq / float(X * Y)
        ssim = ss / (float(Xo) * float(Yo))
        psnr = np.inf if mse == 0.0 else 10.0 * np.log10((R * R) / mse)
    return float(mse), float(ssim), float(psnr)


def batch(ref, test):
    ref, test = np.asarray(ref), np.asarray(test)
    if ref.ndim == 2:
        ref, test = ref[None], test[None]
    return np.array([merits(a, b) for a, b in zip(ref, test)], np.float64).reshape(len(ref), 3)


# ---- seeded inputs shared by tests/test_merit_cpu.py and tests/test_gpu_merit.py.  Every reference image has min 0, so max|r| = R:
# the error of S grows like (max|r| / R)^2 (c2 scales with R^2), and the tests' bars are stated for max|r| <= 2 R.
SHAPES = ((3, 4), (5, 5), (6, 40), (7, 7), (8, 9), (37, 38), (130, 67))
KINDS = ("uniform", "foam", "float32")


def seeded_pair(shape, kind, seed=0, n=None):
    """(ref, test) of `shape` (or [n] + shape): 'uniform' noise, a two-level 'foam'-like image plus noise, or 'float32' uniform noise."""
    rng = np.random.default_rng([seed, shape[0], shape[1], KINDS.index(kind)])
    full = ((1 if n is None else n),) + tuple(shape)
    if kind == "foam":
        yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        r = np.empty(full)
        for k in range(full[0]):
            cells = rng.random((shape[0] // 4 + 1, shape[1] // 4 + 1)) < 0.4
            r[k] = 0.15 + 0.6 * cells[yy // 4, xx // 4] + 0.01 * rng.standard_normal(shape)
    else:
        r = rng.random(full)
    r = r - r.min(axis=(1, 2), keepdims=True)
    t = np.clip(r + 0.05 * rng.standard_normal(full), 0.0, 1.0)
    if kind == "float32":
        r, t = r.astype(np.float32), t.astype(np.float32)
        r = r - r.min(axis=(1, 2), keepdims=True)          # exact: the minimum itself becomes 0
    return (r[0], t[0]) if n is None else (r, t)


# ---- the cases of tests/test_gpu_merit.py::test_against_twin_and_compare; tools/time_merit.py measures the same ones for its record
SEAMS = (TILE + 5, TILE + 6, TILE + 7, 2 * TILE + 1)       # win = 7: one tile short by a position, exactly one tile, one position over, two tiles + 1
GPU_SHAPES = SHAPES + ((128, 128), (40, 56), (512, 96)) + tuple((v, 9) for v in SEAMS) + tuple((9, v) for v in SEAMS) + ((TILE + 7, 2 * TILE + 1),)
GPU_N = 17


def gpu_case_inputs(shape, dtype_name):
    """(ref, test) [17][X][Y] of one case: float32 uniform noise, or float64 alternating uniform noise and the foam-like image by shape."""
    kind = "float32" if dtype_name == "float32" else ("foam" if GPU_SHAPES.index(shape) % 2 else "uniform")
    return seeded_pair(shape, kind, seed=5, n=GPU_N)
