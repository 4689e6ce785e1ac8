"""numpy restatement of csrc/convblock.hip: the periodic pad by index arrays, its backward by the two ascending float32 folds the
file header states, the maxout and its backward by np.where.  tests/test_convblock_cpu.py holds it to the trainer's _PeriodicPad
and _Maxout on the CPU (torch's CPU index_add_ adds in ascending order); tests/test_gpu_convblock.py holds the kernels to it."""
import numpy as np

#            [N, C, H, W]       (wl, wr, hl, hr)
PAD_CASES = [((1, 1, 1, 1), (2, 1, 2, 1)),        # every output is one element; four copies per axis
             ((2, 2, 2, 3), (2, 1, 2, 1)),        # wraps twice on one axis
             ((1, 2, 1, 9), (2, 1, 2, 1)),        # one axis wraps, the other does not
             ((2, 3, 5, 7), (2, 1, 1, 1)),        # odd extents, asymmetric pads
             ((3, 2, 16, 16), (1, 1, 1, 1)),      # aligned rows, the stride-2 case
             ((2, 1, 130, 67), (2, 1, 1, 1)),     # several workgroups, ragged vector tails
             ((2, 2, 8, 8), (0, 0, 0, 0))]        # a copy
MAXOUT_SHAPES = [(2, 6, 3, 5), (1, 2, 1, 1), (3, 4, 16, 16), (2, 2, 130, 67)]      # y [N][2C][H][W]


def pad_id(case):
    return "x".join(map(str, case[0])) + "+" + ".".join(map(str, case[1]))


def shape_id(shape):
    return "x".join(map(str, shape))


def at_most_two_copies(shape, pads):
    """Every source element has at most two copies per axis: the pads of an axis together do not exceed its extent.  Then a
    backward sum has at most two terms per axis and does not depend on the order of addition."""
    wl, wr, hl, hr = pads
    return wl + wr <= shape[3] and hl + hr <= shape[2]


def pad_index(n, lo, hi):
    return np.arange(-lo, n + hi) % n


def pad_fwd(x, pads):
    wl, wr, hl, hr = pads
    return np.ascontiguousarray(x[:, :, pad_index(x.shape[2], hl, hr)][:, :, :, pad_index(x.shape[3], wl, wr)])


def _fold(g, axis, index, n):
    """out[.., j, ..] = the float32 sum of g[.., k, ..] over k ASCENDING with index[k] = j, starting from its first term."""
    g = np.moveaxis(np.asarray(g, np.float32), axis, -1)
    out = np.zeros(g.shape[:-1] + (n,), np.float32)
    seen = np.zeros(n, bool)
    for k, j in enumerate(index):
        out[..., j] = g[..., k] if not seen[j] else out[..., j] + g[..., k]
        seen[j] = True
    assert seen.all()
    return np.moveaxis(out, -1, axis)


def pad_bwd(g, hw, pads):
    """gx [N][C][H][W] of the cotangent g [N][C][OH][OW]: columns folded per padded row (q ascending), then rows (r ascending)."""
    H, W = hw
    wl, wr, hl, hr = pads
    t = _fold(g, 3, pad_index(W, wl, wr), W)
    return np.ascontiguousarray(_fold(t, 2, pad_index(H, hl, hr), H))


def maxout_fwd(y):
    """(out, first): first = a >= b (False where either is NaN), out = first ? a : b."""
    c = y.shape[1] // 2
    a, b = y[:, :c], y[:, c:]
    with np.errstate(invalid="ignore"):
        first = a >= b
    return np.where(first, a, b).astype(np.float32), first


def maxout_bwd(g, first):
    g = np.asarray(g, np.float32)
    zero = np.zeros_like(g)
    return np.concatenate([np.where(first, g, zero), np.where(first, zero, g)], axis=1)


def planted_maxout():
    """y [1][2][1][8]: a tie, a NaN in the first half only, a NaN in the second half only, (-0, +0), (+0, -0), (inf, inf), (-inf, 1)
    and an ordinary pair; and which half each takes."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = np.array([1.5, nan, 2.0, -0.0, 0.0, inf, -inf, 3.0], np.float32)
    b = np.array([1.5, 2.0, nan, 0.0, -0.0, inf, 1.0, 4.0], np.float32)
    first = np.array([True, False, False, True, True, True, False, False])
    return np.stack([a, b]).reshape(1, 2, 1, 8), first.reshape(1, 1, 1, 8)
