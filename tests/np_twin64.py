"""numpy restatement of the two float64 backwards of the rotate projector (ctpvae_rotate_bwd_f64), on tables from
oracle.rotate_transforms / oracle.invert_transforms.  Coordinates and weights are np.float32 (unfused: numpy rounds every
operation); taps, products and sums are in `acc` (np.float64 for the float64 backwards).  With acc=np.float32 the same code
states the fp32 rules of oracle.rotate_bwd_tfcompat / oracle.rotate_bwd_exact, term for term.

  bwd_tfcompat: TensorFlow's gradient -- the cotangent row broadcast over the canvas rows, sampled with the inverted rows,
                summed over angles in ascending order, cropped to the slice.
  bwd_exact:    the transpose of oracle.rotate_fwd_f64 as a scatter in (angle, canvas row, bin, tap) order (np.add.at
                adds in index order); a term is ((double)wy * (double)wx) * g -- in fp32 mode wy * (wx * g), the oracle's."""
import numpy as np

from tests.np_twin import round_half_away

f32 = np.float32


def angle_set(A, rng):
    """A angles: multiples of pi/4 first (where the coordinates meet rounding ties), then uniform ones."""
    quarter = np.arange(8) * (np.pi / 4)
    return np.concatenate([quarter[:A], rng.uniform(0.0, 2 * np.pi, max(0, A - 8))])


def tables(theta, geom):
    """(T8, Tinv8) of oracle.rotate_transforms / oracle.invert_transforms for the canvas of `geom` (an oracle.Geometry)."""
    from oracle import radon_oracle as orc
    T = orc.rotate_transforms(np.asarray(theta, f32), geom.PH, geom.PW)
    return T, orc.invert_transforms(T)


def _bcast_read(grow, PH, PW, iy, ix):
    """grow [S][PW]: the cotangent row of every slice, broadcast over the PH canvas rows; zero outside the canvas."""
    ok = (iy >= 0) & (iy < PH) & (ix >= 0) & (ix < PW)
    return np.where(ok, grow[:, np.clip(ix, 0, PW - 1)], grow.dtype.type(0))


def bwd_tfcompat(gsino, geom, Tinv8, interp, acc=np.float64):
    """gsino [S][A][PW] -> [S][H][W]."""
    gsino = np.asarray(gsino).astype(acc)
    Tinv8 = np.asarray(Tinv8, f32)
    S, A = gsino.shape[:2]
    r, c = np.meshgrid(np.arange(geom.H), np.arange(geom.W), indexing="ij")
    fx, fy = (c + geom.px).astype(f32), (r + geom.py).astype(f32)
    out = np.zeros((S, geom.H, geom.W), acc)
    for a in range(A):
        t = Tinv8[a]
        x = (t[0] * fx + t[1] * fy) + t[2]
        y = (t[3] * fx + t[4] * fy) + t[5]
        grow = gsino[:, a, :]

        def rd(iy, ix):
            return _bcast_read(grow, geom.PH, geom.PW, iy.astype(np.int64), ix.astype(np.int64))

        if interp == 0:
            v = rd(round_half_away(y), round_half_away(x))
        else:
            yf, xf = np.floor(y), np.floor(x)
            yc, xc = yf + f32(1), xf + f32(1)
            wx0, wx1 = (xc - x).astype(acc), (x - xf).astype(acc)
            v_yf = wx0 * rd(yf, xf) + wx1 * rd(yf, xc)
            v_yc = wx0 * rd(yc, xf) + wx1 * rd(yc, xc)
            v = (yc - y).astype(acc) * v_yf + (y - yf).astype(acc) * v_yc
        out = out + v
    return out


def bwd_exact(gsino, geom, T8, interp, acc=np.float64):
    """gsino [S][A][PW] -> [S][H][W]."""
    gsino = np.asarray(gsino).astype(acc)
    T8 = np.asarray(T8, f32)
    S, A = gsino.shape[:2]
    H, W, HW = geom.H, geom.W, geom.H * geom.W
    i, j = np.meshgrid(np.arange(geom.PH), np.arange(geom.PW), indexing="ij")
    fi, fj = i.astype(f32), j.astype(f32)
    out = np.zeros(S * HW, acc)
    srow = (np.arange(S) * HW)[:, None, None, None]
    for a in range(A):
        t = T8[a]
        x = (t[0] * fj + t[1] * fi) + t[2]
        y = (t[3] * fj + t[4] * fi) + t[5]
        g = gsino[:, a, :][:, None, :, None]                      # [S][1][PW][1]: the bin's cotangent on every row
        if interp == 0:
            iy, ix = round_half_away(y)[..., None], round_half_away(x)[..., None]
            terms = np.broadcast_to(g, (S, geom.PH, geom.PW, 1))
        else:
            yf, xf = np.floor(y), np.floor(x)
            yc, xc = yf + f32(1), xf + f32(1)
            iy = np.stack([yf, yf, yc, yc], -1)
            ix = np.stack([xf, xc, xf, xc], -1)
            wy = np.stack([yc - y, yc - y, y - yf, y - yf], -1)
            wx = np.stack([xc - x, x - xf, xc - x, x - xf], -1)
            if acc is np.float32:
                terms = wy * (wx * g)
            else:
                terms = (wy.astype(acc) * wx.astype(acc)) * g
        rr = iy.astype(np.int64) - geom.py
        cc = ix.astype(np.int64) - geom.px
        ok = np.broadcast_to((rr >= 0) & (rr < H) & (cc >= 0) & (cc < W), terms.shape)
        idx = np.broadcast_to(srow + rr * W + cc, terms.shape)    # [S][PH][PW][tap]: C order = (slice, row, bin, tap)
        np.add.at(out, idx[ok], np.asarray(terms, acc)[ok])
    return out.reshape(S, H, W)
