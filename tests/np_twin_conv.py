"""numpy restatement of csrc/conv.hip: the forward chain with its tail rule and selection, the chunked weight and bias gradient, the
cotangent of the padded input with its invalid taps and the fold (tests/np_twin_convblock.pad_bwd), every fused multiply-add a
correctly rounded float32 fma; and the error bars that hold the twin (tests/test_conv_cpu.py) and the device (tests/test_gpu_conv.py) to
a float64 evaluation.  The chains are vectorised over the outputs and sequential along the sum, as the header states them."""
import numpy as np

from tests import np_twin_convblock as cb

CHUNK = 1024        # csrc/conv.hip kConvChunk, restated
U = 2.0 ** -24

#        (N, Cin, H, W, C, k, s)
CASES = [(1, 1, 1, 1, 1, 1, 1),          # everything degenerate
         (2, 3, 5, 7, 1, 3, 1),          # K = 27: the k-step tail; 2C = 2
         (1, 2, 2, 3, 3, 4, 1),          # pads of 3 wrap a 2-row image more than once
         (3, 4, 9, 10, 20, 4, 2),        # odd extent under stride 2; 2C = 40 straddles a 32-column tile
         (2, 5, 33, 65, 17, 2, 1),       # the toy recipe's kernel size; one past 32 rows and one past 64 columns
         (1, 2, 7, 8, 3, 3, 3),          # stride 3
         (1, 1, 9, 9, 2, 8, 2),          # k = 8
         (1, 40, 16, 16, 40, 4, 1),      # c3's K = 640 and 2C = 80 at a small extent
         (1, 4, 128, 128, 4, 4, 1),      # c3's row length, many chunks
         (2, 6, 12, 12, 1, 4, 1)]        # the head's 6 -> 2
CHUNK_CASES = [(1, 1, 33, 31, 1, 1, 1), (1, 1, 32, 32, 1, 1, 1), (1, 1, 25, 41, 1, 1, 1)]      # M = CHUNK - 1, CHUNK, CHUNK + 1


def case_id(case):
    return "x".join(map(str, case))


def block_pads(H, W, k, s):
    """(wl, wr, hl, hr) as ConvBlock.forward computes them."""
    pads = []
    for n in (W, H):
        p = k - (n % s if n % s else s)
        pads += [p // 2 + p % 2, p // 2]
    return tuple(pads)


def out_hw(H, W, k, s, pads):
    wl, wr, hl, hr = pads
    return (H + hl + hr - k) // s + 1, (W + wl + wr - k) // s + 1


def fma32(a, b, c):
    """The correctly rounded float32 a * b + c, elementwise: the product of two float32 is exact in float64; the float64 sum is taken
    with round-to-odd (TwoSum gives the error of the round-to-nearest sum; an inexact sum with an even last bit moves to its odd
    neighbour on the error's side), and a round-to-odd value with 29 bits to spare rounds to float32 as the exact sum does."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
        c = np.asarray(c, np.float32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def gamma(n):
    return n * U / (1.0 - n * U)


def columns(x, k, s, pads):
    """cols [N][P][K] float32: cols[n][oh * OW + ow][(ci * k + kh) * k + kw] = xp[n][ci][oh * s + kh][ow * s + kw], xp the periodic pad."""
    xp = cb.pad_fwd(np.asarray(x, np.float32), pads)
    N, Cin, PH, PW = xp.shape
    OH, OW = (PH - k) // s + 1, (PW - k) // s + 1
    rows = (np.arange(OH) * s)[:, None] + np.arange(k)[None, :]                    # [OH][kh]
    cols = (np.arange(OW) * s)[:, None] + np.arange(k)[None, :]                    # [OW][kw]
    t = xp[:, :, rows][:, :, :, :, cols]                                           # [N][Cin][OH][kh][OW][kw]
    return np.ascontiguousarray(t.transpose(0, 2, 4, 1, 3, 5).reshape(N, OH * OW, Cin * k * k))


def conv_y(x, w, b, s, pads):
    """y [N][2C][OH][OW]: acc = b[c2], then acc = fma(xp, w, acc) over ci, kh, kw ascending; for odd K one closing fma(+0, +0, acc)."""
    C2, Cin, k, _ = w.shape
    K = Cin * k * k
    OH, OW = out_hw(x.shape[2], x.shape[3], k, s, pads)
    cols, wm = columns(x, k, s, pads), np.asarray(w, np.float32).reshape(C2, K)
    acc = np.broadcast_to(np.asarray(b, np.float32)[None, :, None], (x.shape[0], C2, OH * OW)).copy()
    for kk in range(K):
        acc = fma32(cols[:, None, :, kk], wm[None, :, kk, None], acc)
    if K % 2:
        acc = fma32(np.float32(0), np.float32(0), acc)
    return acc.reshape(x.shape[0], C2, OH, OW)


def forward(x, w, b, s, pads):
    """(out [N][C][OH][OW], first bool): convblock.hip's maxout rule on the two halves of conv_y."""
    return cb.maxout_fwd(conv_y(x, w, b, s, pads))


def forward_bar(x, w, b, s, pads):
    """[N][2C][OH][OW]: gamma_n * (|b| + sum |xp * w|) with n = K rounded up to even, around the float64 value of y."""
    C2, Cin, k, _ = w.shape
    K = Cin * k * k
    OH, OW = out_hw(x.shape[2], x.shape[3], k, s, pads)
    mag = np.abs(columns(x, k, s, pads)).astype(np.float64) @ np.abs(w.reshape(C2, K)).astype(np.float64).T      # [N][P][2C]
    mag = mag.transpose(0, 2, 1) + np.abs(np.asarray(b, np.float64))[None, :, None]
    return (gamma(K + K % 2) * mag).reshape(x.shape[0], C2, OH, OW)


def chunks_of(M):
    return (M + CHUNK - 1) // CHUNK


def _wgrad_operands(x, g, first, k, s, pads):
    gy = cb.maxout_bwd(g, first)                                                   # [N][2C][OH][OW], by selection
    N, C2 = gy.shape[:2]
    gym = np.ascontiguousarray(gy.reshape(N, C2, -1).transpose(0, 2, 1)).reshape(-1, C2)       # [M][2C], m = (n * OH + oh) * OW + ow
    cols = columns(x, k, s, pads)
    cols = np.concatenate([cols.reshape(gym.shape[0], -1), np.ones((gym.shape[0], 1), np.float32)], axis=1)      # tap K: the bias's 1
    return gym, cols


def weight_grad(x, g, first, k, s, pads):
    """(gw [2C][Cin][k][k], gb [2C]): chunks of CHUNK consecutive m, each one chain from +0 ascending in m, the partials added in
    ascending chunk order in float32 starting from the first.  (The closing fma(+0, +0, acc) of an odd chunk is invisible: a chain
    from +0 is never -0.)"""
    gym, cols = _wgrad_operands(x, g, first, k, s, pads)
    M, C2 = gym.shape
    total = None
    for j in range(chunks_of(M)):
        a, c = gym[j * CHUNK:(j + 1) * CHUNK], cols[j * CHUNK:(j + 1) * CHUNK]
        acc = np.zeros((C2, cols.shape[1]), np.float32)
        for m in range(a.shape[0]):
            acc = fma32(a[m][:, None], c[m][None, :], acc)
        with np.errstate(all="ignore"):
            total = acc if total is None else (total + acc).astype(np.float32)
    return np.ascontiguousarray(total[:, :-1]).reshape(C2, x.shape[1], k, k), np.ascontiguousarray(total[:, -1])


def weight_grad_bar(x, g, first, k, s, pads):
    """([2C][Cin][k][k], [2C]): gamma_n * sum |gy * xp| with n = the chunk length (M where that is shorter) + the number of chunks."""
    gym, cols = _wgrad_operands(x, g, first, k, s, pads)
    mag = gamma(min(CHUNK, gym.shape[0]) + chunks_of(gym.shape[0])) * (np.abs(gym).astype(np.float64).T @ np.abs(cols).astype(np.float64))
    return mag[:, :-1].reshape(-1, x.shape[1], k, k), mag[:, -1]


def _spread(gy, k, s, PH, PW):
    """v[kh][kw] [N][2C][PH][PW]: gy at the padded positions (oh * s + kh, ow * s + kw), +0 at every other one (the invalid taps)."""
    N, C2, OH, OW = gy.shape
    out = {}
    for kh in range(k):
        for kw in range(k):
            v = np.zeros((N, C2, PH, PW), np.float32)
            v[:, :, kh:kh + s * OH:s, kw:kw + s * OW:s] = gy
            out[kh, kw] = v
    return out


def padded_grad(g, first, w, hw, s, pads):
    """gp [N][Cin][PH][PW]: acc = +0, then acc = fma(w[c2][ci][kh][kw], v, acc) over c2, kh, kw ascending, v the selected cotangent at a
    valid tap and +0 at an invalid one."""
    C2, Cin, k, _ = w.shape
    wl, wr, hl, hr = pads
    PH, PW = hw[0] + hl + hr, hw[1] + wl + wr
    v = _spread(cb.maxout_bwd(g, first), k, s, PH, PW)
    acc = np.zeros((g.shape[0], Cin, PH, PW), np.float32)
    for c2 in range(C2):
        for kh in range(k):
            for kw in range(k):
                acc = fma32(np.asarray(w, np.float32)[c2, :, kh, kw][None, :, None, None], v[kh, kw][:, c2][:, None], acc)
    return acc


def input_grad(g, first, w, hw, s, pads):
    """gx [N][Cin][H][W]: padded_grad folded with the periodic pad's order (columns ascending in q, then rows ascending in r)."""
    return cb.pad_bwd(padded_grad(g, first, w, hw, s, pads), hw, pads)


def input_grad_bar(g, first, w, hw, s, pads):
    """[N][Cin][H][W]: gamma_n * the folded sum |w * v|, n = 2C * k * k plus the additions of the fold (copies per axis, at most)."""
    C2, Cin, k, _ = w.shape
    wl, wr, hl, hr = pads
    H, W = hw
    PH, PW = H + hl + hr, W + wl + wr
    v = _spread(np.abs(cb.maxout_bwd(g, first)), k, s, PH, PW)
    mag = np.zeros((g.shape[0], Cin, PH, PW), np.float64)
    aw = np.abs(np.asarray(w, np.float64))
    for (kh, kw), t in v.items():
        mag += np.einsum("ci,nchw->nihw", aw[:, :, kh, kw], t.astype(np.float64))
    fold = np.zeros((g.shape[0], Cin, H, W), np.float64)
    np.add.at(fold, (slice(None), slice(None), cb.pad_index(H, hl, hr)[:, None], cb.pad_index(W, wl, wr)[None, :]), mag)
    copies = -(-PH // H) + -(-PW // W)
    return gamma(C2 * k * k + copies) * fold
