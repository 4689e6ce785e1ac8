"""numpy restatement of csrc/conv_transpose.hip: the forward's phase chains with their tail rule and the selection, the input gradient
with its invalid taps, the chunked weight gradient over the input pixels and the chunked bias gradient over the output pixels, every
fused multiply-add a correctly rounded float32 fma (np_twin_conv.fma32); and the error bars that hold the twin
(tests/test_conv_transpose_cpu.py) and the device (tests/test_gpu_conv_transpose.py) to a float64 evaluation.  The chains are
vectorised over the outputs and sequential along the sum, as the header states them."""
import numpy as np

from tests import np_twin_convblock as cb
from tests.np_twin_conv import CHUNK, chunks_of, fma32, gamma

#        (N, Cin, H, W, C, k, s)
CASES = [(1, 1, 1, 1, 1, 1, 1),          # everything degenerate
         (2, 3, 5, 7, 1, 4, 2),          # the recipes' k4 s2; an odd chain length comes from odd Cin only
         (1, 3, 3, 4, 3, 3, 2),          # opad = 1; phases of 1, 2 and 4 taps: odd and even chains in one call
         (2, 5, 4, 6, 2, 2, 1),          # the toy recipe's --ks 2 --se 1: one pixel larger than the input, cropped by the decoder
         (1, 2, 3, 3, 2, 5, 3),          # stride 3
         (1, 1, 2, 3, 2, 8, 2),          # k = 8, pad 3
         (1, 2, 2, 2, 1, 3, 3),          # one tap per phase
         (3, 4, 9, 10, 20, 4, 2),        # 2C = 40 straddles a 32-row tile
         (1, 24, 4, 4, 44, 4, 2),        # c3's first transposed block, 24 -> 44: 2C = 88, three row tiles
         (1, 66, 3, 5, 3, 4, 2),         # c3's 66 input channels: three ci tiles, two rows in the last
         (1, 2, 33, 65, 1, 4, 2),        # one past 32 and one past 64 pixels per phase row
         (1, 2, 64, 64, 2, 4, 2)]        # 4 chunks of m and 16 chunks of mo
# (M, Mo) = (1023, 1023), (1024, 1024), (1025, 1025), (256, 1024), (960, 1025)
CHUNK_CASES = [(1, 1, 33, 31, 1, 1, 1), (1, 1, 32, 32, 1, 1, 1), (1, 1, 25, 41, 1, 1, 1), (1, 1, 16, 16, 1, 2, 2), (1, 1, 24, 40, 1, 2, 1)]


def case_id(case):
    return "x".join(map(str, case))


def block_pad(k, s):
    """(pad, opad) as ConvBlock.__init__ derives them for a transposed block."""
    pad = (k - s + 1) // 2
    opad = s + 2 * pad - k
    if not 0 <= opad < s:
        pad = max((k - s) // 2, 0)
        opad = min(max(s + 2 * pad - k, 0), s - 1)
    return pad, opad


def out_hw(H, W, k, s, pad, opad):
    return (H - 1) * s - 2 * pad + k + opad, (W - 1) * s - 2 * pad + k + opad


def _shifted(t, rows, cols):
    """t[..., rows, cols] as an outer product of the two index vectors, +0 where an index is outside its axis."""
    H, W = t.shape[-2:]
    rv, cv = (rows >= 0) & (rows < H), (cols >= 0) & (cols < W)
    v = t[..., np.clip(rows, 0, H - 1), :][..., np.clip(cols, 0, W - 1)]
    return np.where(rv[:, None] & cv[None, :], v, np.float32(0)).astype(np.float32)


def _phases(OH, OW, k, s, pad):
    """Per phase (py, px) = ((oy + pad) mod s, (ox + pad) mod s): its output rows, its output columns, its taps kh and its taps kw."""
    for py in range(s):
        oys = np.arange((py - pad) % s, OH, s)
        for px in range(s):
            oxs = np.arange((px - pad) % s, OW, s)
            if oys.size and oxs.size:
                yield oys, oxs, list(range(py, k, s)), list(range(px, k, s))


def conv_y(x, w, b, s, pad, opad):
    """y [N][2C][OH][OW]: per phase acc = b[c2], then acc = fma(v, w[ci][c2][kh][kw], acc) over ci, phase kh, phase kw ascending, v = +0
    at a phase tap outside the image; for an odd chain length one closing fma(+0, +0, acc)."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    N, Cin, H, W = x.shape
    C2, k = w.shape[1], w.shape[2]
    OH, OW = out_hw(H, W, k, s, pad, opad)
    y = np.zeros((N, C2, OH, OW), np.float32)
    for oys, oxs, khs, kws in _phases(OH, OW, k, s, pad):
        acc = np.broadcast_to(np.asarray(b, np.float32)[None, :, None, None], (N, C2, oys.size, oxs.size)).copy()
        for ci in range(Cin):
            for kh in khs:
                for kw in kws:
                    v = _shifted(x[:, ci], (oys + pad - kh) // s, (oxs + pad - kw) // s)
                    acc = fma32(v[:, None], w[ci, :, kh, kw][None, :, None, None], acc)
        if (Cin * len(khs) * len(kws)) % 2:
            acc = fma32(np.float32(0), np.float32(0), acc)
        y[:, :, oys[:, None], oxs[None, :]] = acc
    return y


def forward(x, w, b, s, pad, opad):
    """(out [N][C][OH][OW], first bool): convblock.hip's maxout rule on the two halves of conv_y."""
    return cb.maxout_fwd(conv_y(x, w, b, s, pad, opad))


def forward_bar(x, w, b, s, pad, opad):
    """[N][2C][OH][OW]: gamma_n * (|b| + sum |v * w|) with n = the pixel's phase chain length rounded up to even, around float64's y."""
    x, w = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64))
    N, Cin, H, W = x.shape
    C2, k = w.shape[1], w.shape[2]
    OH, OW = out_hw(H, W, k, s, pad, opad)
    bar = np.zeros((N, C2, OH, OW))
    for oys, oxs, khs, kws in _phases(OH, OW, k, s, pad):
        mag = np.broadcast_to(np.abs(np.asarray(b, np.float64))[None, :, None, None], (N, C2, oys.size, oxs.size)).copy()
        for kh in khs:
            for kw in kws:
                rows, cols = (oys + pad - kh) // s, (oxs + pad - kw) // s
                rv, cv = (rows >= 0) & (rows < H), (cols >= 0) & (cols < W)
                v = x[:, :, np.clip(rows, 0, H - 1), :][:, :, :, np.clip(cols, 0, W - 1)] * (rv[:, None] & cv[None, :])
                mag += np.einsum("nihw,ic->nchw", v, w[:, :, kh, kw])
        L = Cin * len(khs) * len(kws)
        bar[:, :, oys[:, None], oxs[None, :]] = gamma(L + L % 2) * mag
    return bar


def _taps(gy, hw, k, s, pad):
    """v[kh, kw] [N][2C][H][W]: gy at (iy * s - pad + kh, ix * s - pad + kw), +0 where that position is outside the output."""
    H, W = hw
    return {(kh, kw): _shifted(gy, np.arange(H) * s - pad + kh, np.arange(W) * s - pad + kw) for kh in range(k) for kw in range(k)}


def input_grad(g, first, w, hw, s, pad):
    """gx [N][Cin][H][W]: acc = +0, then acc = fma(w[ci][c2][kh][kw], v, acc) over c2, kh, kw ascending, v the selected cotangent at a
    valid tap and +0 at an invalid one."""
    w = np.asarray(w, np.float32)
    Cin, C2, k, _ = w.shape
    v = _taps(cb.maxout_bwd(g, first), hw, k, s, pad)
    acc = np.zeros((g.shape[0], Cin) + tuple(hw), np.float32)
    for c2 in range(C2):
        for kh in range(k):
            for kw in range(k):
                acc = fma32(w[:, c2, kh, kw][None, :, None, None], v[kh, kw][:, c2][:, None], acc)
    return acc


def input_grad_bar(g, first, w, hw, s, pad):
    """[N][Cin][H][W]: gamma_n * sum |w * v| with n = 2C * k * k."""
    aw = np.abs(np.asarray(w, np.float64))
    Cin, C2, k, _ = aw.shape
    v = _taps(np.abs(cb.maxout_bwd(g, first)), hw, k, s, pad)
    mag = np.zeros((g.shape[0], Cin) + tuple(hw), np.float64)
    for (kh, kw), t in v.items():
        mag += np.einsum("ic,nchw->nihw", aw[:, :, kh, kw], t.astype(np.float64))
    return gamma(C2 * k * k) * mag


def _wgrad_operands(x, g, first, k, s, pad):
    """xm [M][Cin] and gt [M][2C][k][k], m = (n * H + iy) * W + ix: the input and the selected cotangent at m's position shifted by the tap."""
    x = np.asarray(x, np.float32)
    N, Cin, H, W = x.shape
    v = _taps(cb.maxout_bwd(g, first), (H, W), k, s, pad)
    gt = np.stack([np.stack([v[kh, kw] for kw in range(k)], axis=-1) for kh in range(k)], axis=-2)      # [N][2C][H][W][kh][kw]
    gt = np.ascontiguousarray(gt.transpose(0, 2, 3, 1, 4, 5)).reshape(N * H * W, -1, k, k)
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(N * H * W, Cin), gt


def weight_grad(x, g, first, k, s, pad):
    """gw [Cin][2C][k][k]: chunks of CHUNK consecutive m, each one chain from +0 ascending in m, acc = fma(gy_tap, x, acc); the partials
    added in ascending chunk order in float32 starting from the first."""
    xm, gt = _wgrad_operands(x, g, first, k, s, pad)
    total = None
    for j in range(chunks_of(xm.shape[0])):
        a, c = gt[j * CHUNK:(j + 1) * CHUNK], xm[j * CHUNK:(j + 1) * CHUNK]
        acc = np.zeros((xm.shape[1],) + gt.shape[1:], np.float32)
        for m in range(a.shape[0]):
            acc = fma32(a[m][None], c[m][:, None, None, None], acc)
        with np.errstate(all="ignore"):
            total = acc if total is None else (total + acc).astype(np.float32)
    return total


def weight_grad_bar(x, g, first, k, s, pad):
    """[Cin][2C][k][k]: gamma_n * sum |x * gy_tap| with n = the chunk length (M where that is shorter) + the number of chunks."""
    xm, gt = _wgrad_operands(x, g, first, k, s, pad)
    M = xm.shape[0]
    return gamma(min(CHUNK, M) + chunks_of(M)) * np.einsum("mi,mckl->ickl", np.abs(xm).astype(np.float64), np.abs(gt).astype(np.float64))


def bias_grad(g, first):
    """gb [2C]: chunks of CHUNK consecutive mo = (n * OH + oy) * OW + ox, each one chain of float32 additions from +0 ascending in mo
    (fma(gy, 1, acc)); the partials added in ascending chunk order starting from the first."""
    gy = cb.maxout_bwd(g, first)
    gym = np.ascontiguousarray(gy.reshape(gy.shape[0], gy.shape[1], -1).transpose(0, 2, 1)).reshape(-1, gy.shape[1])
    total = None
    with np.errstate(all="ignore"):
        for j in range(chunks_of(gym.shape[0])):
            acc = np.zeros(gym.shape[1], np.float32)
            for row in gym[j * CHUNK:(j + 1) * CHUNK]:
                acc = (acc + row).astype(np.float32)
            total = acc if total is None else (total + acc).astype(np.float32)
    return total


def bias_grad_bar(g, first):
    """[2C]: gamma_n * sum |gy| with n = the chunk length (Mo where that is shorter) + the number of its chunks."""
    gy = np.abs(cb.maxout_bwd(g, first)).astype(np.float64)
    Mo = gy.shape[0] * gy.shape[2] * gy.shape[3]
    return gamma(min(CHUNK, Mo) + chunks_of(Mo)) * gy.sum(axis=(0, 2, 3))
