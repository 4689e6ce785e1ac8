"""Per-pixel posterior marginals of the P-VAE's output head (the reference's CT_VAE.pixel_dist) -- the TruncatedNormal head of --normal
or the reference's default Beta head --: a histogram and two moments per pixel, accumulated on the device with no sample ever written to
memory (csrc/marginals.hip states the layout, the bin rule and the fixed order of the float64 sums; csrc/beta_marginals.hip runs the
same code on the Beta head's samples).

    m = PixelMarginals((X, Y), bins=50, lo=0.005, width=0.01, device="cuda")    the reference's np.arange(0.005, 0.51, 0.01)
    m.add(alpha, beta, draws=100, seed=1234, draw0=0, first_object=0)           alpha, beta [n][1][X][Y]: n * draws samples per pixel,
                                                                                sample (o, pixel, k) IS truncated_normal_head's x
                                                                                for draw = draw0 + k
    m = PixelMarginals((X, Y), head="beta")                                     the same of the default Beta head: sample (o, pixel, k)
                                                                                IS beta_head's x for draw = draw0 + k
    m.count, m.hist, m.mean(), m.std(), m.edges, m.save(path), PixelMarginals.load(path)
    bin_samples(samples, lo, width, bins)                                       the same bin rule on any [..., pix] host array (e.g.
                                                                                hmc_sample's output), so two curves share their bins
    hist_distance(a, b)                                                         total-variation distance per pixel of two hist

Nothing in add() grows with `draws`: beside alpha, beta and the state it allocates one workspace of at most 1024 * X * Y bytes.
There is no CPU path for add()."""
import math

import numpy as np
import torch

from . import _lib
from ._args import check_float32, counter_args
from .forward_functions import _stream_ptr

__all__ = ["PixelMarginals", "bin_samples", "bin_columns", "hist_distance", "MAX_BINS"]

MAX_BINS = 254     # CTPVAE_MARGINALS_MAX_BINS
HEADS = {"truncated_normal": "tn_marginals", "beta": "beta_marginals"}     # head -> the stem of its two entry points


def _grid_args(bins, lo, width):
    bins, lo, width = int(bins), float(lo), float(width)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must be 1 .. {MAX_BINS} (got {bins})")
    if not (math.isfinite(lo) and math.isfinite(width)) or width <= 0:
        raise ValueError(f"lo and width must be finite and width > 0 (got lo={lo}, width={width})")
    with np.errstate(over="ignore"):
        lo32, width32 = float(np.float32(lo)), float(np.float32(width))
    if not (math.isfinite(lo32) and math.isfinite(width32)) or width32 <= 0:
        raise ValueError(f"lo and width must be finite float32 values and width > 0 as float32 (got lo={lo}, width={width})")
    return bins, lo, width


def bin_columns(x, lo, width, bins):
    """int32 array of x's shape: the column of every float32 value under the library's own bin rule (host code of the kernel's
    function): t = (x - lo) / width in float32; 0 if not t >= 0 (NaN too), bins + 1 if t >= bins, else 1 + int(t)."""
    bins, lo, width = _grid_args(bins, lo, width)
    x = np.ascontiguousarray(x, dtype=np.float32)
    col = np.empty(x.shape, np.int32)
    _lib.check(_lib.load().ctpvae_tn_marginals_bin_host_f32(x.ctypes.data, x.size, lo, width, bins, col.ctypes.data), "tn_marginals_bin_host")
    return col


def bin_samples(samples, lo, width, bins):
    """int64 [pix][bins + 2]: the histogram of a host array [..., pix] of samples (any leading axes; float32, or cast to it) under the
    rule PixelMarginals uses on the device.  Column 0 counts samples below lo (and NaN), column bins + 1 those at or above lo + bins *
    width (in the float32 arithmetic of the rule), every row sums to the number of samples per pixel."""
    samples = np.asarray(samples)
    if samples.ndim < 1 or samples.shape[-1] < 1:
        raise ValueError(f"bin_samples: samples must be [..., pix] with pix >= 1 (got {samples.shape})")
    col = bin_columns(samples, lo, width, bins).reshape(-1, samples.shape[-1])
    pix, cols = col.shape[1], int(bins) + 2
    flat = (np.arange(pix, dtype=np.int64)[None, :] * cols + col).ravel()
    return np.bincount(flat, minlength=pix * cols).astype(np.int64).reshape(pix, cols)


def hist_distance(a, b):
    """float64 [pix]: the total-variation distance 0.5 * sum_col |a / sum(a) - b / sum(b)| between two binned marginals, integer
    arrays [pix][cols] of one shape (two hist of one grid: a PixelMarginals' against an HmcMarginals' object).  A row with an empty
    total gives NaN."""
    a, b = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in (a, b))
    if a.ndim != 2 or a.shape != b.shape or a.dtype.kind not in "iu" or b.dtype.kind not in "iu":
        raise ValueError(f"hist_distance: two integer arrays [pix][cols] of one shape (got {a.shape} {a.dtype}, {b.shape} {b.dtype})")
    a, b = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.5 * np.abs(a / a.sum(1, keepdims=True) - b / b.sum(1, keepdims=True)).sum(1)


def _check_input(name, t, shape_xy):
    check_float32("PixelMarginals.add", name, t, 4, f"[n][1][{shape_xy[0]}][{shape_xy[1]}], the decoder's layout",
                  lambda shape: shape[1] == 1 and tuple(shape[2:]) == shape_xy)


class PixelMarginals:
    """State of the per-pixel marginals of an (X, Y) pixel grid: hist [X * Y][bins + 2] int64, s1, s2 [X * Y] float64 and a count, all
    zero at first; add() accumulates into them on the device.  head: "truncated_normal" (the output head of --normal) or "beta" (the
    reference's default output head) -- whose samples add() draws."""

    def __init__(self, shape, bins=50, lo=0.005, width=0.01, device="cuda", head="truncated_normal"):
        if head not in HEADS:
            raise ValueError(f"PixelMarginals: head must be one of {sorted(HEADS)} (got {head!r})")
        self.head = head
        X, Y = (int(v) for v in shape)
        if X < 1 or Y < 1:
            raise ValueError(f"PixelMarginals: the pixel grid must be (X, Y) with both >= 1 (got {tuple(shape)})")
        self.bins, self.lo, self.width = _grid_args(bins, lo, width)
        self.shape = (X, Y)
        self.count = 0
        self._hist = torch.zeros((X * Y, self.bins + 2), dtype=torch.int64, device=torch.device(device))
        self.device = self._hist.device            # ("cuda" has become the current device, with its index)
        self._s1 = torch.zeros(X * Y, dtype=torch.float64, device=self.device)
        self._s2 = torch.zeros(X * Y, dtype=torch.float64, device=self.device)

    def add(self, alpha, beta, *, draws, seed, draw0=0, first_object=0):
        """Add the n * draws samples per pixel of alpha, beta [n][1][X][Y] (contiguous float32 tensors on the state's device; detached,
        no autograd): sample (o, pixel, k) is truncated_normal_head(alpha, beta, seed=seed, draw=draw0 + k, first_object=first_object).x
        of object o at that pixel, bit for bit; with head="beta" it is beta_head(alpha, beta, seed=seed, draw=draw0 + k,
        first_object=first_object)[0] (the sample is not clamped: sqrt_reg plays no part in it).  Every check is made before anything
        is launched."""
        _check_input("alpha", alpha, self.shape)
        _check_input("beta", beta, self.shape)
        if beta.shape != alpha.shape:
            raise ValueError(f"PixelMarginals.add: alpha and beta must have one shape (got {tuple(alpha.shape)}, {tuple(beta.shape)})")
        draws = int(draws)
        if draws < 1:
            raise ValueError(f"PixelMarginals.add: draws must be >= 1 (got {draws})")
        seed, draw0, first_object = counter_args(seed, draw0, first_object)
        if draw0 + draws > 2 ** 32:
            raise ValueError(f"PixelMarginals.add: draw0 + draws must be <= 2^32, the draw is one 32-bit counter word (got {draw0} + {draws})")
        n, pix = alpha.shape[0], self.shape[0] * self.shape[1]
        if alpha.numel() >= 2 ** 31 or n * draws >= 2 ** 32:
            raise ValueError(f"PixelMarginals.add: at most 2^31 - 1 pixels and 2^32 - 1 samples per pixel in one call (got n={n}, "
                             f"pixels={alpha.numel()}, draws={draws})")
        if self.device.type != "cuda" or alpha.device != self.device or beta.device != self.device:
            raise _lib.RadonLibraryError(f"PixelMarginals.add: alpha, beta and the state must be on one CUDA device (state on {self.device}, "
                                         f"alpha on {alpha.device}, beta on {beta.device}); there is no CPU path")
        a, b = alpha.detach(), beta.detach()
        lib = _lib.load()
        stem = HEADS[self.head]
        ws_bytes = _lib.check(getattr(lib, f"ctpvae_{stem}_workspace_bytes")(n, pix, draws), f"{stem}_workspace_bytes")
        with torch.cuda.device(self.device):
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)
            _lib.check(getattr(lib, f"ctpvae_{stem}_f32")(a.data_ptr(), b.data_ptr(), n, pix, first_object, seed, draw0, draws, self.lo,
                                                          self.width, self.bins, self._hist.data_ptr(), self._s1.data_ptr(),
                                                          self._s2.data_ptr(), ws.data_ptr(), _stream_ptr()), stem)
        self.count += n * draws
        return self

    @property
    def hist(self):
        """int64 [X * Y][bins + 2]: below lo | the bins | at or above lo + bins * width."""
        return self._hist

    @property
    def s1(self):
        return self._s1

    @property
    def s2(self):
        return self._s2

    @property
    def edges(self):
        """float64 [bins + 1], nominal: membership is the float32 rule of the kernel, not a comparison with these."""
        return self.lo + self.width * np.arange(self.bins + 1, dtype=np.float64)

    def mean(self):
        """float64 [X][Y] (NaN while count == 0)."""
        if self.count < 1:
            return torch.full(self.shape, float("nan"), dtype=torch.float64, device=self.device)
        return (self._s1 / self.count).view(self.shape)

    def std(self):
        """float64 [X][Y], the sample standard deviation (count - 1); NaN while count < 2."""
        if self.count < 2:
            return torch.full(self.shape, float("nan"), dtype=torch.float64, device=self.device)
        var = (self._s2 - self._s1 * self._s1 / self.count) / (self.count - 1)
        return var.clamp_min(0.0).sqrt().view(self.shape)

    def save(self, path):
        """One .npz: hist, s1, s2, count, lo, width, head (a plain numpy string) and the grid's shape."""
        np.savez(path, hist=self._hist.cpu().numpy(), s1=self._s1.cpu().numpy(), s2=self._s2.cpu().numpy(), count=np.int64(self.count),
                 lo=np.float64(self.lo), width=np.float64(self.width), shape=np.asarray(self.shape, np.int64),
                 head=np.str_(self.head))

    @classmethod
    def load(cls, path, device="cuda"):
        """The state save() wrote; a file without `head` (written before there were two) is a TruncatedNormal state."""
        with np.load(path) as f:
            hist = f["hist"]
            head = str(f["head"]) if "head" in f.files else "truncated_normal"
            m = cls(tuple(int(v) for v in f["shape"]), bins=hist.shape[1] - 2, lo=float(f["lo"]), width=float(f["width"]), device=device,
                    head=head)
            if hist.shape[0] != m.shape[0] * m.shape[1]:
                raise ValueError(f"{path}: hist has {hist.shape[0]} rows for a grid of {m.shape}")
            m._hist.copy_(torch.from_numpy(hist))
            m._s1.copy_(torch.from_numpy(f["s1"]))
            m._s2.copy_(torch.from_numpy(f["s2"]))
            m.count = int(f["count"])
        return m
