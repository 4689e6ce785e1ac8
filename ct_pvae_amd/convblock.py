"""The glue around every convolution of the P-VAE's ConvBlock as one forward and one backward launch each (csrc/convblock.hip states
the functions, the layout and the backward's order of addition).

    periodic_pad(x, pads)   x [N][C][H][W] -> [N][C][H + hl + hr][W + wl + wr], pads = (wl, wr, hl, hr) as ConvBlock.forward builds
                            them: out[.., r, q] = x[.., (r - hl) mod H, (q - wl) mod W]; what trainer._PeriodicPad computes
    maxout(y)               y [N][2C][H][W] -> [N][C][H][W]: the first channel half where it is >= the second, else the second; what
                            trainer._Maxout computes

    dropout(x, rate, *, seed, draw, layer, first_object=0)             x [N][C][H][W] -> the same shape: the ConvBlock's dropout
                            (ctvae/models.py:283-284) with a Philox-keyed mask; the backward draws the mask again, nothing is saved
    dropout_pad(x, pads, rate, *, seed, draw, layer, first_object=0)   periodic_pad(dropout(x), pads) as one launch each way
    dropout_mask(n, length, rate, *, seed, draw, layer, first_object=0)   the keep decisions the kernels take, on the host (no GPU
                            needed), a numpy bool [n][length]

The dropout's stream (include/ctpvae_radon.h states it): element i of object n of the block input, e = (first_object + n) * C * H * W + i,
takes word e & 3 of Philox4x32-10((lo32(e >> 2), hi32(e >> 2), draw, 0x44000000 | layer), key = seed); k = w >> 8 is kept iff
k * 2^-24 >= float32(rate); a kept element is x * float32(1 / (1 - rate)), a dropped one is +0 BY SELECTION: a dropped inf or NaN gives
+0, where TensorFlow's x * scale * mask gives NaN.

There is no CPU path for the tensor operations."""
import math

import numpy as np
import torch

from . import _lib, forward_functions
from ._args import check_float32, counter_args
from .forward_functions import _stream_ptr

__all__ = ["periodic_pad", "maxout", "dropout", "dropout_pad", "dropout_mask"]


NCHW = "a non-empty [N][C][H][W] tensor"


class _FusedPeriodicPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pads):
        N, C, H, W = x.shape
        wl, wr, hl, hr = pads
        out = forward_functions._new_output((N, C, H + hl + hr, W + wl + wr), torch.float32, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().ctpvae_periodic_pad_fwd_f32(x.data_ptr(), N * C, H, W, wl, wr, hl, hr, out.data_ptr(), _stream_ptr()),
                       "periodic_pad_fwd")
        ctx.geom = (N, C, H, W, wl, wr, hl, hr)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None
        N, C, H, W, wl, wr, hl, hr = ctx.geom
        g = g.to(torch.float32).contiguous()
        gx = forward_functions._new_output((N, C, H, W), torch.float32, g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().ctpvae_periodic_pad_bwd_f32(g.data_ptr(), N * C, H, W, wl, wr, hl, hr, gx.data_ptr(), _stream_ptr()),
                       "periodic_pad_bwd")
        return gx, None


class _FusedMaxout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        N, C2, H, W = y.shape
        length = (C2 // 2) * H * W
        out = forward_functions._new_output((N, C2 // 2, H, W), torch.float32, y.device)
        first = torch.empty((N, C2 // 2, H, W), dtype=torch.uint8, device=y.device)     # (saved state, every byte written by the launch)
        with torch.cuda.device(y.device):
            _lib.check(_lib.load().ctpvae_maxout_fwd_f32(y.data_ptr(), N, length, out.data_ptr(), first.data_ptr(), _stream_ptr()),
                       "maxout_fwd")
        ctx.save_for_backward(first)                  # one byte per output element; never a copy of y
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None
        first, = ctx.saved_tensors
        N, C, H, W = first.shape
        g = g.to(torch.float32).contiguous()
        gy = forward_functions._new_output((N, 2 * C, H, W), torch.float32, g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().ctpvae_maxout_bwd_f32(g.data_ptr(), first.data_ptr(), N, C * H * W, gy.data_ptr(), _stream_ptr()),
                       "maxout_bwd")
        return gy


def _rate_args(what, rate):
    """(T, scale) of a rate: T = ceil(float32(rate) * 2^24), the least k = w >> 8 that is kept; scale = float32(1 / (1 - rate)), the
    quotient taken in double."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)):
        raise TypeError(f"{what}: rate must be a Python float (got {type(rate).__name__})")
    rate = float(rate)
    r32 = float(np.float32(rate))
    if not 0.0 < r32 < 1.0:                                            # (a NaN fails both comparisons)
        raise ValueError(f"{what}: rate must satisfy 0 < float32(rate) < 1 (got {rate!r})")
    return int(math.ceil(r32 * 2.0 ** 24)), float(np.float32(1.0 / (1.0 - rate)))          # r32 * 2^24 is exact in double


def _key_args(what, seed, draw, layer, first_object, n, length):
    seed, draw, first_object = counter_args(seed, draw, first_object)
    layer = int(layer)
    if not 0 <= layer < 2 ** 24:
        raise ValueError(f"{what}: layer shares a counter word with the tag: 0 <= layer < 2^24 (got {layer})")
    if (first_object + n) * length >= 2 ** 63:
        raise ValueError(f"{what}: (first_object + N) * C * H * W must fit 63 bits (got first_object = {first_object})")
    return seed, draw, layer, first_object


def _pads_args(what, x, pads):
    pads = tuple(int(p) for p in pads)
    if len(pads) != 4 or min(pads) < 0:
        raise ValueError(f"{what}: pads must be four non-negative integers (wl, wr, hl, hr) (got {pads})")
    if (x.shape[0] * x.shape[1]) * (x.shape[2] + pads[2] + pads[3]) * (x.shape[3] + pads[0] + pads[1]) >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 padded elements per call (got {tuple(x.shape)} with pads {pads})")
    return pads


class _Dropout(torch.autograd.Function):
    """key = (first_object, seed, draw, layer, T, scale): all the backward needs -- the mask is drawn again."""

    @staticmethod
    def forward(ctx, x, key):
        N, C, H, W = x.shape
        out = forward_functions._new_output((N, C, H, W), torch.float32, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().ctpvae_dropout_fwd_f32(x.data_ptr(), N, C * H * W, *key, out.data_ptr(), _stream_ptr()), "dropout_fwd")
        ctx.geom, ctx.key = (N, C, H, W), key
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None
        N, C, H, W = ctx.geom
        g = g.to(torch.float32).contiguous()
        gx = forward_functions._new_output((N, C, H, W), torch.float32, g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().ctpvae_dropout_bwd_f32(g.data_ptr(), N, C * H * W, *ctx.key, gx.data_ptr(), _stream_ptr()), "dropout_bwd")
        return gx, None


class _FusedDropoutPad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pads, key):
        N, C, H, W = x.shape
        wl, wr, hl, hr = pads
        out = forward_functions._new_output((N, C, H + hl + hr, W + wl + wr), torch.float32, x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().ctpvae_dropout_pad_fwd_f32(x.data_ptr(), N, C, H, W, wl, wr, hl, hr, *key, out.data_ptr(), _stream_ptr()),
                       "dropout_pad_fwd")
        ctx.geom, ctx.key = (N, C, H, W, wl, wr, hl, hr), key
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None
        N, C, H, W, wl, wr, hl, hr = ctx.geom
        g = g.to(torch.float32).contiguous()
        gx = forward_functions._new_output((N, C, H, W), torch.float32, g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().ctpvae_dropout_pad_bwd_f32(g.data_ptr(), N, C, H, W, wl, wr, hl, hr, *ctx.key, gx.data_ptr(),
                                                              _stream_ptr()), "dropout_pad_bwd")
        return gx, None, None


def dropout_mask(n, length, rate, *, seed, draw, layer, first_object=0):
    """numpy bool [n][length]: True where dropout / dropout_pad keep element i of object b of a block input with C * H * W = length --
    (w >> 8) * 2^-24 >= float32(rate) for w = word e & 3 of Philox4x32-10((lo32(e >> 2), hi32(e >> 2), draw, 0x44000000 | layer),
    key = seed), e = (first_object + b) * length + i.  Computed on the host; needs no GPU."""
    T, _ = _rate_args("dropout_mask", rate)
    n, length = int(n), int(length)
    if n < 1 or length < 1:
        raise ValueError(f"dropout_mask: n and length must be positive (got {n}, {length})")
    seed, draw, layer, first_object = _key_args("dropout_mask", seed, draw, layer, first_object, n, length)
    out = np.empty((n, length), np.uint8)
    _lib.check(_lib.load().ctpvae_dropout_keep_host_u8(n, length, first_object, seed, draw, layer, T, out.ctypes.data), "dropout_keep_host")
    return out.astype(bool)


def dropout(x, rate, *, seed, draw, layer, first_object=0):
    """x [N][C][H][W]: a contiguous float32 CUDA tensor, a ConvBlock's input; rate a Python float with 0 < float32(rate) < 1.  Returns
    where(keep, x * float32(1 / (1 - rate)), +0) with keep = dropout_mask(N, C * H * W, rate, ...): one float32 multiply at a kept element;
    a dropped element is +0 by selection, so a dropped inf or NaN gives +0 (TensorFlow's x * scale * mask gives NaN there).  The mask
    depends on (seed, draw, layer, first_object + n, element) alone: pass the step index as `draw`, the block's number as `layer` and
    the offset of x's first object in the global batch as `first_object`, and a batch cut over calls or ranks drops what the whole
    batch drops.  Differentiable once in x: gx = where(keep, scale * g, +0), the mask drawn again -- the forward saves no tensor."""
    check_float32("dropout", "x", x, 4, NCHW)
    key_rate = _rate_args("dropout", rate)
    if x.numel() >= 2 ** 31:
        raise ValueError(f"dropout: at most 2^31 - 1 elements per call (got {tuple(x.shape)})")
    seed, draw, layer, first_object = _key_args("dropout", seed, draw, layer, first_object, x.shape[0], x.numel() // x.shape[0])
    if x.device.type != "cuda":
        raise _lib.RadonLibraryError("dropout: x must be a CUDA tensor; there is no CPU path")
    return _Dropout.apply(x, (first_object, seed, draw, layer) + key_rate)


def dropout_pad(x, pads, rate, *, seed, draw, layer, first_object=0):
    """periodic_pad(dropout(x, rate, ...), pads) -- the same bits -- as ONE launch, and its backward as one: the keep decision belongs
    to the source element, so every wrapped copy of an element shares its fate; the backward is periodic_pad's gather with its order
    of addition, then where(keep, scale * sum, +0) at the source element, the mask drawn again -- the forward saves no tensor.
    x, rate and the keyword arguments as dropout's, pads = (wl, wr, hl, hr) as periodic_pad's."""
    check_float32("dropout_pad", "x", x, 4, NCHW)
    pads = _pads_args("dropout_pad", x, pads)
    key_rate = _rate_args("dropout_pad", rate)
    seed, draw, layer, first_object = _key_args("dropout_pad", seed, draw, layer, first_object, x.shape[0], x.numel() // x.shape[0])
    if x.device.type != "cuda":
        raise _lib.RadonLibraryError("dropout_pad: x must be a CUDA tensor; there is no CPU path")
    return _FusedDropoutPad.apply(x, pads, (first_object, seed, draw, layer) + key_rate)


def periodic_pad(x, pads):
    """x [N][C][H][W]: a contiguous float32 CUDA tensor; pads = (wl, wr, hl, hr), non-negative integers, last axis first as
    torch.nn.functional.pad orders them.  Returns out [N][C][H + hl + hr][W + wl + wr] with out[n, c, r, q] = x[n, c, (r - hl) mod H,
    (q - wl) mod W] (the mathematical modulo; a pad may exceed the extent).  Differentiable once in x.  The backward is a
    deterministic gather with a fixed order of addition: per padded row the cotangents of a source column's copies are added in
    ascending q, then the rows of a source row in ascending r, each sum starting from its first term -- the same bits from run to
    run; with at most two copies per axis (every pad of the trainer's recipes) the value of trainer._PeriodicPad's index_add_ chain."""
    check_float32("periodic_pad", "x", x, 4, NCHW)
    pads = _pads_args("periodic_pad", x, pads)
    if x.device.type != "cuda":
        raise _lib.RadonLibraryError("periodic_pad: x must be a CUDA tensor; there is no CPU path")
    return _FusedPeriodicPad.apply(x, pads)


def maxout(y):
    """y [N][2C][H][W]: a contiguous float32 CUDA tensor, the two convolutions of a ConvBlock side by side on the channel axis.  Returns
    out [N][C][H][W] = where(first, y[:, :C], y[:, C:]) with first = y[:, :C] >= y[:, C:]: a tie takes the first half (TensorFlow's
    MaximumGrad), a NaN in either half makes the comparison false and takes the second half, -0.0 >= +0.0 is true.  Differentiable
    once in y: the cotangent goes to the half that was taken and +0 to the other, by selection (an infinite cotangent gives inf and 0,
    where g * first gives inf and NaN).  The backward keeps one byte per output element, never a copy of y."""
    check_float32("maxout", "y", y, 4, NCHW)
    if y.shape[1] % 2 != 0:
        raise ValueError(f"maxout: y needs an even channel count, the two convolutions' halves (got {tuple(y.shape)})")
    if y.numel() >= 2 ** 31:
        raise ValueError(f"maxout: at most 2^31 - 1 elements per call (got {tuple(y.shape)})")
    if y.device.type != "cuda":
        raise _lib.RadonLibraryError("maxout: y must be a CUDA tensor; there is no CPU path")
    return _FusedMaxout.apply(y)
