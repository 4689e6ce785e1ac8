"""The glue around every convolution of the P-VAE's ConvBlock as one forward and one backward launch each (csrc/convblock.hip states
the functions, the layout and the backward's order of addition).

    periodic_pad(x, pads)   x [N][C][H][W] -> [N][C][H + hl + hr][W + wl + wr], pads = (wl, wr, hl, hr) as ConvBlock.forward builds
                            them: out[.., r, q] = x[.., (r - hl) mod H, (q - wl) mod W]; what trainer._PeriodicPad computes
    maxout(y)               y [N][2C][H][W] -> [N][C][H][W]: the first channel half where it is >= the second, else the second; what
                            trainer._Maxout computes

There is no CPU path."""
import torch

from . import _lib, forward_functions
from .forward_functions import _stream_ptr

__all__ = ["periodic_pad", "maxout"]


def _check_input(what, name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch tensor (got {type(t).__name__})")
    if t.dtype is not torch.float32:
        raise TypeError(f"{what}: {name} must be float32 (got {t.dtype})")
    if t.dim() != 4 or t.numel() == 0:
        raise ValueError(f"{what}: {name} must be a non-empty [N][C][H][W] tensor (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous (got strides {tuple(t.stride())})")


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


def periodic_pad(x, pads):
    """x [N][C][H][W]: a contiguous float32 CUDA tensor; pads = (wl, wr, hl, hr), non-negative integers, last axis first as
    torch.nn.functional.pad orders them.  Returns out [N][C][H + hl + hr][W + wl + wr] with out[n, c, r, q] = x[n, c, (r - hl) mod H,
    (q - wl) mod W] (the mathematical modulo; a pad may exceed the extent).  Differentiable once in x.  The backward is a
    deterministic gather with a fixed order of addition: per padded row the cotangents of a source column's copies are added in
    ascending q, then the rows of a source row in ascending r, each sum starting from its first term -- the same bits from run to
    run; with at most two copies per axis (every pad of the trainer's recipes) the value of trainer._PeriodicPad's index_add_ chain."""
    _check_input("periodic_pad", "x", x)
    pads = tuple(int(p) for p in pads)
    if len(pads) != 4 or min(pads) < 0:
        raise ValueError(f"periodic_pad: pads must be four non-negative integers (wl, wr, hl, hr) (got {pads})")
    if (x.shape[0] * x.shape[1]) * (x.shape[2] + pads[2] + pads[3]) * (x.shape[3] + pads[0] + pads[1]) >= 2 ** 31:
        raise ValueError(f"periodic_pad: at most 2^31 - 1 padded elements per call (got {tuple(x.shape)} with pads {pads})")
    if x.device.type != "cuda":
        raise _lib.RadonLibraryError("periodic_pad: x must be a CUDA tensor; there is no CPU path")
    return _FusedPeriodicPad.apply(x, pads)


def maxout(y):
    """y [N][2C][H][W]: a contiguous float32 CUDA tensor, the two convolutions of a ConvBlock side by side on the channel axis.  Returns
    out [N][C][H][W] = where(first, y[:, :C], y[:, C:]) with first = y[:, :C] >= y[:, C:]: a tie takes the first half (TensorFlow's
    MaximumGrad), a NaN in either half makes the comparison false and takes the second half, -0.0 >= +0.0 is true.  Differentiable
    once in y: the cotangent goes to the half that was taken and +0 to the other, by selection (an infinite cotangent gives inf and 0,
    where g * first gives inf and NaN).  The backward keeps one byte per output element, never a copy of y."""
    _check_input("maxout", "y", y)
    if y.shape[1] % 2 != 0:
        raise ValueError(f"maxout: y needs an even channel count, the two convolutions' halves (got {tuple(y.shape)})")
    if y.numel() >= 2 ** 31:
        raise ValueError(f"maxout: at most 2^31 - 1 elements per call (got {tuple(y.shape)})")
    if y.device.type != "cuda":
        raise _lib.RadonLibraryError("maxout: y must be a CUDA tensor; there is no CPU path")
    return _FusedMaxout.apply(y)
