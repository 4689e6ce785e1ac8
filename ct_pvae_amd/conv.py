"""The convolution of a padded (non-transposed) ConvBlock with its periodic padding in front and its maxout behind as ONE forward
launch and at most four backward launches on the matrix cores (csrc/conv.hip states every sum's one order: the kernels give the same
bits from run to run, with no switch to set and no atomics).

    periodic_conv_maxout(x, weight, bias, stride, pads)
        x [N][Cin][H][W], weight [2C][Cin][k][k] and bias [2C] (a ConvBlock's ab.weight / ab.bias), pads = (wl, wr, hl, hr) as
        ConvBlock.forward builds them -> out [N][C][OH][OW] = maxout(conv2d(periodic_pad(x, pads), weight, bias, stride))

The padded input and the convolution's 2C-channel result are never written to memory; the backward keeps x, weight and one byte per
output element.  There is no CPU path."""
import torch

from . import _conv_common as common
from . import _lib, forward_functions
from .forward_functions import _stream_ptr

__all__ = ["periodic_conv_maxout"]


WHAT, PREFIX = "periodic_conv_maxout", "conv"     # the operator's name in messages, the stem of its C symbols


def _geometry(x, weight, bias, stride, pads):
    """The eleven integers of the C ABI, (N, Cin, H, W, C, k, s, wl, wr, hl, hr), and the output's (OH, OW); every check that needs no
    device, before any launch."""
    common.check_tensors(WHAT, x, weight, bias)
    common.check_ints(WHAT, stride=stride)
    pads = tuple(int(p) for p in pads)
    if len(pads) != 4 or min(pads) < 0:
        raise ValueError(f"periodic_conv_maxout: pads must be four non-negative integers (wl, wr, hl, hr) (got {pads})")
    N, Cin, H, W = x.shape
    C2, k = weight.shape[0], weight.shape[2]
    if C2 % 2 != 0 or tuple(weight.shape) != (C2, Cin, k, k):
        raise ValueError(f"periodic_conv_maxout: weight must be [2C][Cin = {Cin}][k][k], the two convolutions' halves (got {tuple(weight.shape)})")
    if tuple(bias.shape) != (C2,):
        raise ValueError(f"periodic_conv_maxout: bias must be [2C = {C2}] (got {tuple(bias.shape)})")
    common.check_kernel_and_stride(WHAT, k, stride)
    wl, wr, hl, hr = pads
    PH, PW = H + hl + hr, W + wl + wr
    if PH < k or PW < k:
        raise ValueError(f"periodic_conv_maxout: the padded image ({PH} x {PW}) must hold one window of {k} x {k}")
    OH, OW = (PH - k) // stride + 1, (PW - k) // stride + 1
    if max(N * Cin * PH * PW, N * C2 * OH * OW, C2 * (Cin * k * k + 1)) >= 2 ** 31:
        raise ValueError(f"periodic_conv_maxout: at most 2^31 - 1 elements per tensor (got x {tuple(x.shape)}, weight "
                         f"{tuple(weight.shape)}, pads {pads})")
    return (N, Cin, H, W, C2 // 2, k, stride, wl, wr, hl, hr), (OH, OW)


class _PeriodicConvMaxout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geom, hw):
        out, first = common.forward(PREFIX, x, weight, bias, geom, hw)
        ctx.save_for_backward(x, weight, first)       # never the 2C-channel result or a padded copy
        ctx.geom = geom
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None
        x, weight, first = ctx.saved_tensors
        geom = ctx.geom
        N, Cin, H, W, _, _, _, wl, wr, hl, hr = geom
        g = g.to(torch.float32).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = common.weight_grad(PREFIX, x, g, first, weight, geom)
        if ctx.needs_input_grad[0]:
            lib = _lib.load()
            with torch.cuda.device(g.device):
                gp = forward_functions._new_output((N, Cin, H + hl + hr, W + wl + wr), torch.float32, g.device)
                _lib.check(lib.ctpvae_conv_bwd_input_f32(g.data_ptr(), first.data_ptr(), weight.data_ptr(), *geom, gp.data_ptr(),
                                                         _stream_ptr()), "conv_bwd_input")
                gx = forward_functions._new_output((N, Cin, H, W), torch.float32, g.device)
                _lib.check(lib.ctpvae_periodic_pad_bwd_f32(gp.data_ptr(), N * Cin, H, W, wl, wr, hl, hr, gx.data_ptr(), _stream_ptr()),
                           "periodic_pad_bwd")
        return (gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None, None)


def _conv_maxout_with_first(x, weight, bias, stride, pads):
    """(out, first) of the forward launch, detached: first [N][C][OH][OW], uint8, 1 where the first channel half was taken (a tie
    takes it, a NaN on either side does not).  For tests and tools that read the selection; arguments as periodic_conv_maxout's."""
    geom, hw = _geometry(x, weight, bias, stride, pads)
    common.require_cuda(WHAT, x, weight, bias)
    return common.forward(PREFIX, x.detach(), weight.detach(), bias.detach(), geom, hw)


def periodic_conv_maxout(x, weight, bias, stride, pads):
    """x [N][Cin][H][W], weight [2C][Cin][k][k], bias [2C]: contiguous float32 CUDA tensors; stride a Python int, 1 <= stride <= k <= 8;
    pads = (wl, wr, hl, hr), non-negative integers, last axis first.  Returns out [N][C][OH][OW], OH = (H + hl + hr - k) // stride + 1:
    with xp[n, ci, r, q] = x[n, ci, (r - hl) mod H, (q - wl) mod W], y[n, c2, oh, ow] is ONE float32 fmaf chain from bias[c2] over ci, kh,
    kw ascending of xp[n, ci, oh * stride + kh, ow * stride + kw] * weight[c2, ci, kh, kw], and out = where(y[:, :C] >= y[:, C:], y[:, :C],
    y[:, C:]) -- a tie takes the first half, a NaN on either side the second.  An object's result does not depend on the other objects
    of the call.  Differentiable once in x, weight and bias, each only where it is needed; the cotangent goes to the half that was
    taken by selection; the weight gradient's sum over the N * OH * OW output pixels is cut into chunks of 1024 by the shapes alone, so
    every gradient has the same bits on every run (csrc/conv.hip)."""
    geom, hw = _geometry(x, weight, bias, stride, pads)
    common.require_cuda(WHAT, x, weight, bias)
    return _PeriodicConvMaxout.apply(x, weight, bias, geom, hw)
