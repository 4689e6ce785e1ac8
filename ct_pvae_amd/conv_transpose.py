"""The transposed convolution of an up-sampling ConvBlock with its maxout behind as ONE forward launch and at most three backward
launches on the matrix cores (csrc/conv_transpose.hip states every sum's one order: the kernels give the same bits from run to run,
with no switch to set and no atomics).

    conv_transpose_maxout(x, weight, bias, stride, padding, output_padding)
        x [N][Cin][H][W], weight [Cin][2C][k][k] and bias [2C] (a transposed ConvBlock's ab.weight / ab.bias, read where the module
        keeps them) -> out [N][C][OH][OW] = maxout(conv_transpose2d(x, weight, bias, stride, padding, output_padding))

The convolution's 2C-channel result is never written to memory; the backward keeps x, weight and one byte per output element.  There
is no CPU path."""
import torch

from . import _conv_common as common
from . import _lib, forward_functions
from .forward_functions import _stream_ptr

__all__ = ["conv_transpose_maxout"]


WHAT, PREFIX = "conv_transpose_maxout", "convt"     # the operator's name in messages, the stem of its C symbols


def _geometry(x, weight, bias, stride, padding, output_padding):
    """The nine integers of the C ABI, (N, Cin, H, W, C, k, s, pad, opad), and the output's (OH, OW); every check that needs no device,
    before any launch."""
    common.check_tensors(WHAT, x, weight, bias)
    common.check_ints(WHAT, stride=stride, padding=padding, output_padding=output_padding)
    N, Cin, H, W = x.shape
    C2, k = weight.shape[1], weight.shape[2]
    if C2 % 2 != 0 or tuple(weight.shape) != (Cin, C2, k, k):
        raise ValueError(f"conv_transpose_maxout: weight must be [Cin = {Cin}][2C][k][k], the two convolutions' halves on axis 1 (got "
                         f"{tuple(weight.shape)})")
    if tuple(bias.shape) != (C2,):
        raise ValueError(f"conv_transpose_maxout: bias must be [2C = {C2}] (got {tuple(bias.shape)})")
    common.check_kernel_and_stride(WHAT, k, stride)
    if not 0 <= padding < k:
        raise ValueError(f"conv_transpose_maxout: the padding must be in 0 .. k - 1 = {k - 1} (got {padding})")
    if not 0 <= output_padding < stride:
        raise ValueError(f"conv_transpose_maxout: the output padding must be in 0 .. stride - 1 = {stride - 1} (got {output_padding})")
    OH = (H - 1) * stride - 2 * padding + k + output_padding
    OW = (W - 1) * stride - 2 * padding + k + output_padding
    if OH < 1 or OW < 1:
        raise ValueError(f"conv_transpose_maxout: the output ({OH} x {OW}) must have at least one pixel")
    if max(N * Cin * H * W, N * C2 * OH * OW, Cin * C2 * k * k) >= 2 ** 31:
        raise ValueError(f"conv_transpose_maxout: at most 2^31 - 1 elements per tensor (got x {tuple(x.shape)}, weight "
                         f"{tuple(weight.shape)}, output {OH} x {OW})")
    return (N, Cin, H, W, C2 // 2, k, stride, padding, output_padding), (OH, OW)


class _ConvTransposeMaxout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geom, hw):
        out, first = common.forward(PREFIX, x, weight, bias, geom, hw)
        ctx.save_for_backward(x, weight, first)       # never the 2C-channel result
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
        g = g.to(torch.float32).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = common.weight_grad(PREFIX, x, g, first, weight, geom)
        if ctx.needs_input_grad[0]:
            with torch.cuda.device(g.device):
                gx = forward_functions._new_output(tuple(x.shape), torch.float32, g.device)
                _lib.check(_lib.load().ctpvae_convt_bwd_input_f32(g.data_ptr(), first.data_ptr(), weight.data_ptr(), *geom, gx.data_ptr(),
                                                                  _stream_ptr()), "convt_bwd_input")
        return (gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None, None)


def _conv_transpose_maxout_with_first(x, weight, bias, stride, padding, output_padding):
    """(out, first) of the forward launch, detached: first [N][C][OH][OW], uint8, 1 where the first channel half was taken (a tie
    takes it, a NaN on either side does not).  For tests and tools that read the selection; arguments as conv_transpose_maxout's."""
    geom, hw = _geometry(x, weight, bias, stride, padding, output_padding)
    common.require_cuda(WHAT, x, weight, bias)
    return common.forward(PREFIX, x.detach(), weight.detach(), bias.detach(), geom, hw)


def conv_transpose_maxout(x, weight, bias, stride, padding, output_padding):
    """x [N][Cin][H][W], weight [Cin][2C][k][k], bias [2C]: contiguous float32 CUDA tensors; stride, padding and output_padding Python
    ints, 1 <= stride <= k <= 8, 0 <= padding < k, 0 <= output_padding < stride.  Returns out [N][C][OH][OW], OH = (H - 1) * stride -
    2 * padding + k + output_padding: y[n, c2, oy, ox] is ONE float32 fmaf chain from bias[c2] over ci, kh, kw ascending of x[n, ci,
    (oy + padding - kh) / stride, (ox + padding - kw) / stride] * weight[ci, c2, kh, kw] over the taps where stride divides both
    numerators (a source outside the image enters as +0), and out = where(y[:, :C] >= y[:, C:], y[:, :C], y[:, C:]) -- a tie takes the
    first half, a NaN on either side the second.  An object's result does not depend on the other objects of the call.
    Differentiable once in x, weight and bias, each only where it is needed; the cotangent goes to the half that was taken by
    selection; the weight gradient's sum over the N * H * W input pixels and the bias gradient's over the N * OH * OW output pixels
    are cut into chunks of 1024 by the shapes alone, so every gradient has the same bits on every run (csrc/conv_transpose.hip)."""
    geom, hw = _geometry(x, weight, bias, stride, padding, output_padding)
    common.require_cuda(WHAT, x, weight, bias)
    return _ConvTransposeMaxout.apply(x, weight, bias, geom, hw)
