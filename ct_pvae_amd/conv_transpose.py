"""The transposed convolution of an up-sampling ConvBlock with its maxout behind as ONE forward launch and at most three backward
launches on the matrix cores (csrc/conv_transpose.hip states every sum's one order: the kernels give the same bits from run to run,
with no switch to set and no atomics).

    conv_transpose_maxout(x, weight, bias, stride, padding, output_padding)
        x [N][Cin][H][W], weight [Cin][2C][k][k] and bias [2C] (a transposed ConvBlock's ab.weight / ab.bias, read where the module
        keeps them) -> out [N][C][OH][OW] = maxout(conv_transpose2d(x, weight, bias, stride, padding, output_padding))

The convolution's 2C-channel result is never written to memory; the backward keeps x, weight and one byte per output element.  There
is no CPU path."""
import torch

from . import _lib, forward_functions
from .forward_functions import _stream_ptr

__all__ = ["conv_transpose_maxout"]


def _check_tensor(name, t, dim):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"conv_transpose_maxout: {name} must be a torch tensor (got {type(t).__name__})")
    if t.dtype is not torch.float32:
        raise TypeError(f"conv_transpose_maxout: {name} must be float32 (got {t.dtype})")
    if t.dim() != dim or t.numel() == 0:
        raise ValueError(f"conv_transpose_maxout: {name} must be a non-empty tensor of {dim} axes (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"conv_transpose_maxout: {name} must be contiguous (got strides {tuple(t.stride())})")


def _geometry(x, weight, bias, stride, padding, output_padding):
    """The nine integers of the C ABI, (N, Cin, H, W, C, k, s, pad, opad), and the output's (OH, OW); every check that needs no device,
    before any launch."""
    _check_tensor("x", x, 4)
    _check_tensor("weight", weight, 4)
    _check_tensor("bias", bias, 1)
    for name, v in (("stride", stride), ("padding", padding), ("output_padding", output_padding)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"conv_transpose_maxout: {name} must be a Python int (got {type(v).__name__})")
    N, Cin, H, W = x.shape
    C2, k = weight.shape[1], weight.shape[2]
    if C2 % 2 != 0 or tuple(weight.shape) != (Cin, C2, k, k):
        raise ValueError(f"conv_transpose_maxout: weight must be [Cin = {Cin}][2C][k][k], the two convolutions' halves on axis 1 (got "
                         f"{tuple(weight.shape)})")
    if tuple(bias.shape) != (C2,):
        raise ValueError(f"conv_transpose_maxout: bias must be [2C = {C2}] (got {tuple(bias.shape)})")
    if not 1 <= k <= 8:
        raise ValueError(f"conv_transpose_maxout: the kernel size must be in 1 .. 8 (got {k})")
    if not 1 <= stride <= k:
        raise ValueError(f"conv_transpose_maxout: the stride must be in 1 .. k = {k} (got {stride})")
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


def _forward(x, weight, bias, geom, hw):
    N, C = geom[0], geom[4]
    out = forward_functions._new_output((N, C) + hw, torch.float32, x.device)
    first = torch.empty((N, C) + hw, dtype=torch.uint8, device=x.device)     # (saved state, every byte written by the launch)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ctpvae_convt_fwd_f32(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), *geom, out.data_ptr(), first.data_ptr(),
                                                    _stream_ptr()), "convt_fwd")
    return out, first


class _ConvTransposeMaxout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geom, hw):
        out, first = _forward(x, weight, bias, geom, hw)
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
        N, Cin, H, W, C = geom[:5]
        g = g.to(torch.float32).contiguous()
        lib = _lib.load()
        gx = gw = gb = None
        with torch.cuda.device(g.device):
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                ws = torch.empty(_lib.check(lib.ctpvae_convt_wgrad_workspace_bytes(*geom), "convt_wgrad_workspace_bytes") // 4,
                                 dtype=torch.float32, device=g.device)
                gw = forward_functions._new_output(tuple(weight.shape), torch.float32, g.device)
                gb = forward_functions._new_output((2 * C,), torch.float32, g.device)
                _lib.check(lib.ctpvae_convt_bwd_weight_f32(x.data_ptr(), g.data_ptr(), first.data_ptr(), *geom, ws.data_ptr(), gw.data_ptr(),
                                                           gb.data_ptr(), _stream_ptr()), "convt_bwd_weight")
            if ctx.needs_input_grad[0]:
                gx = forward_functions._new_output((N, Cin, H, W), torch.float32, g.device)
                _lib.check(lib.ctpvae_convt_bwd_input_f32(g.data_ptr(), first.data_ptr(), weight.data_ptr(), *geom, gx.data_ptr(),
                                                          _stream_ptr()), "convt_bwd_input")
        return (gx, gw if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None, None)


def _require_cuda(x, weight, bias):
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t.device.type != "cuda":
            raise _lib.RadonLibraryError(f"conv_transpose_maxout: {name} must be a CUDA tensor; there is no CPU path")
        if t.device != x.device:
            raise ValueError(f"conv_transpose_maxout: {name} is on {t.device}, x on {x.device}")


def _conv_transpose_maxout_with_first(x, weight, bias, stride, padding, output_padding):
    """(out, first) of the forward launch, detached: first [N][C][OH][OW], uint8, 1 where the first channel half was taken (a tie
    takes it, a NaN on either side does not).  For tests and tools that read the selection; arguments as conv_transpose_maxout's."""
    geom, hw = _geometry(x, weight, bias, stride, padding, output_padding)
    _require_cuda(x, weight, bias)
    return _forward(x.detach(), weight.detach(), bias.detach(), geom, hw)


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
    _require_cuda(x, weight, bias)
    return _ConvTransposeMaxout.apply(x, weight, bias, geom, hw)
