"""The P-VAE decoder's TruncatedNormal output head as one forward and one backward launch (csrc/head.hip states the function, the
layout of the random numbers, the order of the per-object sum and what the backward re-evaluates).

    truncated_normal_head(alpha, beta, *, seed, draw, first_object=0)   (x [n][X][Y][1], LP [n]): the reparameterised sample of
                                                                        TruncatedNormal(pr(alpha), pr(beta), 0, 1e10) and the
                                                                        per-object sum of its log-density at that sample
    head_uniforms(n, pix, *, seed, draw, first_object=0)                the uniforms the kernels draw, on the host (no GPU needed)

There is no CPU path."""
import numpy as np
import torch

from . import _lib, forward_functions
from ._args import check_float32
from .forward_functions import _stream_ptr

__all__ = ["truncated_normal_head", "head_uniforms"]


def _counter_args(seed, draw, first_object):
    seed, draw, first_object = int(seed), int(draw), int(first_object)
    if not 0 <= draw < 2 ** 32:
        raise ValueError(f"draw is one 32-bit counter word: 0 <= draw < 2^32 (got {draw})")
    if not 0 <= first_object < 2 ** 63:
        raise ValueError(f"first_object must be >= 0 (got {first_object})")
    return seed & (2 ** 64 - 1), draw, first_object


def head_uniforms(n, pix, *, seed, draw, first_object=0):
    """float32 numpy array [n][pix]: u of pixel `pixel` of object o is word e & 3 of Philox4x32-10((lo32(e >> 2), hi32(e >> 2), draw,
    0x544E48), key = seed), e = (first_object + o) * pix + pixel, as ((w >> 8) + 0.5f) * 2^-24."""
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    n, pix = int(n), int(pix)
    if n < 1 or pix < 1:
        raise ValueError(f"head_uniforms: n and pix must be positive (got {n}, {pix})")
    out = np.empty((n, pix), np.float32)
    _lib.check(_lib.load().ctpvae_tn_head_uniforms_host_f32(n, pix, first_object, seed, draw, out.ctypes.data), "tn_head_uniforms_host")
    return out


def _check_input(name, t):
    check_float32("truncated_normal_head", name, t, 4, "[n][1][X][Y], the decoder's layout", lambda shape: shape[1] == 1)


class _TruncatedNormalHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, beta, seed, draw, first_object, u):
        n, _, X, Y = alpha.shape
        a, b = alpha.detach(), beta.detach()
        # [n][1][X][Y] with one channel IS the projector's [n][X][Y][1], byte for byte
        x = forward_functions._new_output((n, X, Y, 1), torch.float32, alpha.device)
        lp_sum = forward_functions._new_output((n,), torch.float32, alpha.device)
        with torch.cuda.device(alpha.device):
            _lib.check(_lib.load().ctpvae_tn_head_fwd_f32(a.data_ptr(), b.data_ptr(), n, X * Y, first_object, seed, draw,
                                                          u.data_ptr() if u is not None else None, x.data_ptr(), lp_sum.data_ptr(),
                                                          None, _stream_ptr()), "tn_head_fwd")
        ctx.save_for_backward(a, b)
        ctx.u, ctx.counter = u, (first_object, seed, draw)
        ctx.set_materialize_grads(False)
        return x, lp_sum

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x, g_lp):
        a, b = ctx.saved_tensors
        if g_x is None and g_lp is None:
            return None, None, None, None, None, None
        n, pix = a.shape[0], a.shape[2] * a.shape[3]
        if g_x is not None:
            g_x = g_x.to(torch.float32).contiguous()
        if g_lp is not None:
            g_lp = g_lp.to(torch.float32).contiguous()
        g_alpha = forward_functions._new_output(tuple(a.shape), torch.float32, a.device)
        g_beta = forward_functions._new_output(tuple(a.shape), torch.float32, a.device)
        with torch.cuda.device(a.device):
            _lib.check(_lib.load().ctpvae_tn_head_bwd_f32(a.data_ptr(), b.data_ptr(), n, pix, *ctx.counter,
                                                          ctx.u.data_ptr() if ctx.u is not None else None,
                                                          g_x.data_ptr() if g_x is not None else None,
                                                          g_lp.data_ptr() if g_lp is not None else None,
                                                          g_alpha.data_ptr(), g_beta.data_ptr(), _stream_ptr()), "tn_head_bwd")
        return g_alpha, g_beta, None, None, None, None


def truncated_normal_head(alpha, beta, *, seed, draw, first_object=0, _u=None):
    """alpha, beta [n][1][X][Y]: contiguous float32 CUDA tensors, the decoder's raw outputs.  Returns (x [n][X][Y][1], LP [n]): x the
    reparameterised sample of TruncatedNormal(positive_range(alpha), positive_range(beta), low=0, high=1e10) in the projector's layout,
    LP[o] the sum over object o of log_prob(x), added in a fixed order (the same bits from run to run, whatever n and first_object).
    The uniforms depend on (seed, draw, (first_object + o) * X * Y + pixel) alone: pass the step index as `draw` and the batch
    offset as `first_object`, and a batch cut over calls or ranks draws what the whole batch draws.  Differentiable once in alpha and
    beta, through both outputs.  _u [n][1][X][Y] (tests) replaces the generator's uniforms."""
    _check_input("alpha", alpha)
    _check_input("beta", beta)
    if beta.shape != alpha.shape:
        raise ValueError(f"truncated_normal_head: alpha and beta must have one shape (got {tuple(alpha.shape)}, {tuple(beta.shape)})")
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    if alpha.numel() >= 2 ** 31:
        raise ValueError(f"truncated_normal_head: at most 2^31 - 1 pixels per call (got {alpha.numel()})")
    if alpha.device.type != "cuda" or beta.device != alpha.device:
        raise _lib.RadonLibraryError("truncated_normal_head: alpha and beta must be CUDA tensors on one device; there is no CPU path")
    if _u is not None:
        _check_input("_u", _u)
        if _u.shape != alpha.shape or _u.device != alpha.device:
            raise ValueError("truncated_normal_head: _u must have alpha's shape and device")
        _u = _u.detach()
    return _TruncatedNormalHead.apply(alpha, beta, seed, draw, first_object, _u)
