"""The P-VAE decoder's default Beta output head as one forward and one backward launch (csrc/beta_head.hip states the function, the
layout of the random numbers, the order of the per-object sum and what the backward re-evaluates).

    beta_head(alpha, beta, *, seed, draw, first_object=0, sqrt_reg=EPS32)   (x [n][X][Y][1], LP [n]): the reparameterised sample of
                                                                            Beta(pr(alpha), pr(beta)) and the per-object sum of its
                                                                            log-density at clamp(x, sqrt_reg, 1 - sqrt_reg)
    beta_head_words(n, pix, *, seed, draw, first_object=0, gamma, attempt)  the Philox words of one (gamma, attempt), on the host

There is no CPU path."""
import numpy as np
import torch

from . import _lib, forward_functions
from ._args import check_float32
from .forward_functions import _stream_ptr
from .output_head import _counter_args

__all__ = ["beta_head", "beta_head_words"]

EPS32 = float(np.finfo(np.float32).eps)


def beta_head_words(n, pix, *, seed, draw, first_object=0, gamma, attempt):
    """uint32 numpy array [n][pix][4]: the block Philox4x32-10((lo32(e), hi32(e), draw, 0x42000000 | gamma << 8 | attempt), key = seed),
    e = (first_object + o) * pix + pixel.  Attempt `attempt` of gamma `gamma` (0: alpha's, 1: beta's) takes zn = ndtri(u24(word 0)),
    ua = u24(word 1), ub = u24(word 2)."""
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    n, pix, gamma, attempt = int(n), int(pix), int(gamma), int(attempt)
    if n < 1 or pix < 1:
        raise ValueError(f"beta_head_words: n and pix must be positive (got {n}, {pix})")
    if gamma not in (0, 1) or not 0 <= attempt < 16:
        raise ValueError(f"beta_head_words: gamma must be 0 or 1 and 0 <= attempt < 16 (got {gamma}, {attempt})")
    out = np.empty((n, pix, 4), np.uint32)
    _lib.check(_lib.load().ctpvae_beta_head_words_host_u32(n, pix, first_object, seed, draw, gamma, attempt, out.ctypes.data),
               "beta_head_words_host")
    return out


def _check_input(name, t):
    check_float32("beta_head", name, t, 4, "[n][1][X][Y], the decoder's layout", lambda shape: shape[1] == 1)


class _BetaHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, beta, seed, draw, first_object, sqrt_reg):
        n, _, X, Y = alpha.shape
        a, b = alpha.detach(), beta.detach()
        # [n][1][X][Y] with one channel IS the projector's [n][X][Y][1], byte for byte
        x = forward_functions._new_output((n, X, Y, 1), torch.float32, alpha.device)
        lp_sum = forward_functions._new_output((n,), torch.float32, alpha.device)
        with torch.cuda.device(alpha.device):
            _lib.check(_lib.load().ctpvae_beta_head_fwd_f32(a.data_ptr(), b.data_ptr(), n, X * Y, first_object, seed, draw, sqrt_reg,
                                                            x.data_ptr(), lp_sum.data_ptr(), None, None, _stream_ptr()), "beta_head_fwd")
        ctx.save_for_backward(a, b)
        ctx.counter = (first_object, seed, draw, sqrt_reg)
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
            _lib.check(_lib.load().ctpvae_beta_head_bwd_f32(a.data_ptr(), b.data_ptr(), n, pix, *ctx.counter,
                                                            g_x.data_ptr() if g_x is not None else None,
                                                            g_lp.data_ptr() if g_lp is not None else None,
                                                            g_alpha.data_ptr(), g_beta.data_ptr(), _stream_ptr()), "beta_head_bwd")
        return g_alpha, g_beta, None, None, None, None


def beta_head(alpha, beta, *, seed, draw, first_object=0, sqrt_reg=EPS32):
    """alpha, beta [n][1][X][Y]: contiguous float32 CUDA tensors, the decoder's raw outputs.  Returns (x [n][X][Y][1], LP [n]): x the
    reparameterised sample of Beta(positive_range(alpha), positive_range(beta)) in the projector's layout (not clamped), LP[o] the sum
    over object o of log_prob(clamp(x, sqrt_reg, 1 - sqrt_reg)), added in a fixed order (the same bits from run to run, whatever n and
    first_object).  The draws depend on (seed, draw, (first_object + o) * X * Y + pixel) alone: pass the step index as `draw` and the
    batch offset as `first_object`, and a batch cut over calls or ranks draws what the whole batch draws.  Differentiable once in alpha
    and beta, through both outputs: the implicit reparameterisation gradient of the two gammas (TensorFlow's, not torch's direct Beta
    derivative)."""
    _check_input("alpha", alpha)
    _check_input("beta", beta)
    if beta.shape != alpha.shape:
        raise ValueError(f"beta_head: alpha and beta must have one shape (got {tuple(alpha.shape)}, {tuple(beta.shape)})")
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    sqrt_reg = float(sqrt_reg)
    if not 0.0 < sqrt_reg < 0.5:
        raise ValueError(f"beta_head: sqrt_reg must lie in (0, 0.5) (got {sqrt_reg})")
    if alpha.numel() >= 2 ** 31:
        raise ValueError(f"beta_head: at most 2^31 - 1 pixels per call (got {alpha.numel()})")
    if alpha.device.type != "cuda" or beta.device != alpha.device:
        raise _lib.RadonLibraryError("beta_head: alpha and beta must be CUDA tensors on one device; there is no CPU path")
    return _BetaHead.apply(alpha, beta, seed, draw, first_object, sqrt_reg)
