"""What the wrappers of the four fused sampling operators share (output_head.py: `op` "truncated_normal_head", symbol stem "tn_head";
beta_head.py: "beta_head", "beta_head"; latents.py: "normal_latents", "latent"; beta_latents.py: "beta_latents", "beta_latent"): the
checks every call makes before it looks at a device, in one order, and the two launches behind an autograd.Function, whose arguments
differ only in what each C entry point has between the sizes and the outputs.  Every C symbol is fetched from _lib.load() by name when
it is called."""
import numpy as np
import torch

from . import _lib, forward_functions
from ._args import check_float32, counter_args
from .forward_functions import _stream_ptr

EPS32 = float(np.finfo(np.float32).eps)


def _ptr(t):
    """A tensor's address, or None: a null pointer."""
    return None if t is None else t.data_ptr()


def key_args(ns, level, max_ns, ns_message):
    ns, level = int(ns), int(level)
    if not 1 <= ns <= max_ns:
        raise ValueError(f"{ns_message}: 1 <= ns <= {max_ns} (got {ns})")
    if not 0 <= level <= 255:
        raise ValueError(f"level is one byte of a counter word: 0 <= level <= 255 (got {level})")
    return ns, level


def require_cuda(op, what, *tensors):
    for t in tensors:
        if t.device.type != "cuda" or t.device != tensors[0].device:
            raise _lib.RadonLibraryError(f"{op}: {what}; there is no CPU path")


# ---- the heads: alpha, beta [n][1][X][Y] -> x [n][X][Y][1], LP [n] -----------------------------------------------------------------
def check_head_input(op, name, t):
    check_float32(op, name, t, 4, "[n][1][X][Y], the decoder's layout", lambda shape: shape[1] == 1)


def check_head_pair(op, alpha, beta, seed, draw, first_object, sqrt_reg=None):
    """The checks of a head's call, in their order: both tensors, one shape, the counter words, sqrt_reg where the head takes one, the
    pixel limit, the device.  Returns (seed, draw, first_object) as the library takes them."""
    check_head_input(op, "alpha", alpha)
    check_head_input(op, "beta", beta)
    if beta.shape != alpha.shape:
        raise ValueError(f"{op}: alpha and beta must have one shape (got {tuple(alpha.shape)}, {tuple(beta.shape)})")
    counter = counter_args(seed, draw, first_object)
    if sqrt_reg is not None and not 0.0 < sqrt_reg < 0.5:
        raise ValueError(f"{op}: sqrt_reg must lie in (0, 0.5) (got {sqrt_reg})")
    if alpha.numel() >= 2 ** 31:
        raise ValueError(f"{op}: at most 2^31 - 1 pixels per call (got {alpha.numel()})")
    require_cuda(op, "alpha and beta must be CUDA tensors on one device", alpha, beta)
    return counter


def head_function(stem, test_outputs):
    """The autograd.Function of the head behind ctpvae_<stem>_fwd_f32 / _bwd_f32: apply(alpha, beta, seed, draw, first_object, extra),
    extra being the one argument its entry points take after the draw (a tensor: its address; None or a number: itself).  The forward
    entry point ends in `test_outputs` pointers that only tests ask for."""
    fwd, bwd, unasked = f"ctpvae_{stem}_fwd_f32", f"ctpvae_{stem}_bwd_f32", (None,) * test_outputs

    class _Head(torch.autograd.Function):
        @staticmethod
        def forward(ctx, alpha, beta, seed, draw, first_object, extra):
            n, _, X, Y = alpha.shape
            a, b = alpha.detach(), beta.detach()
            # [n][1][X][Y] with one channel IS the projector's [n][X][Y][1], byte for byte
            x = forward_functions._new_output((n, X, Y, 1), torch.float32, alpha.device)
            lp_sum = forward_functions._new_output((n,), torch.float32, alpha.device)
            ctx.extra = extra                                                   # (a tensor stays alive for the backward)
            ctx.key = (first_object, seed, draw, extra.data_ptr() if isinstance(extra, torch.Tensor) else extra)
            with torch.cuda.device(alpha.device):
                _lib.check(getattr(_lib.load(), fwd)(a.data_ptr(), b.data_ptr(), n, X * Y, *ctx.key, x.data_ptr(), lp_sum.data_ptr(), *unasked,
                                                     _stream_ptr()), f"{stem}_fwd")
            ctx.save_for_backward(a, b)
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
                _lib.check(getattr(_lib.load(), bwd)(a.data_ptr(), b.data_ptr(), n, pix, *ctx.key, _ptr(g_x), _ptr(g_lp), g_alpha.data_ptr(),
                                                     g_beta.data_ptr(), _stream_ptr()), f"{stem}_bwd")
            return g_alpha, g_beta, None, None, None, None
    return _Head


# ---- the latents: skip [B][2C][H][W] -> z [ns * B][C][H][W], KL [B] ------------------------------------------------------------------
def check_skip_input(op, name, t):
    check_float32(op, name, t, 4, "[B][channels][H][W], the encoder's layout")


def check_skip(op, skip, ns, seed, draw, level, first_object, max_ns, ns_message):
    """The checks of a latent call up to its test operands, in their order: the tensor, its channel count, the counter words, ns and
    the level, the sample limit.  Returns (ns, seed, draw, level, first_object) as the library takes them; require_cuda comes after the
    operator's own checks."""
    check_skip_input(op, "skip", skip)
    if skip.shape[1] % 2 != 0:
        raise ValueError(f"{op}: skip needs an even channel count, loc then log_scale (got {tuple(skip.shape)})")
    seed, draw, first_object = counter_args(seed, draw, first_object)
    ns, level = key_args(ns, level, max_ns, ns_message)
    if ns * (skip.numel() // 2) >= 2 ** 31:
        raise ValueError(f"{op}: at most 2^31 - 1 samples per call (got {ns} x {skip.numel() // 2})")
    return ns, seed, draw, level, first_object


class LatentsFunction(torch.autograd.Function):
    """Base of the two latents' Functions.  A subclass's forward takes EIGHT operands, skip first, and returns launch(ctx, stem, skip,
    key, ..): key is what ctpvae_<stem>_fwd_f32 / _bwd_f32 take between (skip, B, len) and their outputs, ns first, a tensor's place
    taken by its address (the subclass keeps the tensor alive on ctx)."""

    @staticmethod
    def launch(ctx, stem, skip, key, want_kl=True, extras=None):
        """(z, KL or None).  extras (tests, the Beta latents): a dict that receives kl_elem [B][len] and aux [ns * B][len][2][4]."""
        B, C2, H, W = skip.shape
        length, ns = (C2 // 2) * H * W, key[0]
        sk = skip.detach()
        z = forward_functions._new_output((ns * B, C2 // 2, H, W), torch.float32, skip.device)
        kl = forward_functions._new_output((B,), torch.float32, skip.device) if want_kl else None
        kl_elem = aux = None
        if extras is not None:                                       # tests: the per-element terms and the accepted draws
            kl_elem = forward_functions._new_output((B, length), torch.float32, skip.device) if want_kl else None
            aux = forward_functions._new_output((ns * B, length, 2, 4), torch.float32, skip.device)
            extras["kl_elem"], extras["aux"] = kl_elem, aux
        with torch.cuda.device(skip.device):
            _lib.check(getattr(_lib.load(), f"ctpvae_{stem}_fwd_f32")(sk.data_ptr(), B, length, *key, z.data_ptr(), _ptr(kl), _ptr(kl_elem),
                                                                      _ptr(aux), _stream_ptr()), f"{stem}_fwd")
        ctx.save_for_backward(sk)
        ctx.stem, ctx.key = stem, key
        ctx.set_materialize_grads(False)
        return z, kl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_z, g_kl):
        sk, = ctx.saved_tensors
        if g_z is None and g_kl is None:
            return (None,) * 8
        B, C2, H, W = sk.shape
        if g_z is not None:
            g_z = g_z.to(torch.float32).contiguous()
        if g_kl is not None:
            g_kl = g_kl.to(torch.float32).contiguous()
        g_skip = forward_functions._new_output(tuple(sk.shape), torch.float32, sk.device)
        with torch.cuda.device(sk.device):
            _lib.check(getattr(_lib.load(), f"ctpvae_{ctx.stem}_bwd_f32")(sk.data_ptr(), B, (C2 // 2) * H * W, *ctx.key, _ptr(g_z), _ptr(g_kl),
                                                                          g_skip.data_ptr(), _stream_ptr()), f"{ctx.stem}_bwd")
        return (g_skip,) + (None,) * 7
