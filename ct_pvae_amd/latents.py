"""The P-VAE's Normal latent block at one skip level as one forward and one backward launch (csrc/latent.hip states the function, the
layout of the random numbers, the order of the per-object sum and what the backward regenerates).

    normal_latents(skip, *, ns, seed, draw, level, first_object=0, sqrt_reg=EPS32)   (z [ns * B][C][H][W], KL [B]): the ns
                                                                        reparameterised samples of Normal(loc, pr(log_scale) + sqrt_reg),
                                                                        sample-major, and the per-object sum of KL(. || N(0, 1))
    latent_draws(n, length, *, ns, seed, draw, level, first_object=0)   the signed tail probabilities v the kernels draw, on the host
                                                                        (no GPU needed): eps = copysign(-ndtri(|v|), v)

There is no CPU path."""
import numpy as np
import torch

from . import _lib, forward_functions
from ._args import check_float32
from .forward_functions import _stream_ptr
from .output_head import _counter_args

__all__ = ["normal_latents", "latent_draws"]

EPS32 = float(np.finfo(np.float32).eps)


def _key_args(ns, level):
    ns, level = int(ns), int(level)
    if not 1 <= ns <= 65535:
        raise ValueError(f"ns shares a counter word with the level: 1 <= ns <= 65535 (got {ns})")
    if not 0 <= level <= 255:
        raise ValueError(f"level is one byte of a counter word: 0 <= level <= 255 (got {level})")
    return ns, level


def latent_draws(n, length, *, ns, seed, draw, level, first_object=0):
    """float32 numpy array [ns][n][length]: v of element i of object b, sample s, is +-t with t = (((w >> 7) & 0xFFFFFF) + 0.5f) * 2^-25,
    negative when bit 31 of w is set; w is word e & 3 of Philox4x32-10((lo32(e >> 2), hi32(e >> 2), draw, 0x4C000000 | level << 16 | s),
    key = seed), e = (first_object + b) * length + i.  The kernels' eps is copysign(-ndtri(|v|), v)."""
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    ns, level = _key_args(ns, level)
    n, length = int(n), int(length)
    if n < 1 or length < 1:
        raise ValueError(f"latent_draws: n and length must be positive (got {n}, {length})")
    out = np.empty((ns, n, length), np.float32)
    _lib.check(_lib.load().ctpvae_latent_draws_host_f32(n, length, ns, first_object, seed, draw, level, out.ctypes.data), "latent_draws_host")
    return out


def _check_input(name, t):
    check_float32("normal_latents", name, t, 4, "[B][channels][H][W], the encoder's layout")


class _NormalLatents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, skip, ns, sqrt_reg, seed, draw, level, first_object, eps):
        B, C2, H, W = skip.shape
        length = (C2 // 2) * H * W
        sk = skip.detach()
        z = forward_functions._new_output((ns * B, C2 // 2, H, W), torch.float32, skip.device)
        kl = forward_functions._new_output((B,), torch.float32, skip.device)
        with torch.cuda.device(skip.device):
            _lib.check(_lib.load().ctpvae_latent_fwd_f32(sk.data_ptr(), B, length, ns, sqrt_reg, first_object, seed, draw, level,
                                                         eps.data_ptr() if eps is not None else None, z.data_ptr(), kl.data_ptr(),
                                                         None, None, _stream_ptr()), "latent_fwd")
        ctx.save_for_backward(sk)
        ctx.eps, ctx.key = eps, (ns, sqrt_reg, first_object, seed, draw, level)
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
            _lib.check(_lib.load().ctpvae_latent_bwd_f32(sk.data_ptr(), B, (C2 // 2) * H * W, *ctx.key,
                                                         ctx.eps.data_ptr() if ctx.eps is not None else None,
                                                         g_z.data_ptr() if g_z is not None else None,
                                                         g_kl.data_ptr() if g_kl is not None else None,
                                                         g_skip.data_ptr(), _stream_ptr()), "latent_bwd")
        return (g_skip,) + (None,) * 7


def normal_latents(skip, *, ns, seed, draw, level, first_object=0, sqrt_reg=EPS32, _eps=None):
    """skip [B][2C][H][W]: a contiguous float32 CUDA tensor, the encoder's output at one level (channels 0 .. C-1: loc, the rest:
    log_scale).  Returns (z [ns * B][C][H][W], KL [B]): z[s * B + b] = loc[b] + scale[b] * eps(s, b), scale = positive_range(log_scale) +
    sqrt_reg, sample-major as the decoder is fed; KL[b] the sum over object b of 0.5 (scale^2 + loc^2 - 1) - log scale, added in a fixed
    order (the same bits from run to run, whatever B and first_object).  eps depends on (seed, draw, level, s, (first_object + b), element)
    alone: pass the step index as `draw` and the GLOBAL batch offset as `first_object`, and a batch cut over calls or ranks draws what
    the whole batch draws, for any ns.  Differentiable once in skip, through both outputs.  _eps [ns * B][C][H][W] (tests) replaces the
    generator's draws."""
    _check_input("skip", skip)
    if skip.shape[1] % 2 != 0:
        raise ValueError(f"normal_latents: skip needs an even channel count, loc then log_scale (got {tuple(skip.shape)})")
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    ns, level = _key_args(ns, level)
    if ns * (skip.numel() // 2) >= 2 ** 31:
        raise ValueError(f"normal_latents: at most 2^31 - 1 samples per call (got {ns} x {skip.numel() // 2})")
    if _eps is not None:
        _check_input("_eps", _eps)
        if tuple(_eps.shape) != (ns * skip.shape[0], skip.shape[1] // 2) + tuple(skip.shape[2:]) or _eps.device != skip.device:
            raise ValueError("normal_latents: _eps must be [ns * B][C][H][W] on skip's device")
        _eps = _eps.detach()
    if skip.device.type != "cuda":
        raise _lib.RadonLibraryError("normal_latents: skip must be a CUDA tensor; there is no CPU path")
    return _NormalLatents.apply(skip, ns, float(sqrt_reg), seed, draw, level, first_object, _eps)
