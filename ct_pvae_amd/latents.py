"""The P-VAE's Normal latent block at one skip level as one forward and one backward launch (csrc/latent.hip states the function, the
layout of the random numbers, the order of the per-object sum and what the backward regenerates).

    normal_latents(skip, *, ns, seed, draw, level, first_object=0, sqrt_reg=EPS32)   (z [ns * B][C][H][W], KL [B]): the ns
                                                                        reparameterised samples of Normal(loc, pr(log_scale) + sqrt_reg),
                                                                        sample-major, and the per-object sum of KL(. || N(0, 1))
    latent_draws(n, length, *, ns, seed, draw, level, first_object=0)   the signed tail probabilities v the kernels draw, on the host
                                                                        (no GPU needed): eps = copysign(-ndtri(|v|), v)

There is no CPU path."""
import numpy as np

from . import _lib, _sampling_common as sc
from ._args import counter_args
from ._sampling_common import EPS32

__all__ = ["normal_latents", "latent_draws"]

MAX_NS = 65535
NS_MESSAGE = "ns shares a counter word with the level"


def latent_draws(n, length, *, ns, seed, draw, level, first_object=0):
    """float32 numpy array [ns][n][length]: v of element i of object b, sample s, is +-t with t = (((w >> 7) & 0xFFFFFF) + 0.5f) * 2^-25,
    negative when bit 31 of w is set; w is word e & 3 of Philox4x32-10((lo32(e >> 2), hi32(e >> 2), draw, 0x4C000000 | level << 16 | s),
    key = seed), e = (first_object + b) * length + i.  The kernels' eps is copysign(-ndtri(|v|), v)."""
    seed, draw, first_object = counter_args(seed, draw, first_object)
    ns, level = sc.key_args(ns, level, MAX_NS, NS_MESSAGE)
    n, length = int(n), int(length)
    if n < 1 or length < 1:
        raise ValueError(f"latent_draws: n and length must be positive (got {n}, {length})")
    out = np.empty((ns, n, length), np.float32)
    _lib.check(_lib.load().ctpvae_latent_draws_host_f32(n, length, ns, first_object, seed, draw, level, out.ctypes.data), "latent_draws_host")
    return out


class _NormalLatents(sc.LatentsFunction):
    @staticmethod
    def forward(ctx, skip, ns, sqrt_reg, seed, draw, level, first_object, eps):
        ctx.eps = eps                                                           # (stays alive for the backward)
        return sc.LatentsFunction.launch(ctx, "latent", skip, (ns, sqrt_reg, first_object, seed, draw, level, sc._ptr(eps)))


def normal_latents(skip, *, ns, seed, draw, level, first_object=0, sqrt_reg=EPS32, _eps=None):
    """skip [B][2C][H][W]: a contiguous float32 CUDA tensor, the encoder's output at one level (channels 0 .. C-1: loc, the rest:
    log_scale).  Returns (z [ns * B][C][H][W], KL [B]): z[s * B + b] = loc[b] + scale[b] * eps(s, b), scale = positive_range(log_scale) +
    sqrt_reg, sample-major as the decoder is fed; KL[b] the sum over object b of 0.5 (scale^2 + loc^2 - 1) - log scale, added in a fixed
    order (the same bits from run to run, whatever B and first_object).  eps depends on (seed, draw, level, s, (first_object + b), element)
    alone: pass the step index as `draw` and the GLOBAL batch offset as `first_object`, and a batch cut over calls or ranks draws what
    the whole batch draws, for any ns.  Differentiable once in skip, through both outputs.  _eps [ns * B][C][H][W] (tests) replaces the
    generator's draws."""
    ns, seed, draw, level, first_object = sc.check_skip("normal_latents", skip, ns, seed, draw, level, first_object, MAX_NS, NS_MESSAGE)
    if _eps is not None:
        sc.check_skip_input("normal_latents", "_eps", _eps)
        if tuple(_eps.shape) != (ns * skip.shape[0], skip.shape[1] // 2) + tuple(skip.shape[2:]) or _eps.device != skip.device:
            raise ValueError("normal_latents: _eps must be [ns * B][C][H][W] on skip's device")
        _eps = _eps.detach()
    sc.require_cuda("normal_latents", "skip must be a CUDA tensor", skip)
    return _NormalLatents.apply(skip, ns, float(sqrt_reg), seed, draw, level, first_object, _eps)
