"""The P-VAE's default Beta latent block at one skip level as one forward and one backward launch (csrc/beta_latent.hip states the
function, the layout of the random numbers, the work split, the order of the per-object sum and what the backward redraws).

    beta_latents(skip, *, ns, seed, draw, level, first_object=0, want_kl=True)   (z [ns * B][C][H][W], KL [B] or None): the ns
                                                                        reparameterised samples of Beta(pr(loc), pr(log_scale)),
                                                                        sample-major, and the per-object sum of KL(. || Beta(0.5, 0.5))
    beta_latent_words(n, length, *, seed, draw, level, s, gamma, attempt, first_object=0)
                                                                        the Philox words of one (level, s, gamma, attempt), on the host

There is no CPU path."""
import numpy as np
import torch

from . import _lib, forward_functions
from ._args import check_float32
from .forward_functions import _stream_ptr
from .output_head import _counter_args

__all__ = ["beta_latents", "beta_latent_words"]

MAX_NS = 2048


def _key_args(ns, level):
    ns, level = int(ns), int(level)
    if not 1 <= ns <= MAX_NS:
        raise ValueError(f"the sample index shares a counter word with the level, the gamma and the attempt: 1 <= ns <= {MAX_NS} (got {ns})")
    if not 0 <= level <= 255:
        raise ValueError(f"level is one byte of a counter word: 0 <= level <= 255 (got {level})")
    return ns, level


def beta_latent_words(n, length, *, seed, draw, level, s, gamma, attempt, first_object=0):
    """uint32 numpy array [n][length][4]: the block Philox4x32-10((lo32(e), hi32(e), draw, 0x51000000 | level << 16 | s << 5 | gamma << 4 |
    attempt), key = seed), e = (first_object + b) * length + i.  Attempt `attempt` of gamma `gamma` (0: pr(loc)'s, 1: pr(log_scale)'s) of
    sample s takes zn = ndtri(u24(word 0)), ua = u24(word 1), ub = u24(word 2)."""
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    _, level = _key_args(1, level)
    n, length, s, gamma, attempt = int(n), int(length), int(s), int(gamma), int(attempt)
    if n < 1 or length < 1:
        raise ValueError(f"beta_latent_words: n and length must be positive (got {n}, {length})")
    if not 0 <= s < MAX_NS:
        raise ValueError(f"beta_latent_words: 0 <= s < {MAX_NS} (got {s})")
    if gamma not in (0, 1) or not 0 <= attempt < 16:
        raise ValueError(f"beta_latent_words: gamma must be 0 or 1 and 0 <= attempt < 16 (got {gamma}, {attempt})")
    out = np.empty((n, length, 4), np.uint32)
    _lib.check(_lib.load().ctpvae_beta_latent_words_host_u32(n, length, first_object, seed, draw, level, s, gamma, attempt, out.ctypes.data),
               "beta_latent_words_host")
    return out


def _check_input(name, t):
    check_float32("beta_latents", name, t, 4, "[B][channels][H][W], the encoder's layout")


class _BetaLatents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, skip, ns, seed, draw, level, first_object, want_kl, extras):
        B, C2, H, W = skip.shape
        length = (C2 // 2) * H * W
        sk = skip.detach()
        z = forward_functions._new_output((ns * B, C2 // 2, H, W), torch.float32, skip.device)
        kl = forward_functions._new_output((B,), torch.float32, skip.device) if want_kl else None
        kl_elem = aux = None
        if extras is not None:                                       # tests: the per-element terms and the accepted draws
            kl_elem = forward_functions._new_output((B, length), torch.float32, skip.device) if want_kl else None
            aux = forward_functions._new_output((ns * B, length, 2, 4), torch.float32, skip.device)
            extras["kl_elem"], extras["aux"] = kl_elem, aux
        with torch.cuda.device(skip.device):
            _lib.check(_lib.load().ctpvae_beta_latent_fwd_f32(sk.data_ptr(), B, length, ns, first_object, seed, draw, level, z.data_ptr(),
                                                              kl.data_ptr() if kl is not None else None,
                                                              kl_elem.data_ptr() if kl_elem is not None else None,
                                                              aux.data_ptr() if aux is not None else None, _stream_ptr()), "beta_latent_fwd")
        ctx.save_for_backward(sk)
        ctx.key = (ns, first_object, seed, draw, level)
        ctx.set_materialize_grads(False)
        if kl is None:
            return z, None
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
            _lib.check(_lib.load().ctpvae_beta_latent_bwd_f32(sk.data_ptr(), B, (C2 // 2) * H * W, *ctx.key,
                                                              g_z.data_ptr() if g_z is not None else None,
                                                              g_kl.data_ptr() if g_kl is not None else None,
                                                              g_skip.data_ptr(), _stream_ptr()), "beta_latent_bwd")
        return (g_skip,) + (None,) * 7


def beta_latents(skip, *, ns, seed, draw, level, first_object=0, want_kl=True, _extras=None):
    """skip [B][2C][H][W]: a contiguous float32 CUDA tensor, the encoder's output at one level (channels 0 .. C-1: loc, the rest:
    log_scale).  Returns (z [ns * B][C][H][W], KL [B]): z[s * B + b] the reparameterised sample s of Beta(positive_range(loc[b]),
    positive_range(log_scale[b])), sample-major as the decoder is fed, not clamped; KL[b] the sum over object b of the KL term against
    the Beta(0.5, 0.5) prior, added in a fixed order (the same bits from run to run, whatever B and first_object).  want_kl=False: no KL
    is computed and None is returned in its place (the trainer's input level).  The draws depend on (seed, draw, level, s,
    (first_object + b), element) alone: pass the step index as `draw` and the GLOBAL batch offset as `first_object`, and a batch cut
    over calls or ranks draws what the whole batch draws, for any ns.  Differentiable once in skip, through both outputs: the implicit
    reparameterisation gradient of the two gammas (TensorFlow's, not torch's direct Beta derivative) and the closed-form gradient of the
    KL term.  _extras (tests): a dict that receives kl_elem [B][len] and aux [ns * B][len][2][4], the (zn, ub, attempt, lg) of each
    gamma's accepted attempt."""
    _check_input("skip", skip)
    if skip.shape[1] % 2 != 0:
        raise ValueError(f"beta_latents: skip needs an even channel count, loc then log_scale (got {tuple(skip.shape)})")
    seed, draw, first_object = _counter_args(seed, draw, first_object)
    ns, level = _key_args(ns, level)
    if ns * (skip.numel() // 2) >= 2 ** 31:
        raise ValueError(f"beta_latents: at most 2^31 - 1 samples per call (got {ns} x {skip.numel() // 2})")
    if _extras is not None and not isinstance(_extras, dict):
        raise TypeError("beta_latents: _extras must be a dict")
    if skip.device.type != "cuda":
        raise _lib.RadonLibraryError("beta_latents: skip must be a CUDA tensor; there is no CPU path")
    return _BetaLatents.apply(skip, ns, seed, draw, level, first_object, bool(want_kl), _extras)
