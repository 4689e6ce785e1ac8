"""The P-VAE decoder's TruncatedNormal output head as one forward and one backward launch (csrc/head.hip states the function, the
layout of the random numbers, the order of the per-object sum and what the backward re-evaluates).

    truncated_normal_head(alpha, beta, *, seed, draw, first_object=0)   (x [n][X][Y][1], LP [n]): the reparameterised sample of
                                                                        TruncatedNormal(pr(alpha), pr(beta), 0, 1e10) and the
                                                                        per-object sum of its log-density at that sample
    head_uniforms(n, pix, *, seed, draw, first_object=0)                the uniforms the kernels draw, on the host (no GPU needed)

There is no CPU path."""
import numpy as np

from . import _lib, _sampling_common as sc
from ._args import counter_args

__all__ = ["truncated_normal_head", "head_uniforms"]


def head_uniforms(n, pix, *, seed, draw, first_object=0):
    """float32 numpy array [n][pix]: u of pixel `pixel` of object o is word e & 3 of Philox4x32-10((lo32(e >> 2), hi32(e >> 2), draw,
    0x544E48), key = seed), e = (first_object + o) * pix + pixel, as ((w >> 8) + 0.5f) * 2^-24."""
    seed, draw, first_object = counter_args(seed, draw, first_object)
    n, pix = int(n), int(pix)
    if n < 1 or pix < 1:
        raise ValueError(f"head_uniforms: n and pix must be positive (got {n}, {pix})")
    out = np.empty((n, pix), np.float32)
    _lib.check(_lib.load().ctpvae_tn_head_uniforms_host_f32(n, pix, first_object, seed, draw, out.ctypes.data), "tn_head_uniforms_host")
    return out


_TruncatedNormalHead = sc.head_function("tn_head", test_outputs=1)         # extra: u [n][1][X][Y] or None


def truncated_normal_head(alpha, beta, *, seed, draw, first_object=0, _u=None):
    """alpha, beta [n][1][X][Y]: contiguous float32 CUDA tensors, the decoder's raw outputs.  Returns (x [n][X][Y][1], LP [n]): x the
    reparameterised sample of TruncatedNormal(positive_range(alpha), positive_range(beta), low=0, high=1e10) in the projector's layout,
    LP[o] the sum over object o of log_prob(x), added in a fixed order (the same bits from run to run, whatever n and first_object).
    The uniforms depend on (seed, draw, (first_object + o) * X * Y + pixel) alone: pass the step index as `draw` and the batch
    offset as `first_object`, and a batch cut over calls or ranks draws what the whole batch draws.  Differentiable once in alpha and
    beta, through both outputs.  _u [n][1][X][Y] (tests) replaces the generator's uniforms."""
    seed, draw, first_object = sc.check_head_pair("truncated_normal_head", alpha, beta, seed, draw, first_object)
    if _u is not None:
        sc.check_head_input("truncated_normal_head", "_u", _u)
        if _u.shape != alpha.shape or _u.device != alpha.device:
            raise ValueError("truncated_normal_head: _u must have alpha's shape and device")
        _u = _u.detach()
    return _TruncatedNormalHead.apply(alpha, beta, seed, draw, first_object, _u)
