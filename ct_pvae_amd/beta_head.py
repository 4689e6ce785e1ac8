"""The P-VAE decoder's default Beta output head as one forward and one backward launch (csrc/beta_head.hip states the function, the
layout of the random numbers, the order of the per-object sum and what the backward re-evaluates).

    beta_head(alpha, beta, *, seed, draw, first_object=0, sqrt_reg=EPS32)   (x [n][X][Y][1], LP [n]): the reparameterised sample of
                                                                            Beta(pr(alpha), pr(beta)) and the per-object sum of its
                                                                            log-density at clamp(x, sqrt_reg, 1 - sqrt_reg)
    beta_head_words(n, pix, *, seed, draw, first_object=0, gamma, attempt)  the Philox words of one (gamma, attempt), on the host

There is no CPU path."""
import numpy as np

from . import _lib, _sampling_common as sc
from ._args import counter_args
from ._sampling_common import EPS32

__all__ = ["beta_head", "beta_head_words"]


def beta_head_words(n, pix, *, seed, draw, first_object=0, gamma, attempt):
    """uint32 numpy array [n][pix][4]: the block Philox4x32-10((lo32(e), hi32(e), draw, 0x42000000 | gamma << 8 | attempt), key = seed),
    e = (first_object + o) * pix + pixel.  Attempt `attempt` of gamma `gamma` (0: alpha's, 1: beta's) takes zn = ndtri(u24(word 0)),
    ua = u24(word 1), ub = u24(word 2)."""
    seed, draw, first_object = counter_args(seed, draw, first_object)
    n, pix, gamma, attempt = int(n), int(pix), int(gamma), int(attempt)
    if n < 1 or pix < 1:
        raise ValueError(f"beta_head_words: n and pix must be positive (got {n}, {pix})")
    if gamma not in (0, 1) or not 0 <= attempt < 16:
        raise ValueError(f"beta_head_words: gamma must be 0 or 1 and 0 <= attempt < 16 (got {gamma}, {attempt})")
    out = np.empty((n, pix, 4), np.uint32)
    _lib.check(_lib.load().ctpvae_beta_head_words_host_u32(n, pix, first_object, seed, draw, gamma, attempt, out.ctypes.data),
               "beta_head_words_host")
    return out


_BetaHead = sc.head_function("beta_head", test_outputs=2)                  # extra: sqrt_reg


def beta_head(alpha, beta, *, seed, draw, first_object=0, sqrt_reg=EPS32):
    """alpha, beta [n][1][X][Y]: contiguous float32 CUDA tensors, the decoder's raw outputs.  Returns (x [n][X][Y][1], LP [n]): x the
    reparameterised sample of Beta(positive_range(alpha), positive_range(beta)) in the projector's layout (not clamped), LP[o] the sum
    over object o of log_prob(clamp(x, sqrt_reg, 1 - sqrt_reg)), added in a fixed order (the same bits from run to run, whatever n and
    first_object).  The draws depend on (seed, draw, (first_object + o) * X * Y + pixel) alone: pass the step index as `draw` and the
    batch offset as `first_object`, and a batch cut over calls or ranks draws what the whole batch draws.  Differentiable once in alpha
    and beta, through both outputs: the implicit reparameterisation gradient of the two gammas (TensorFlow's, not torch's direct Beta
    derivative)."""
    sqrt_reg = float(sqrt_reg)
    seed, draw, first_object = sc.check_head_pair("beta_head", alpha, beta, seed, draw, first_object, sqrt_reg)
    return _BetaHead.apply(alpha, beta, seed, draw, first_object, sqrt_reg)
