"""The P-VAE's default Beta latent block at one skip level as one forward and one backward launch (csrc/beta_latent.hip states the
function, the layout of the random numbers, the work split, the order of the per-object sum and what the backward redraws).

    beta_latents(skip, *, ns, seed, draw, level, first_object=0, want_kl=True)   (z [ns * B][C][H][W], KL [B] or None): the ns
                                                                        reparameterised samples of Beta(pr(loc), pr(log_scale)),
                                                                        sample-major, and the per-object sum of KL(. || Beta(0.5, 0.5))
    beta_latent_words(n, length, *, seed, draw, level, s, gamma, attempt, first_object=0)
                                                                        the Philox words of one (level, s, gamma, attempt), on the host

There is no CPU path."""
import numpy as np

from . import _lib, _sampling_common as sc
from ._args import counter_args

__all__ = ["beta_latents", "beta_latent_words"]

MAX_NS = 2048
NS_MESSAGE = "the sample index shares a counter word with the level, the gamma and the attempt"


def beta_latent_words(n, length, *, seed, draw, level, s, gamma, attempt, first_object=0):
    """uint32 numpy array [n][length][4]: the block Philox4x32-10((lo32(e), hi32(e), draw, 0x51000000 | level << 16 | s << 5 | gamma << 4 |
    attempt), key = seed), e = (first_object + b) * length + i.  Attempt `attempt` of gamma `gamma` (0: pr(loc)'s, 1: pr(log_scale)'s) of
    sample s takes zn = ndtri(u24(word 0)), ua = u24(word 1), ub = u24(word 2)."""
    seed, draw, first_object = counter_args(seed, draw, first_object)
    _, level = sc.key_args(1, level, MAX_NS, NS_MESSAGE)
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


class _BetaLatents(sc.LatentsFunction):
    @staticmethod
    def forward(ctx, skip, ns, seed, draw, level, first_object, want_kl, extras):
        return sc.LatentsFunction.launch(ctx, "beta_latent", skip, (ns, first_object, seed, draw, level), want_kl, extras)


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
    ns, seed, draw, level, first_object = sc.check_skip("beta_latents", skip, ns, seed, draw, level, first_object, MAX_NS, NS_MESSAGE)
    if _extras is not None and not isinstance(_extras, dict):
        raise TypeError("beta_latents: _extras must be a dict")
    sc.require_cuda("beta_latents", "skip must be a CUDA tensor", skip)
    return _BetaLatents.apply(skip, ns, seed, draw, level, first_object, bool(want_kl), _extras)
