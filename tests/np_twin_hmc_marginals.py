"""numpy restatement of what hmc_marginals (csrc/hmc_marginals.hip) accumulates, evaluated on stored samples: the histogram pooled over
an object's chains, the strictly sequential float64 sums of each half of the kept steps, the accepted steps -- and split R-hat straight
from the samples, without the sums."""
import numpy as np

from ct_pvae_amd import marginals


def seq_sum(x):
    """((x_0 + x_1) + x_2) + ... along axis 0 in float64 (np.sum adds pairwise); zeros for no rows."""
    x = np.asarray(x, np.float64)
    return np.cumsum(x, axis=0)[-1] if x.shape[0] else np.zeros(x.shape[1:])


def stats_from_samples(samples, accepted, lo, width, bins, chains_per_object):
    """samples [R][C][K] float32, accepted [R][C] (bool or 0 / 1) -> hist int64 [B][K][bins + 2], s1, s2 float64 [2][C][K],
    accepted int64 [C].  Half 0 is rows [0, R // 2), half 1 the rest."""
    samples = np.asarray(samples)
    assert samples.dtype == np.float32 and samples.ndim == 3
    R, C, K = samples.shape
    cpo, cols = int(chains_per_object), int(bins) + 2
    assert C % cpo == 0
    col = marginals.bin_columns(samples, lo, width, bins)                     # the library's host code of the rule
    obj = (np.arange(C) // cpo)[None, :, None]
    flat = ((obj * K + np.arange(K)[None, None, :]) * cols + col).ravel()
    hist = np.bincount(flat, minlength=(C // cpo) * K * cols).astype(np.int64).reshape(C // cpo, K, cols)
    x = samples.astype(np.float64)
    h = R // 2
    s1 = np.stack([seq_sum(x[:h]), seq_sum(x[h:])])
    s2 = np.stack([seq_sum(x[:h] * x[:h]), seq_sum(x[h:] * x[h:])])           # squares formed in float64: exact
    return hist, s1, s2, np.asarray(accepted).astype(bool).sum(0).astype(np.int64)


def rhat_from_samples(samples, chains_per_object):
    """Split R-hat [B][K] by numpy on the samples [R][C][K] themselves (R even): the sequences of an object are its chains' halves."""
    x = np.asarray(samples, np.float64)
    R, C, K = x.shape
    n, cpo = R // 2, int(chains_per_object)
    seqs = x.reshape(2, n, C // cpo, cpo, K).transpose(2, 0, 3, 1, 4).reshape(C // cpo, 2 * cpo, n, K)     # [B][m][n][K]
    W = seqs.var(axis=2, ddof=1).mean(axis=1)
    Bn = seqs.mean(axis=2).var(axis=1, ddof=1)
    return np.sqrt(((n - 1) / n * W + Bn) / W)
