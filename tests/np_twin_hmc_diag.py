"""numpy restatement of what hmc_marginals(max_lag=, cov=) adds to the launch (csrc/hmc_diagnostics.hip), evaluated on stored samples
[n][C][K]: the lagged products r, the first and the last values (head, ring) and the cross products xx by the kernel's strictly
sequential float64 rule -- and the same statistics directly, from centred differences, without any raw sum."""
import numpy as np

from tests.np_twin_hmc_marginals import seq_sum


def raw_sums(samples, max_lag, cov=True):
    """samples [n][C][K] float32 -> lag float64 [C][Lm + 1][K], ring float32 [C][Lm + 1][K], head float32 [C][Lm][K], xx float64
    [C][K][K] (None without cov).  r_l = ((0 + x_l x_0) + x_(l+1) x_1) + ... in float64 (every product is exact); lags >= n stay 0.
    ring: step j in slot j mod (Lm + 1), unwritten slots 0; head: rows j < min(n, Lm), the rest 0."""
    samples = np.asarray(samples)
    assert samples.dtype == np.float32 and samples.ndim == 3 and max_lag >= 1
    n, C, K = samples.shape
    x = samples.astype(np.float64)
    slots = max_lag + 1
    lag = np.zeros((C, slots, K))
    for l in range(min(slots, n)):
        lag[:, l] = seq_sum(x[l:] * x[:n - l])
    ring = np.zeros((C, slots, K), np.float32)
    for j in range(max(0, n - slots), n):
        ring[:, j % slots] = samples[j]
    head = np.zeros((C, max_lag, K), np.float32)
    head[:, :min(n, max_lag)] = samples[:max_lag].transpose(1, 0, 2)
    xx = None
    if cov:
        xx = np.zeros((C, K, K))
        for c in range(C):
            for k in range(K):
                xx[c, k] = seq_sum(x[:, c, k, None] * x[:, c, :])
    return lag, ring, head, xx


def autocov_direct(samples, max_lag):
    """float64 [C][Lm + 1][K]: sum_j (x_j - m)(x_(j-l) - m) / n with m the chain's mean, by numpy's pairwise sums; 0 for l >= n."""
    x = np.asarray(samples, np.float64)
    n = x.shape[0]
    d = x - x.mean(axis=0)
    out = np.zeros((x.shape[1], max_lag + 1, x.shape[2]))
    for l in range(min(max_lag + 1, n)):
        out[:, l] = (d[l:] * d[:n - l]).sum(axis=0) / n
    return out


def cov_direct(samples, chains_per_object):
    """float64 [B][K][K]: np.cov (count - 1) of an object's pooled samples."""
    x = np.asarray(samples, np.float64)
    n, C, K = x.shape
    pooled = x.reshape(n, C // chains_per_object, chains_per_object, K).transpose(1, 0, 2, 3).reshape(-1, n * chains_per_object, K)
    return np.stack([np.cov(p, rowvar=False, ddof=1) for p in pooled])


def ar1(phi, n, C, K, seed, mean=0.0, std=1.0):
    """float32 [n][C][K]: stationary AR(1) series x_j = mean + phi (x_(j-1) - mean) + e_j of marginal standard deviation std."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, C, K))
    y = e
    if phi != 0.0:
        s = np.sqrt(1.0 - phi * phi)
        for j in range(1, n):                            # y_0 = e_0 has the stationary variance 1
            y[j] = phi * y[j - 1] + s * e[j]
    return (mean + std * y).astype(np.float32)
