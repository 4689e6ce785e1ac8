"""numpy restatement of recon(algorithm='mlem' | 'osem') (ct_pvae_amd/recon.py _mlem; libtomo mlem.c / osem.c [3P-recalled:
TomoPy 1.11.0]), composed from the oracle's projector pair: _project_grid is tomopy.project on the reconstruction grid (center =
dx / 2), siddon_backproject its ray-driven transpose in libtomo's order of terms.  Per iteration and block, in float32:

    sim    = A_b x
    ratio  = data_b / sim   where sim != 0, else 0            (rule="guarded": the build's)
             data_b / sim   where the ray has segments, else 0 (rule="libtomo": mlem.c's `if (sum_dist2 != 0.0)`, inf / NaN allowed)
    update = A_b^T ratio
    x      = x * (update / sum_dist)  where sum_dist != 0, else x unchanged        sum_dist = A_b^T 1

Block b of osem is ind_block[b * (dt // num_block) : ...], the last one to the end; mlem is the one block arange(dt)."""
import numpy as np

from oracle import radon_oracle as orc

F = np.float32


def blocks_of(dt, num_block=1, ind_block=None):
    ind = np.arange(dt) if ind_block is None else np.asarray(ind_block)
    step = dt // num_block
    return [ind[b * step:(b + 1) * step if b < num_block - 1 else dt] for b in range(num_block)]


def mlem(data, theta, num_iter=1, init=1e-6, ngridx=None, ngridy=None, num_block=1, ind_block=None, rule="guarded", each=None):
    """data [oy][dt][dx] -> [oy][gx][gy].  each(it, x): called with every finished iterate (it = 1 .. num_iter)."""
    data, theta = np.ascontiguousarray(data, F), np.ascontiguousarray(theta, F)
    oy, dt, dx = data.shape
    gx, gy = int(ngridx or dx), int(ngridy or dx)
    x = np.full((oy, gx, gy), init, F) if np.isscalar(init) else np.ascontiguousarray(init, F).copy()
    geo = []
    for blk in blocks_of(dt, num_block, ind_block):
        th = np.ascontiguousarray(theta[blk])
        sum_dist = orc.siddon_backproject(np.ones((1, blk.size, dx), F), th, gx, gy)[0]
        has_segments = orc._project_grid(np.ones((1, gx, gy), F), th, dx)[0] != 0          # sum of dist > 0 <=> sum of dist^2 != 0
        geo.append((th, np.ascontiguousarray(data[:, blk]), sum_dist, has_segments))
    for it in range(1, int(num_iter) + 1):
        for th, meas, sum_dist, has_segments in geo:
            sim = orc._project_grid(x, th, dx)
            with np.errstate(all="ignore"):
                q = meas / sim
                ratio = np.where(sim != 0 if rule == "guarded" else has_segments[None], q, F(0.0)).astype(F)
                update = orc.siddon_backproject(ratio, th, gx, gy)
                x = np.where(sum_dist != 0, x * (update / sum_dist), x).astype(F)
        if each is not None:
            each(it, x)
    return x


def poisson_loglik(data, sim):
    """sum of data log(sim) - sim over the rays with sim > 0, in float64 (the terms of the Poisson log-likelihood that depend on x)."""
    data, sim = np.asarray(data, np.float64), np.asarray(sim, np.float64)
    ok = sim > 0
    return float((np.where(data[ok] > 0, data[ok] * np.log(sim[ok]), 0.0) - sim[ok]).sum())
