"""hmc_marginals (ct_pvae_amd.mcmc, csrc/hmc_marginals.hip) on the GPU: its chains are hmc_sample's bit for bit, and its statistics are
those of the samples -- integers, and float64 by bits -- against the numpy twin (tests/np_twin_hmc_marginals.py) on the stored samples."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import np_twin_hmc as tw
from tests import np_twin_hmc_marginals as twm
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# the kept window (steps 6 .. 29) opens inside the first launch of 7 steps; the half boundary (step 18) falls inside the third
RUN = dict(num_results=24, num_burnin_steps=6, num_adaptation_steps=10, steps_per_launch=7, chains_per_object=8)
GRIDS = {"toy": dict(lo=0.005, width=0.01, bins=50), "n3": dict(lo=0.2, width=0.01, bins=5), "n8": dict(lo=0.005, width=0.01, bins=50),
         "max": dict(lo=0.0, width=2e-4, bins=254)}
NAMES = ("toy", "n3", "n8")


@functools.lru_cache(maxsize=None)
def _problem(name):
    from oracle import radon_oracle
    radon_oracle.build()
    return tw.problem(radon_oracle, name)


def _args(name, C=8, **kw):
    import torch
    pb = _problem(name)
    dev = torch.device("cuda", 0)
    a = dict(RUN, prior=pb["prior"], initial_state=tw.random_starts(name, C), step_size=tw.STEP[name], seed=tw.SEEDS[name])
    a.update(kw)
    return (torch.from_numpy(pb["meas"]).to(dev), torch.from_numpy(pb["mask"]).to(dev), pb["theta"], pb["pnm"]), a


@functools.lru_cache(maxsize=None)
def _kept(name):
    """The run of test 1 on problem `name`: (hmc_sample's result, hmc_marginals' with keep_samples=True); never modified."""
    import torch

    import ct_pvae_amd as cp
    pos, kw = _args(name)
    ref = cp.hmc_sample(*pos, **kw)
    m = cp.hmc_marginals(*pos, keep_samples=True, **GRIDS[name], **kw)
    torch.cuda.synchronize()
    return ref, m


def _same_as_sampler(ref, m):
    import torch
    assert torch.equal(m.samples, ref[0]) and not torch.isnan(m.samples).any()
    assert set(m.trace) == set(ref[1])
    for k, v in ref[1].items():
        assert torch.equal(m.trace[k], v) and m.trace[k].dtype == v.dtype, k
    assert torch.equal(m.step_size, ref[1]["step_size"])


def _same_as_twin(m, grid, cpo):
    hist, s1, s2, acc = twm.stats_from_samples(m.samples.cpu().numpy(), m.trace["is_accepted"].cpu().numpy(), chains_per_object=cpo, **grid)
    got = [v.cpu().numpy() for v in (m.hist, m.s1, m.s2, m.accepted)]
    assert got[0].dtype == np.int64 and got[1].dtype == got[2].dtype == np.float64 and got[3].dtype == np.int64
    assert np.array_equal(got[0], hist)
    assert np.array_equal(got[1].view(np.int64), s1.view(np.int64)) and np.array_equal(got[2].view(np.int64), s2.view(np.int64))
    assert np.array_equal(got[3], acc)
    return hist


def _equal_stats(a, b):
    import torch
    for k in ("hist", "s1", "s2", "accepted", "step_size"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("name", NAMES)
def test_the_statistics_are_those_of_the_samples(name):
    ref, m = _kept(name)
    _same_as_sampler(ref, m)
    K = _problem(name)["N"] ** 2
    assert m.shape == (_problem(name)["N"],) * 2 and m.count == 24 * 8 and tuple(m.hist.shape) == (1, K, GRIDS[name]["bins"] + 2)
    hist = _same_as_twin(m, GRIDS[name], 8)
    assert np.all(hist.sum(-1) == 24 * 8)
    if name == "n3":
        assert hist[..., 0].sum() + hist[..., -1].sum() > 0.5 * hist.sum()       # the grid puts most samples in the outer columns
    else:
        assert hist[..., 1:-1].sum() > 0
    acc = m.accepted.cpu().numpy()
    assert 0 < acc.sum() < 24 * 8                                               # both decisions occur
    np.testing.assert_allclose(m.mean().sum((1, 2)), 1.0, rtol=0, atol=1e-5)    # points of the simplex


def test_the_extremes_at_once():
    """8 x 8, 256 angles, 4 components, 32 leapfrog steps and 254 bins: the largest LDS request the entry point admits."""
    import torch

    import ct_pvae_amd as cp
    pos, kw = _args("max", num_results=4, num_burnin_steps=0, num_adaptation_steps=2, steps_per_launch=3, num_leapfrog_steps=tw.EXTREME_L)
    ref = cp.hmc_sample(*pos, **kw)
    m = cp.hmc_marginals(*pos, keep_samples=True, **GRIDS["max"], **kw)
    torch.cuda.synchronize()
    _same_as_sampler(ref, m)
    hist = _same_as_twin(m, GRIDS["max"], 8)
    assert np.all(hist.sum(-1) == 32) and (hist[0].sum(0) > 0).sum() > 50          # the samples spread over the columns
    assert cp._lib.load().ctpvae_hmc_marginals_lds_bytes(8, 256, 254) > 64 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_cutting_into_launches(name):
    import torch

    import ct_pvae_amd as cp
    _, kept = _kept(name)
    for spl in (1, 5, 512):
        pos, kw = _args(name, steps_per_launch=spl)
        m = cp.hmc_marginals(*pos, **GRIDS[name], **kw)
        torch.cuda.synchronize()
        assert m.samples is None and m.trace is None
        _equal_stats(m, kept)


def test_placement():
    """8 chains in one call against chains 0 .. 3 and 4 .. 7 in two: per-chain arrays concatenate, the histograms add up."""
    import torch

    import ct_pvae_amd as cp
    _, one = _kept("n3")
    starts = tw.random_starts("n3", 8)
    parts = []
    for first in (0, 4):
        pos, kw = _args("n3", chains_per_object=4, first_chain=first, initial_state=starts[first:first + 4])
        parts.append(cp.hmc_marginals(*pos, **GRIDS["n3"], **kw))
    torch.cuda.synchronize()
    a, b = parts
    assert torch.equal(one.s1, torch.cat([a.s1, b.s1], 1)) and torch.equal(one.s2, torch.cat([a.s2, b.s2], 1))
    assert torch.equal(one.accepted, torch.cat([a.accepted, b.accepted])) and torch.equal(one.step_size, torch.cat([a.step_size, b.step_size]))
    assert torch.equal(one.hist, a.hist + b.hist) and not torch.equal(a.hist, b.hist)


def test_nothing_grows_with_the_run():
    """Peak device memory of a call above what was allocated before it, at 20 and at 20000 kept steps of 64 chains: within 1 MiB of
    each other (stored outputs would add 20000 * 64 * (4 + 3) * 4 B = 35.8 MB)."""
    import torch

    import ct_pvae_amd as cp
    pos, kw = _args("toy", C=64, chains_per_object=64, num_burnin_steps=0, steps_per_launch=None)
    peaks = []
    for n in (20, 20000):
        kw["num_results"] = n
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        m = cp.hmc_marginals(*pos, **GRIDS["toy"], **kw)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - before)
        assert m.samples is None and m.trace is None and int(m.hist.sum()) == 4 * 64 * n and m.count == 64 * n
        del m
    print("peak bytes above the baseline at 20 and 20000 results:", peaks)
    assert abs(peaks[1] - peaks[0]) <= 2 ** 20


@pytest.mark.parametrize("name", NAMES)
def test_rhat_is_that_of_the_stored_samples(name):
    _, m = _kept(name)
    want = twm.rhat_from_samples(m.samples.cpu().numpy(), 8)
    got = m.rhat()
    print(name, "split R-hat", got.min(), "..", got.max())
    assert got.shape == (1, _problem(name)["N"] ** 2) and np.all(np.isfinite(want))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


def test_cli(tmp_path):
    """python -m ct_pvae_amd.mcmc --marginals --no_trace on a toy folder: hmc_marginals.npz appears and loads, no
    posterior_prob_trace.npy; --compare runs against a PixelMarginals.save file of the same grid and refuses one with other bins."""
    import torch

    import ct_pvae_amd as cp
    from ct_pvae_amd import phantoms
    dev = torch.device("cuda", 0)
    imgs = np.tile(phantoms.toy_images(), (2, 1, 1))
    theta = np.array([0, np.pi / 2], np.float32)
    sino = torch.stack([cp.project_tf_fast(torch.from_numpy(im).to(dev), theta, pad=False, dim=2)[..., 0] for im in imgs])
    masks, samples = cp.create_all_masks(sino, 2, str(tmp_path), 1e3, train=True, toy_masks=True, device=dev)
    g = torch.Generator().manual_seed(0)
    alpha, beta = (torch.rand((3, 1, 2, 2), generator=g).to(dev) for _ in range(2))
    cp.PixelMarginals((2, 2), device=dev).add(alpha, beta, draws=50, seed=1).save(tmp_path / "pixel_dist_0.npz")
    cp.PixelMarginals((2, 2), bins=20, device=dev).add(alpha, beta, draws=50, seed=1).save(tmp_path / "other_bins.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "ct_pvae_amd.mcmc", "--save_path", str(tmp_path), "-s", "300", "-b", "100", "--chains", "4", "--marginals",
           "--no_trace", "--compare"]
    subprocess.run(cmd + [str(tmp_path / "pixel_dist_0.npz")], check=True, env=env, cwd=ROOT, timeout=300)
    assert not (tmp_path / "posterior_prob_trace.npy").exists()
    m = cp.HmcMarginals.load(tmp_path / "hmc_marginals.npz", device=dev)
    assert m.shape == (2, 2) and m.count == 1200 and m.samples is None and int(m.hist.sum()) == 4 * 1200
    used = masks[0] > 0
    want = cp.hmc_marginals(samples[0][used], masks[0][used], theta[used.cpu().numpy()], 1e3, num_results=300, num_burnin_steps=100,
                            chains_per_object=4)
    _equal_stats(m, want)
    d = np.load(tmp_path / "hmc_vs_pvae.npy")
    assert d.shape == (4,) and d.dtype == np.float64 and np.all((d >= 0) & (d <= 1))
    assert np.array_equal(d, cp.hist_distance(cp.PixelMarginals.load(tmp_path / "pixel_dist_0.npz", device=dev).hist, m.hist[0]))
    os.remove(tmp_path / "hmc_marginals.npz")
    out = subprocess.run(cmd + [str(tmp_path / "other_bins.npz")], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert out.returncode != 0 and "another grid" in out.stderr and not (tmp_path / "hmc_marginals.npz").exists()
