"""hmc_marginals(max_lag=, cov=) (ct_pvae_amd.mcmc, csrc/hmc_diagnostics.hip) on the GPU, on the problems, seeds and run shape of
tests/test_gpu_hmc_marginals.py: everything the call returned before keeps its bits, and the new raw sums are those of the stored samples
-- float64 and float32 by bits -- against the numpy twin (tests/np_twin_hmc_diag.py), however the run is cut into launches and calls."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import np_twin_hmc as tw
from tests import np_twin_hmc_diag as twd
from tests import test_gpu_hmc_marginals as base
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

NAMES = base.NAMES
NEW = ("lag", "ring", "head", "xx")
# 24 kept steps after 6 of burn-in in launches of 7 (base.RUN): 6 ring slots wrap four times, and lags of up to 5 reach across launches
DIAG = dict(max_lag=5, cov=True)
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def _diag(name):
    """The run of test 1 on problem `name` with keep_samples=True, max_lag=5, cov=True; never modified."""
    import torch

    import ct_pvae_amd as cp
    pos, kw = base._args(name)
    m = cp.hmc_marginals(*pos, keep_samples=True, **DIAG, **base.GRIDS[name], **kw)
    torch.cuda.synchronize()
    return m


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same_as_twin(m, max_lag, cov=True):
    lag, ring, head, xx = twd.raw_sums(m.samples.cpu().numpy(), max_lag, cov)
    assert _bits(m.lag).dtype == np.int64 and _bits(m.ring).dtype == _bits(m.head).dtype == np.int32
    assert np.array_equal(_bits(m.lag), _bits(lag)), "lag"
    assert np.array_equal(_bits(m.ring), _bits(ring)), "ring"
    assert np.array_equal(_bits(m.head), _bits(head)), "head"
    if cov:
        assert _bits(m.xx).dtype == np.int64 and np.array_equal(_bits(m.xx), _bits(xx)), "xx"
    else:
        assert m.xx is None


def _equal_new(a, b):
    import torch
    for k in NEW:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("name", NAMES)
def test_bits_against_the_marginals_and_the_twin(name):
    import torch
    _, plain = base._kept(name)                      # hmc_marginals without the new keywords
    m = _diag(name)
    K = base._problem(name)["N"] ** 2
    assert torch.equal(m.samples, plain.samples) and not torch.isnan(m.samples).any()
    for k, v in plain.trace.items():
        assert torch.equal(m.trace[k], v) and m.trace[k].dtype == v.dtype, k
    base._equal_stats(m, plain)
    assert m.max_lag == 5 and tuple(m.lag.shape) == (8, 6, K) and tuple(m.ring.shape) == (8, 6, K) and tuple(m.head.shape) == (8, 5, K)
    assert tuple(m.xx.shape) == (8, K, K) and plain.lag is None and plain.xx is None and plain.max_lag == 0
    _same_as_twin(m, 5)
    assert (m.lag >= 0).all() and (m.lag[:, 0] > 0).all() and (m.xx >= 0).all()
    # the finish, on the device's sums, against numpy on the stored samples
    x = m.samples.cpu().numpy()
    c, want = m.autocov(), twd.autocov_direct(x, 5)
    np.testing.assert_allclose(c, want, rtol=0, atol=2.5 * 24 * EPS)            # the CPU file's bar; the values lie in [0, 1]
    np.testing.assert_allclose(m.cov(), twd.cov_direct(x, 8), rtol=0, atol=2.5 * 192 * EPS)
    assert m.ess().shape == (1, K) and m.ess(cross_chain=False).shape == (8, K) and m.ess_truncated().dtype == bool


def test_both_features_off_is_the_marginals_launch():
    """ctpvae_hmc_run_diagnostics_f32 with max_lag = 0 and no xx, called the way hmc_marginals calls the marginals' entry point."""
    import torch

    from ct_pvae_amd import _lib, mcmc
    from ct_pvae_amd.forward_functions import _stream_ptr
    _, plain = base._kept("n3")
    pos, kw = base._args("n3")
    kw = dict(kw, num_leapfrog_steps=5, first_chain=0)
    r = mcmc._start_run("hmc_marginals", *pos, **kw, grid=tuple(base.GRIDS["n3"][k] for k in ("bins", "lo", "width")), diag=(0, False))
    bins, lo, width = r.grid
    hist = torch.zeros((r.B, r.K, bins + 2), dtype=torch.int64, device=r.dev)
    mom = torch.zeros((2, 2, r.C, r.K), dtype=torch.float64, device=r.dev)
    accepted = torch.zeros(r.C, dtype=torch.int64, device=r.dev)
    L, keep_from, n_adapt, seed64 = r.run_args
    with torch.cuda.device(r.dev):
        for n, _ in mcmc._launches(r):
            _lib.check(r.lib.ctpvae_hmc_run_diagnostics_f32(r.state.data_ptr(), r.C, r.first_chain, r.cpo, *r.model, L, n, keep_from, n_adapt,
                                                            seed64, None, None, None, None, keep_from + r.num_results // 2, lo, width, bins,
                                                            hist.data_ptr(), mom.data_ptr(), accepted.data_ptr(), 0, None, None, None, None,
                                                            _stream_ptr()), "hmc_run_diagnostics")
    torch.cuda.synchronize()
    assert torch.equal(hist, plain.hist) and torch.equal(mom[:, 0], plain.s1) and torch.equal(mom[:, 1], plain.s2)
    assert torch.equal(accepted, plain.accepted) and torch.equal(r.state[:, 2 * r.K - 1], plain.step_size)


def test_lag_window_longer_than_the_run():
    """max_lag = 64 with 24 kept steps: lags >= 24 and head rows >= 24 stay exact zeros, the ring never wraps, autocov is 0 there."""
    import torch

    import ct_pvae_amd as cp
    pos, kw = base._args("toy")
    m = cp.hmc_marginals(*pos, keep_samples=True, max_lag=64, **base.GRIDS["toy"], **kw)
    torch.cuda.synchronize()
    base._equal_stats(m, base._kept("toy")[1])
    _same_as_twin(m, 64, cov=False)
    assert (m.lag[:, 24:] == 0).all() and (m.lag[:, :24] != 0).all() and (m.head[:, 24:] == 0).all() and (m.head[:, :24] > 0).all()
    assert (m.ring[:, 24:] == 0).all() and torch.equal(m.ring[:, :24], m.head[:, :24])
    c = m.autocov()
    assert np.all(c[:, 24:] == 0.0) and np.all(c[:, 0] > 0)
    np.testing.assert_allclose(c, twd.autocov_direct(m.samples.cpu().numpy(), 64), rtol=0, atol=2.5 * 24 * EPS)
    assert torch.equal(m.lag[:, :6], _diag("toy").lag)          # a lag's sum does not depend on the window


@pytest.mark.parametrize("name", NAMES)
def test_cutting_into_launches(name):
    import torch

    import ct_pvae_amd as cp
    kept = _diag(name)
    for spl in (1, 7, 30):
        pos, kw = base._args(name, steps_per_launch=spl)
        m = cp.hmc_marginals(*pos, **DIAG, **base.GRIDS[name], **kw)
        torch.cuda.synchronize()
        assert m.samples is None and m.trace is None
        base._equal_stats(m, kept)
        _equal_new(m, kept)


def test_placement():
    """8 chains in one call against chains 0 .. 3 and 4 .. 7 in two: every new array is per chain and concatenates."""
    import torch

    import ct_pvae_amd as cp
    one = _diag("n3")
    starts = tw.random_starts("n3", 8)
    parts = []
    for first in (0, 4):
        pos, kw = base._args("n3", chains_per_object=4, first_chain=first, initial_state=starts[first:first + 4])
        parts.append(cp.hmc_marginals(*pos, **DIAG, **base.GRIDS["n3"], **kw))
    torch.cuda.synchronize()
    a, b = parts
    for k in NEW:
        assert torch.equal(getattr(one, k), torch.cat([getattr(a, k), getattr(b, k)], 0)), k
    assert torch.equal(one.s1, torch.cat([a.s1, b.s1], 1)) and torch.equal(one.hist, a.hist + b.hist)


@pytest.mark.parametrize("name", NAMES)
def test_symmetry(name):
    m = _diag(name)
    xx = _bits(m.xx)
    assert np.array_equal(xx, xx.transpose(0, 2, 1))
    v = m.cov()
    assert np.array_equal(v, v.transpose(0, 2, 1))
    print(name, "largest |row sum| of cov / largest entry", np.abs(v.sum(-1)).max() / np.abs(v).max())
    assert np.all(np.abs(v.sum(-1)) <= 1e-6 * np.abs(v).max())          # the pixels sum to 1 on the simplex
    r = m.corr()
    assert np.all(np.abs(r[np.isfinite(r)]) <= 1 + 1e-12)


def test_the_largest_lds_request():
    """8 x 8, 256 angles, 4 components, 32 leapfrog steps, 254 bins, cov and the longest lag window the entry point admits beside them
    (9 lags: 163,616 of 163,840 bytes), once, with 4 kept steps; one lag more is refused before any launch."""
    import torch

    import ct_pvae_amd as cp
    kw_run = dict(num_results=4, num_burnin_steps=0, num_adaptation_steps=2, steps_per_launch=3, num_leapfrog_steps=tw.EXTREME_L)
    pos, kw = base._args("max", **kw_run)
    assert cp._lib.load().ctpvae_hmc_diagnostics_lds_bytes(8, 256, 254, 9, 1) == 163616
    with pytest.raises(ValueError, match="bytes of LDS"):
        cp.hmc_marginals(*pos, max_lag=10, cov=True, **base.GRIDS["max"], **kw)
    plain = cp.hmc_marginals(*pos, keep_samples=True, **base.GRIDS["max"], **kw)
    m = cp.hmc_marginals(*pos, keep_samples=True, max_lag=9, cov=True, **base.GRIDS["max"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(m.samples, plain.samples) and not torch.isnan(m.samples).any()
    base._equal_stats(m, plain)
    _same_as_twin(m, 9)
    assert (m.lag[:, 4:] == 0).all() and (m.lag[:, :4] >= 0).all() and (m.lag[:, :4].sum(-1) > 0).all()


def test_nothing_grows_with_the_run():
    """Peak device memory of a call above what was allocated before it, at 24 and at 240 kept steps of 256 chains with 64 lags and
    cov: equal within 64 KiB (one stored float per chain and step would add 216 * 256 * 4 B = 221 KB)."""
    import torch

    import ct_pvae_amd as cp
    pos, kw = base._args("toy", C=256, chains_per_object=256, num_burnin_steps=0)
    peaks = []
    for n in (24, 240):
        kw["num_results"] = n
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        m = cp.hmc_marginals(*pos, max_lag=64, cov=True, **base.GRIDS["toy"], **kw)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - before)
        assert m.samples is None and m.trace is None and int(m.hist.sum()) == 4 * 256 * n and (m.lag[:, min(n, 65) - 1] != 0).all()
        del m
    print("peak bytes above the baseline at 24 and 240 results:", peaks)
    assert abs(peaks[1] - peaks[0]) <= 2 ** 16


def test_cli(tmp_path):
    """python -m ct_pvae_amd.mcmc --marginals --no_trace --ess_lags 5 --cov in a fresh process: prints the ESS, and hmc_marginals.npz
    round-trips through HmcMarginals.load with the arrays of the same call made here."""
    import torch

    import ct_pvae_amd as cp
    from ct_pvae_amd import phantoms
    dev = torch.device("cuda", 0)
    imgs = np.tile(phantoms.toy_images(), (2, 1, 1))
    theta = np.array([0, np.pi / 2], np.float32)
    sino = torch.stack([cp.project_tf_fast(torch.from_numpy(im).to(dev), theta, pad=False, dim=2)[..., 0] for im in imgs])
    masks, samples = cp.create_all_masks(sino, 2, str(tmp_path), 1e3, train=True, toy_masks=True, device=dev)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "ct_pvae_amd.mcmc", "--save_path", str(tmp_path), "-s", "300", "-b", "100", "--chains", "4", "--marginals",
           "--no_trace", "--ess_lags", "5", "--cov"]
    out = subprocess.run(cmd, check=True, env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert "ESS per pixel" in out.stdout and "minimum" in out.stdout and "median" in out.stdout
    m = cp.HmcMarginals.load(tmp_path / "hmc_marginals.npz", device=dev)
    assert m.shape == (2, 2) and m.count == 1200 and m.samples is None and m.max_lag == 5 and tuple(m.xx.shape) == (4, 4, 4)
    used = masks[0] > 0
    want = cp.hmc_marginals(samples[0][used], masks[0][used], theta[used.cpu().numpy()], 1e3, num_results=300, num_burnin_steps=100,
                            chains_per_object=4, max_lag=5, cov=True)
    base._equal_stats(m, want)
    _equal_new(m, want)
    assert np.array_equal(m.ess(), want.ess()) and np.all(np.isfinite(m.ess())) and np.all(m.ess() > 0)
    bad = subprocess.run(cmd[:-3] + ["--ess_lags", "65"], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert bad.returncode != 0 and "--ess_lags must be" in bad.stderr
