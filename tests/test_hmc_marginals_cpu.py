"""hmc_marginals without a GPU: the numpy twin of its statistics (tests/np_twin_hmc_marginals.py) against plain loops, the formulas of
HmcMarginals against numpy on synthetic samples, save / load, hist_distance, the argument checks of the Python call and of the entry
point, and that csrc/hmc_marginals.hip compiles for gfx950 without scratch memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_hmc_marginals as twm
from tests.conftest import ROOT

GRID = dict(lo=0.005, width=0.01, bins=50)


def _synthetic(R=400, C=6, K=4, seed=0):
    rng = np.random.default_rng(seed)
    walk = rng.dirichlet(np.full(K, 3.0), (R, C)) * (1 + 0.1 * np.arange(C))[None, :, None] / 2     # chains that disagree a little
    return walk.astype(np.float32), rng.random((R, C)) < 0.7


def _write_npz(path, samples, accepted, cpo, grid=GRID, N=2):
    hist, s1, s2, acc = twm.stats_from_samples(samples, accepted, chains_per_object=cpo, **grid)
    R, C, _ = samples.shape
    np.savez(path, hist=hist, s1=s1, s2=s2, accepted=acc, step_size=np.full(C, 0.05, np.float32), shape=np.array([N, N]),
             bins=np.int64(grid["bins"]), lo=np.float64(grid["lo"]), width=np.float64(grid["width"]), num_results=np.int64(R),
             chains_per_object=np.int64(cpo), count=np.int64(R * cpo), head=np.str_("hmc"),
             edges=grid["lo"] + grid["width"] * np.arange(grid["bins"] + 1))
    return hist, s1, s2, acc


def test_the_twin_against_plain_loops():
    """A case of a few rows, an odd number of them (halves of 2 and 3 rows), NaN and out-of-range samples included."""
    from ct_pvae_amd import marginals
    rng = np.random.default_rng(1)
    R, C, K, cpo, lo, width, bins = 5, 4, 3, 2, 0.2, 0.1, 4
    x = rng.random((R, C, K)).astype(np.float32)
    x[1, 2, 0], x[3, 1, 1], x[4, 0, 2] = np.nan, 7.0, -1.0
    acc = rng.random((R, C)) < 0.5
    hist, s1, s2, got_acc = twm.stats_from_samples(x, acc, lo, width, bins, cpo)
    want_h = np.zeros((C // cpo, K, bins + 2), np.int64)
    want_1, want_2 = np.zeros((2, C, K)), np.zeros((2, C, K))
    col = marginals.bin_columns(x, lo, width, bins)
    for r in range(R):
        for c in range(C):
            for k in range(K):
                want_h[c // cpo, k, col[r, c, k]] += 1
                v = float(x[r, c, k])
                want_1[int(r >= R // 2), c, k] += v
                want_2[int(r >= R // 2), c, k] += v * v
    assert np.array_equal(hist, want_h) and hist.sum() == R * C * K
    assert hist[1, 0, 0] >= 1 and hist[0, 1, bins + 1] >= 1 and hist[0, 2, 0] >= 1            # NaN, above, below
    assert np.array_equal(s1, want_1, equal_nan=True) and np.array_equal(s2, want_2, equal_nan=True)
    assert np.isnan(s1[0, 2, 0]) and np.isnan(s2[0, 2, 0]) and np.isfinite(s1[1, 2, 0])
    assert np.array_equal(got_acc, np.array([sum(bool(acc[r, c]) for r in range(R)) for c in range(C)]))
    # one row: everything is half 1
    _, a1, _, _ = twm.stats_from_samples(x[:1], acc[:1], lo, width, bins, cpo)
    assert np.all(a1[0][~np.isnan(a1[0])] == 0) and np.array_equal(a1[1], x[0].astype(np.float64))


def test_formulas_against_numpy_on_the_samples(tmp_path):
    """rhat, mean, std, chain_mean, accept_rate of a state loaded from a synthetic file against numpy on the samples, relative 1e-9:
    the values lie in (0, 1) and n is a few hundred, so s2 - s1^2 / n amplifies float64 rounding by about 1e3."""
    import ct_pvae_amd as cp
    samples, accepted = _synthetic()
    R, C, K = samples.shape
    cpo = 3
    _write_npz(tmp_path / "m.npz", samples, accepted, cpo)
    m = cp.HmcMarginals.load(tmp_path / "m.npz", device="cpu")
    assert (m.shape, m.bins, m.lo, m.width, m.num_results, m.chains_per_object, m.count) == ((2, 2), 50, 0.005, 0.01, R, cpo, R * cpo)
    assert m.samples is None and m.trace is None and np.array_equal(m.edges, 0.005 + 0.01 * np.arange(51))
    x = samples.astype(np.float64)
    pooled = x.reshape(R, C // cpo, cpo, K).transpose(1, 0, 2, 3).reshape(C // cpo, R * cpo, K)
    np.testing.assert_allclose(m.mean(), pooled.mean(1).reshape(-1, 2, 2), rtol=1e-9, atol=0)
    np.testing.assert_allclose(m.std(), pooled.std(1, ddof=1).reshape(-1, 2, 2), rtol=1e-9, atol=0)
    np.testing.assert_allclose(m.chain_mean(), x.mean(0), rtol=1e-9, atol=0)
    np.testing.assert_allclose(m.accept_rate(), accepted.mean(0), rtol=1e-9, atol=0)
    want = twm.rhat_from_samples(samples, cpo)
    assert want.shape == (2, K) and np.all(want > 1.0)
    np.testing.assert_allclose(m.rhat(), want, rtol=1e-9, atol=0)
    np.testing.assert_allclose(cp.split_rhat(m.s1.numpy(), m.s2.numpy(), R // 2, cpo), want, rtol=1e-9, atol=0)
    assert m.mean().dtype == m.std().dtype == m.rhat().dtype == np.float64
    # chains that never move: W = 0 is not hidden
    flat = np.full(samples.shape, 0.25, np.float32)            # every sum is exact: W is 0, not a rounding residue
    _write_npz(tmp_path / "flat.npz", flat, accepted, cpo)
    assert not np.isfinite(cp.HmcMarginals.load(tmp_path / "flat.npz", device="cpu").rhat()).any()


@pytest.mark.parametrize("R", [3, 7, 2])
def test_rhat_needs_an_even_number_of_results(tmp_path, R):
    import ct_pvae_amd as cp
    samples, accepted = _synthetic(R=R)
    _write_npz(tmp_path / "m.npz", samples, accepted, 3)
    m = cp.HmcMarginals.load(tmp_path / "m.npz", device="cpu")
    with pytest.raises(ValueError, match="even num_results >= 4"):
        m.rhat()
    assert m.mean().shape == (2, 2, 2)


def test_save_load_round_trip(tmp_path):
    import ct_pvae_amd as cp
    samples, accepted = _synthetic(R=10)
    hist, s1, s2, acc = twm.stats_from_samples(samples, accepted, chains_per_object=2, **GRID)
    t = torch.from_numpy
    trace = dict(log_accept_ratio=t(np.random.default_rng(2).normal(size=(10, 6)).astype(np.float32)), is_accepted=t(accepted),
                 target_log_prob=t(np.zeros((10, 6), np.float32)), step_size=t(np.full(6, 0.03, np.float32)))
    for kept in (False, True):
        m = cp.HmcMarginals((2, 2), 50, 0.005, 0.01, 10, 2, t(hist), t(s1), t(s2), t(acc), t(np.full(6, 0.03, np.float32)),
                            t(samples) if kept else None, trace if kept else None)
        m.save(tmp_path / "rt.npz")
        b = cp.HmcMarginals.load(tmp_path / "rt.npz", device="cpu")
        for k in ("hist", "s1", "s2", "accepted", "step_size"):
            assert torch.equal(getattr(m, k), getattr(b, k)) and getattr(m, k).dtype == getattr(b, k).dtype, k
        assert (b.shape, b.bins, b.lo, b.width, b.num_results, b.chains_per_object, b.count) == ((2, 2), 50, 0.005, 0.01, 10, 2, 20)
        with np.load(tmp_path / "rt.npz") as f:
            assert str(f["head"]) == "hmc" and np.array_equal(f["edges"], m.edges) and int(f["count"]) == 20
        if kept:
            assert torch.equal(b.samples, m.samples) and set(b.trace) == set(trace)
            assert all(torch.equal(b.trace[k], trace[k]) for k in trace)
        else:
            assert b.samples is None and b.trace is None
    cp.PixelMarginals((2, 2), device="cpu").save(tmp_path / "pvae.npz")
    with pytest.raises(ValueError, match="head"):
        cp.HmcMarginals.load(tmp_path / "pvae.npz", device="cpu")


def test_hist_distance():
    import ct_pvae_amd as cp
    a = np.array([[4, 0, 0], [1, 1, 2], [0, 0, 0], [3, 3, 0]])
    b = np.array([[0, 0, 9], [2, 2, 4], [1, 0, 0], [1, 0, 1]])
    d = cp.hist_distance(a, b)
    assert d.dtype == np.float64 and d.shape == (4,)
    assert d[0] == 1.0 and d[1] == 0.0 and np.isnan(d[2]) and d[3] == 0.5 * (0.0 + 0.5 + 0.5)
    assert np.array_equal(cp.hist_distance(torch.from_numpy(a), b), d, equal_nan=True)
    with pytest.raises(ValueError):
        cp.hist_distance(a, b[:, :2])
    with pytest.raises(ValueError):
        cp.hist_distance(a.astype(np.float64), b)


def test_hmc_marginals_argument_errors():
    """Every error case of test_hmc_sample_argument_errors raises from hmc_marginals too; the grid is checked before the device."""
    import ct_pvae_amd as cp
    from ct_pvae_amd._lib import RadonLibraryError
    ok = dict(num_results=4)
    meas, mask, th = torch.zeros(2, 2), torch.ones(2), [0.0, 1.5]
    with pytest.raises(ValueError, match="64 pixels"):
        cp.hmc_marginals(torch.zeros(2, 9), mask, th, 1e3, **ok)
    with pytest.raises(ValueError, match="square"):
        cp.hmc_marginals(torch.zeros(3, 2), mask, th, 1e3, **ok)
    with pytest.raises(ValueError, match="concentrations must be"):
        cp.hmc_marginals(meas, mask, th, 1e3, prior=(np.ones(1), np.ones((1, 6))), **ok)
    with pytest.raises(ValueError, match="256 angles"):
        cp.hmc_marginals(torch.zeros(257, 2), torch.ones(257), np.zeros(257), 1e3, **ok)
    with pytest.raises(ValueError, match="mixture of 1 .. 4"):
        cp.hmc_marginals(meas, mask, th, 1e3, prior=(np.full(5, 0.2), np.ones((5, 4))), **ok)
    with pytest.raises(ValueError, match="positive"):
        cp.hmc_marginals(meas, mask, th, 1e3, prior=(np.ones(1), np.array([[1.0, 0.0, 1.0, 1.0]])), **ok)
    for bad in ([0.5, 0.5, 0.0, 0.0], [0.5, 0.7, -0.1, -0.1], [0.5, 0.5, float("nan"), 0.0], [0.5, 0.5, float("inf"), 0.0]):
        with pytest.raises(ValueError, match="initial_state"):
            cp.hmc_marginals(meas, mask, th, 1e3, initial_state=[bad], **ok)
    with pytest.raises(ValueError, match="chain id"):
        cp.hmc_marginals(meas, mask, th, 1e3, first_chain=2 ** 32 - 2, chains_per_object=3, **ok)
    with pytest.raises(ValueError, match="steps_per_launch"):
        cp.hmc_marginals(meas, mask, th, 1e3, steps_per_launch=10 ** 6, **ok)
    with pytest.raises(TypeError, match="torch tensors"):
        cp.hmc_marginals(np.zeros((2, 2)), mask, th, 1e3, **ok)
    for grid in (dict(bins=0), dict(bins=255), dict(width=0.0), dict(width=-1.0), dict(lo=float("nan")), dict(lo=float("inf")),
                 dict(width=1e-60)):
        with pytest.raises(ValueError, match="bins must be|lo and width"):
            cp.hmc_marginals(meas, mask, th, 1e3, **grid, **ok)
    with pytest.raises(RadonLibraryError, match="no CPU path"):
        cp.hmc_marginals(meas, mask, th, 1e3, **ok)
    with pytest.raises(RadonLibraryError, match="no CPU path"):
        cp.hmc_marginals(meas, mask, th, 1e3, keep_samples=True, bins=254, **ok)
    # the error names the function that was called
    with pytest.raises(ValueError, match="^hmc_marginals:"):
        cp.hmc_marginals(meas, mask, th, 1e3, num_results=0)
    with pytest.raises(ValueError, match="^hmc_sample:"):
        cp.hmc_sample(meas, mask, th, 1e3, num_results=0)


def test_the_entry_point_refuses_bad_arguments_before_any_hip_call():
    from ct_pvae_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    assert p % 8 == 0

    def run(**bad):
        a = dict(state=p, C=2, cpo=1, N=2, A=2, M=1, L=5, n=8, outs=(p, p, p, p), lo=0.005, width=0.01, bins=50, hist=p, mom=p, acc=p)
        a.update(bad)
        return lib.ctpvae_hmc_run_marginals_f32(a["state"], a["C"], 0, a["cpo"], a["N"], p, p, a["A"], p, p, 1e3, a["M"], p, p, p, a["L"],
                                                a["n"], 0, 0, 0, *a["outs"], 4, a["lo"], a["width"], a["bins"], a["hist"], a["mom"],
                                                a["acc"], None)

    cases = [(dict(hist=None), "null state"), (dict(mom=None), "null state"), (dict(acc=None), "null state"),
             (dict(hist=p + 4), "aligned"), (dict(mom=p + 4), "aligned"), (dict(acc=p + 4), "aligned"),
             (dict(bins=0), "bins"), (dict(bins=255), "bins"), (dict(width=0.0), "width"), (dict(lo=float("nan")), "width"),
             (dict(outs=(p, None, p, p)), "per-step"), (dict(outs=(None, None, None, p)), "per-step"), (dict(outs=(None, p, p, p)), "per-step"),
             (dict(outs=(None,) * 4, bins=0), "bins"), (dict(state=None), "null pointer"),
             (dict(N=9), "pixels"), (dict(A=257), "angles"), (dict(M=5), "mixture"), (dict(L=0), "leapfrog"), (dict(n=10 ** 6), "transitions"),
             (dict(n=0), "transitions"), (dict(C=3, cpo=2), "chains")]
    for bad, word in cases:
        assert run(**bad) == _lib.EINVAL, bad
        assert word in _lib.last_error(), (bad, _lib.last_error())
    # the size query: the sampler's tables plus K * (bins + 2) counts of 4 bytes; at most 121 KiB, under the 160 KiB of a CU
    q = lib.ctpvae_hmc_marginals_lds_bytes
    assert q(2, 2, 50) - q(2, 2, 1) == 4 * 49 * 4 and q(8, 256, 254) - q(8, 256, 1) == 64 * 253 * 4
    assert q(8, 256, 254) == 64 * 256 * 4 + (68 + 2052 + 2 * 2048) * 4 + 2048 * 8 + 256 * 64 <= 121 * 1024
    assert q(9, 2, 50) == q(2, 257, 50) == q(2, 2, 0) == q(2, 2, 255) == _lib.EINVAL


def test_hmc_marginals_kernel_uses_no_scratch():
    """The check test_hmc_kernels_use_no_scratch makes for hmc.hip, for hmc_marginals.hip under the Makefile's flags."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    csrc = os.path.join(ROOT, "ct_pvae_amd", "csrc")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "--offload-arch=gfx950" in flags
    out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "hmc_marginals.hip", "-o", os.devnull], cwd=csrc,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert sum("hmc_stats_kernel" in n for n in names) == 1 and not any("hmc_kernel" in n for n in names) and len(scratch) == len(names)
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
    assert "hmc_marginals.hip" in open(os.path.join(csrc, "Makefile")).read().split("SRCS :=")[1].splitlines()[0]
