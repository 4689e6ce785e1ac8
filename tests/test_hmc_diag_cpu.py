"""hmc_marginals(max_lag=, cov=) without a GPU: the host finish of HmcMarginals (autocov, autocorr, ess, ess_truncated, cov, corr) from the
raw sums of the numpy twin (tests/np_twin_hmc_diag.py) against the direct centred estimators and against the law of AR(1) series, two
defective finishes that the bar must refuse, save / load, the LDS query and the argument checks of the call and of the entry point, and
that csrc/hmc_diagnostics.hip compiles for gfx950 without scratch memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_hmc_diag as twd
from tests import np_twin_hmc_marginals as twm
from tests.conftest import ROOT

GRID = dict(lo=0.005, width=0.01, bins=50)
EPS = float(np.finfo(np.float64).eps)
LDS_LIMIT = 160 * 1024
# everything of the model and the histogram at its maximum and cov on: the longest lag window the entry point then admits
LARGEST = dict(N=8, A=256, bins=254, max_lag=9, cov=1)


def _marginals(samples, cpo, max_lag, cov=True):
    """The HmcMarginals (on the CPU) a run with these stored samples [n][C][K] would return, by the twins."""
    import ct_pvae_amd as cp
    n, C, K = samples.shape
    N = int(round(K ** 0.5))
    hist, s1, s2, acc = twm.stats_from_samples(samples, np.ones((n, C), bool), chains_per_object=cpo, **GRID)
    lag, ring, head, xx = twd.raw_sums(samples, max_lag, cov)
    t = torch.from_numpy
    return cp.HmcMarginals((N, N), GRID["bins"], GRID["lo"], GRID["width"], n, cpo, t(hist), t(s1), t(s2), t(acc),
                           t(np.full(C, 0.05, np.float32)), None, None, t(lag), t(ring), t(head), None if xx is None else t(xx))


def _moving_average(n, C, K, seed, mean, std, taps=8):
    """float32 [n][C][K]: white noise averaged over `taps` steps (autocorrelation 1 - l / taps for l < taps), scaled to mean and std."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n + taps - 1, C, K))
    c = np.cumsum(e, axis=0)
    y = (c[taps - 1:] - np.concatenate([np.zeros((1, C, K)), c[:-taps]])) / np.sqrt(taps)
    return (mean + std * y).astype(np.float32)


def _bar(samples):
    """2.5 n eps (1 + (m / s)^2), relative to c_0 -- see test_finish_against_direct_on_correlated_series."""
    x = samples.astype(np.float64)
    n = x.shape[0]
    return 2.5 * n * EPS * (1.0 + float(np.max(np.abs(x.mean(0)) / x.std(0))) ** 2)


def _worst(got, want):
    """max over lags, chains and pixels of |got_l - want_l| / want_0."""
    return float(np.max(np.abs(got - want) / want[:, :1]))


SERIES = [(2 ** 12, 1e-3, 64), (2 ** 16, 1e-2, 64), (2 ** 20, 1e-3, 16), (2 ** 20, 0.1, 16)]


@pytest.mark.parametrize("n,std,max_lag", SERIES)
def test_finish_against_direct_on_correlated_series(n, std, max_lag):
    """autocov() from the raw sums against the direct centred estimator on float32 moving-average series of mean 0.25.

    The bar, relative to c_0 = s^2: c_l n = r_l - m (H_l + T_l) + (n - l) m^2, and each of the four terms is at most n (m^2 + s^2) in
    size.  r_l and S are strictly sequential float64 sums of n terms, each within (n - 1) u sum|terms| of the exact sum, u = eps / 2:
    r_l carries n u n (m^2 + s^2); S enters m (H_l + T_l) ~ 2 m S and (n - l) m^2 = (n - l) S^2 / n^2 with twice its relative error
    each, 2 n u n m^2 apiece.  Together at most 5 n u n (m^2 + s^2); divided by n c_0 = n s^2 that is 2.5 n eps (1 + (m / s)^2):
    3.6e-5 at n = 2^20 and m / s = 250.  (The direct estimator's own error, pairwise sums of centred values, is n-free and far below.)
    Measured worst case, relative to c_0: 4.4e-10 (n 2^12, s 1e-3), 4.2e-11 (2^16, 1e-2), 1.9e-8 (2^20, 1e-3), 2.4e-12 (2^20, 0.1);
    the sequential sums' errors grow like sqrt(n), not n, so the bound is loose by three orders and still refuses both controls below."""
    x = _moving_average(n, 2, 4, seed=n + max_lag, mean=0.25, std=std)
    m = _marginals(x, 2, max_lag, cov=False)
    got, want = m.autocov(), twd.autocov_direct(x, max_lag)
    assert got.shape == (2, max_lag + 1, 4) and got.dtype == np.float64
    worst, bar = _worst(got, want), _bar(x)
    print(f"n={n} std={std}: worst |autocov - direct| / c_0 = {worst:.3g}, bar {bar:.3g}")
    assert worst <= bar
    rho = m.autocorr()
    assert np.all(rho[:, 0] == 1.0) and np.all(np.isfinite(rho))
    np.testing.assert_allclose(rho[:, 4], 0.5, atol=0.2 if n < 2 ** 16 else 0.05)      # the series' law: 1 - 4 / 8


def _finish_without_centring(m):
    return m.lag.numpy() / m.num_results


def _finish_with_T_as_S(m):
    """autocov_from_sums with the sum of the last l values left out of T_l."""
    lag, head, S, n = m.lag.numpy(), m.head.numpy().astype(np.float64), m._chain_sums()[0], m.num_results
    mean = S / n
    out, first = np.zeros_like(lag), np.zeros_like(S)
    for l in range(lag.shape[1]):
        if l:
            first = first + head[:, l - 1]
        out[:, l] = (lag[:, l] - mean * ((S - first) + S) + (n - l) * mean * mean) / n
    return out


@pytest.mark.parametrize("n,std,max_lag", SERIES)
def test_the_bar_refuses_defective_finishes(n, std, max_lag):
    """Controls: the raw lagged product without centring, and T_l taken as S (the last l values not removed), both miss the bar of
    test_finish_against_direct_on_correlated_series on each of its series -- the second by about l (m / s)^2 / n at lag l."""
    x = _moving_average(n, 2, 4, seed=n + max_lag, mean=0.25, std=std)
    m = _marginals(x, 2, max_lag, cov=False)
    want, bar = twd.autocov_direct(x, max_lag), _bar(x)
    for finish in (_finish_without_centring, _finish_with_T_as_S):
        worst = _worst(finish(m), want)
        print(f"n={n} std={std} {finish.__name__}: {worst:.3g} against the bar {bar:.3g}")
        assert worst > 10 * bar


def test_finish_against_direct_on_near_zero_series():
    """Values around 1e-30 (where a Dirichlet concentration of 0.004 puts a pixel): the products are around 1e-60, far inside float64's
    range; the finish holds the same bar and autocorr has neither NaN nor inf."""
    rng = np.random.default_rng(5)
    x = (1e-30 * np.exp(rng.standard_normal((4096, 2, 4)))).astype(np.float32)
    m = _marginals(x, 2, 64)
    got, want = m.autocov(), twd.autocov_direct(x, 64)
    assert np.all(want[:, 0] > 0) and want[:, 0].max() < 1e-55
    worst = _worst(got, want)
    print(f"near zero: worst {worst:.3g}, bar {_bar(x):.3g}")
    assert worst <= _bar(x)
    assert np.all(np.isfinite(m.autocorr())) and np.all(np.isfinite(m.ess())) and np.all(np.isfinite(m.corr()))
    # a pixel that is exactly constant has c_0 = 0: NaN, not a made-up number
    x[:, 0, 1] = np.float32(2.0 ** -100)              # 7.9e-31, a power of two: every sum is exact, c_0 is 0 and not a rounding residue
    m = _marginals(x, 2, 4)
    assert np.all(np.isnan(m.autocorr()[0, 1:, 1])) and np.isnan(m.ess(cross_chain=False)[0, 1]) and np.isfinite(m.ess(cross_chain=False)[1, 1])


# worst |ess / law - 1| of the numpy twin over seeds 0 .. 19 (8 chains, n = 2^16, max_lag 64), cross-chain and per chain; measured by
# this file's _ar1_spread() on the CPU
AR1_SPREAD = {0.0: (0.0197, 0.0825), 0.5: (0.0275, 0.1441), 0.9: (0.0386, 0.1419)}
AR1_SEED = {0.0: 3, 0.5: 3, 0.9: 23}


def _ar1_case(phi, seed, max_lag=64):
    x = twd.ar1(phi, 2 ** 16, 8, 4, seed, mean=0.25, std=0.05)
    return _marginals(x, 8, max_lag, cov=False)


def _ar1_spread(seeds=range(20)):
    """What AR1_SPREAD holds: run by hand (python -c "from tests import test_hmc_diag_cpu as t; print(t._ar1_spread())")."""
    out = {}
    for phi in AR1_SPREAD:
        law = 2 ** 16 * (1 - phi) / (1 + phi)
        dev = [(np.abs(m.ess() / (8 * law) - 1).max(), np.abs(m.ess(cross_chain=False) / law - 1).max(), bool(m.ess_truncated().any()))
               for m in (_ar1_case(phi, s) for s in seeds)]
        out[phi] = (max(d[0] for d in dev), max(d[1] for d in dev), sum(d[2] for d in dev))
    return out


@pytest.mark.parametrize("phi", sorted(AR1_SPREAD))
def test_ess_follows_the_law_of_ar1_series(phi):
    """8 chains of n = 2^16 AR(1) values with coefficient phi: ESS = M n (1 - phi) / (1 + phi).  The twin's worst relative deviation
    from the law over seeds 0 .. 19, measured on the CPU: cross-chain 2.0 % (phi 0), 2.8 % (0.5), 3.9 % (0.9); per chain 8.3 %, 14.4 %,
    14.2 % (AR1_SPREAD).  Asserted at three times that, on the seed AR1_SEED names.

    The flag: with a window of 8 lags every sequence of phi = 0.9 is still positive (rho_8 = 0.43) and flagged; for phi 0 and 0.5 no
    sequence of seeds 0 .. 19 reaches lag 64.  For phi = 0.9 the TRUE sequence is positive at every lag, and whether the estimate
    ends before lag 64 is decided by its noise: the pair sum of lags 62 and 63 is 2.8e-3, the standard error of the cross-chain
    estimate 4.3e-3 per lag, and 42 of the 96 pixels of seeds 0 .. 23 end before it.  Seed 23 is one whose four pixels all do, so "false
    at 64" checks that a sequence which ended is not flagged -- on data where it did end -- and no law."""
    m = _ar1_case(phi, seed=AR1_SEED[phi])
    law = 2 ** 16 * (1 - phi) / (1 + phi)
    ess, per_chain = m.ess(), m.ess(cross_chain=False)
    assert ess.shape == (1, 4) and per_chain.shape == (8, 4) and ess.dtype == np.float64
    dev, dev1 = np.abs(ess / (8 * law) - 1).max(), np.abs(per_chain / law - 1).max()
    print(f"phi={phi}: cross-chain deviation {dev:.4f}, per chain {dev1:.4f}")
    assert dev <= 3 * AR1_SPREAD[phi][0] and dev1 <= 3 * AR1_SPREAD[phi][1]
    assert m.ess_truncated().shape == (1, 4) and m.ess_truncated(cross_chain=False).shape == (8, 4)
    assert not m.ess_truncated().any()                                      # the sequence ended before lag 64
    if phi == 0.9:
        short = _ar1_case(phi, seed=AR1_SEED[phi], max_lag=8)
        assert short.ess_truncated().all() and short.ess_truncated(cross_chain=False).all()
        assert np.all(short.ess() > ess)                                    # cut by the window: an upper bound, and flagged as one


def test_cov_against_numpy_and_its_errors():
    import ct_pvae_amd as cp
    rng = np.random.default_rng(2)
    x = rng.dirichlet(np.full(4, 3.0), (500, 6)).astype(np.float32)
    m = _marginals(x, 3, 5)
    want = twd.cov_direct(x, 3)
    assert m.cov().shape == (2, 4, 4) and m.cov().dtype == np.float64
    np.testing.assert_allclose(m.cov(), want, rtol=0, atol=1e-12 * 500 * 3)       # entries ~ 1e-2; sums of 1500 products below 1
    d = np.sqrt(np.einsum("bkk->bk", want))
    np.testing.assert_allclose(m.corr(), want / (d[:, :, None] * d[:, None, :]), rtol=0, atol=1e-9)
    assert np.all(np.abs(m.cov().sum(-1)) <= 1e-6 * np.abs(m.cov()).max())          # points of the simplex
    assert np.all(np.abs(m.corr()[:, np.arange(4), np.arange(4)] - 1.0) <= 4 * EPS) and (m.corr()[0][~np.eye(4, dtype=bool)] < 0).all()
    plain = cp.HmcMarginals((2, 2), 50, 0.005, 0.01, 500, 3, m.hist, m.s1, m.s2, m.accepted, m.step_size)
    assert plain.max_lag == 0 and plain.lag is None and plain.xx is None
    for call in (plain.autocov, plain.autocorr, plain.ess, plain.ess_truncated):
        with pytest.raises(ValueError, match="max_lag >= 1"):
            call()
    for call in (plain.cov, plain.corr):
        with pytest.raises(ValueError, match="cov=True"):
            call()
    with pytest.raises(ValueError, match="come together"):
        cp.HmcMarginals((2, 2), 50, 0.005, 0.01, 500, 3, m.hist, m.s1, m.s2, m.accepted, m.step_size, lag=m.lag)
    with pytest.raises(ValueError, match="do not fit"):
        cp.HmcMarginals((2, 2), 50, 0.005, 0.01, 500, 3, m.hist, m.s1, m.s2, m.accepted, m.step_size, lag=m.lag, ring=m.ring, head=m.ring)
    with pytest.raises(ValueError, match="xx must be"):
        cp.HmcMarginals((2, 2), 50, 0.005, 0.01, 500, 3, m.hist, m.s1, m.s2, m.accepted, m.step_size, xx=m.xx[:1])


def test_short_runs():
    """Fewer kept steps than lags: the lags >= n are exact zeros, and so is their autocovariance; n = 1 and n = 2 do not fail."""
    x = _moving_average(5, 2, 4, seed=1, mean=0.25, std=0.05)
    m = _marginals(x, 2, 8)
    c = m.autocov()
    assert np.all(c[:, 5:] == 0.0) and np.all(m.lag.numpy()[:, 5:] == 0.0) and np.all(m.head.numpy()[:, 5:] == 0.0)
    np.testing.assert_allclose(c, twd.autocov_direct(x, 8), rtol=0, atol=1e-15)
    assert not m.ess_truncated().any()
    for n in (1, 2):
        m = _marginals(x[:n], 2, 3)
        assert m.autocov().shape == (2, 4, 4) and m.ess().shape == (1, 4)


def test_save_load_carries_the_new_arrays(tmp_path):
    import ct_pvae_amd as cp
    x = _moving_average(40, 4, 4, seed=3, mean=0.25, std=0.05)
    for max_lag, cov in ((5, True), (5, False)):
        m = _marginals(x, 2, max_lag, cov)
        m.save(tmp_path / "d.npz")
        b = cp.HmcMarginals.load(tmp_path / "d.npz", device="cpu")
        assert b.max_lag == 5 and (b.xx is None) == (not cov)
        for k in ("hist", "s1", "s2", "accepted", "step_size", "lag", "ring", "head") + (("xx",) if cov else ()):
            assert torch.equal(getattr(m, k), getattr(b, k)) and getattr(m, k).dtype == getattr(b, k).dtype, k
        assert np.array_equal(b.ess(), m.ess())
        with np.load(tmp_path / "d.npz") as f:
            assert str(f["head"]) == "hmc" and f["lag_head"].shape == (4, 5, 4)
    # a file written without them loads as before
    plain = cp.HmcMarginals((2, 2), 50, 0.005, 0.01, 40, 2, m.hist, m.s1, m.s2, m.accepted, m.step_size)
    plain.save(tmp_path / "p.npz")
    with np.load(tmp_path / "p.npz") as f:
        assert not {"lag", "ring", "lag_head", "xx"} & set(f.files)
    b = cp.HmcMarginals.load(tmp_path / "p.npz", device="cpu")
    assert b.max_lag == 0 and b.lag is None and b.ring is None and b.head is None and b.xx is None and torch.equal(b.s1, m.s1)


def test_lds_query():
    """The query is monotone in each argument; the largest admitted request (LARGEST) is under the limit and one more lag is over it; the
    over-budget request is refused by the call, with CPU tensors -- before the device check, so before any launch -- and by the entry
    point before any HIP call, naming the three knobs."""
    import ct_pvae_amd as cp
    from ct_pvae_amd import _lib, mcmc
    lib = _lib.load()
    q = lib.ctpvae_hmc_diagnostics_lds_bytes
    assert mcmc.LDS_BYTES_PER_WORKGROUP == LDS_LIMIT and mcmc.MAX_LAG == 64
    # with both features off: the marginals' request rounded up to 8
    for N, A, bins in ((2, 2, 50), (3, 7, 5), (8, 256, 254)):
        assert q(N, A, bins, 0, 0) == (lib.ctpvae_hmc_marginals_lds_bytes(N, A, bins) + 7) // 8 * 8
    assert q(3, 7, 5, 4, 0) - q(3, 7, 5, 0, 0) == (5 * 9 * 4 + 4) + 5 * 9 * 8 and q(3, 7, 5, 0, 1) - q(3, 7, 5, 0, 0) == 9 * 9 * 8
    assert q(8, 256, 254, 64, 1) == 205856 > LDS_LIMIT
    base = dict(N=3, A=7, bins=5, max_lag=2, cov=0)
    for key, values in (("N", range(2, 9)), ("A", (1, 2, 7, 8, 9, 64, 255, 256)), ("bins", (1, 2, 5, 6, 253, 254)),
                        ("max_lag", range(0, 65)), ("cov", (0, 1))):
        for other_cov in (0, 1):
            sizes = [q(*{**base, "cov": other_cov, key: v}.values()) for v in values]
            assert all(b > a for a, b in zip(sizes, sizes[1:])), (key, sizes)
            assert all(s % 8 == 0 and s > 0 for s in sizes)
    assert q(*LARGEST.values()) == 163616 <= LDS_LIMIT < q(*dict(LARGEST, max_lag=10).values())
    assert q(*dict(LARGEST, cov=0, max_lag=51).values()) <= LDS_LIMIT < q(*dict(LARGEST, cov=0, max_lag=52).values())
    assert q(9, 2, 5, 1, 0) == q(2, 257, 5, 1, 0) == q(2, 2, 0, 1, 0) == q(2, 2, 5, -1, 0) == q(2, 2, 5, 65, 0) == _lib.EINVAL
    # the call: 8 x 8 pixels, 256 angles
    meas, mask, th = torch.zeros(256, 8), torch.ones(256), np.zeros(256)
    with pytest.raises(ValueError, match="lower bins or max_lag, or turn cov off"):
        cp.hmc_marginals(meas, mask, th, 1e3, prior=(np.ones(1), np.ones((1, 64))), num_results=4, bins=254, max_lag=64, cov=True)
    with pytest.raises(ValueError, match="bytes of LDS"):
        cp.hmc_marginals(meas, mask, th, 1e3, prior=(np.ones(1), np.ones((1, 64))), num_results=4, bins=254, max_lag=10, cov=True)
    with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):       # LARGEST passes the size check
        cp.hmc_marginals(meas, mask, th, 1e3, prior=(np.ones(1), np.ones((1, 64))), num_results=4, bins=254, max_lag=9, cov=True)
    # the entry point
    buf = np.zeros(8, np.float64)
    p = buf.ctypes.data
    rc = lib.ctpvae_hmc_run_diagnostics_f32(p, 2, 0, 1, 8, p, p, 256, p, p, 1e3, 1, p, p, p, 5, 8, 0, 0, 0, None, None, None, None, 4, 0.0, 2e-4,
                                            254, p, p, p, 64, p, p, p, p, None)
    assert rc == _lib.EINVAL
    assert all(w in _lib.last_error() for w in ("bins", "max_lag", "cov", "205856", "163840")), _lib.last_error()


def test_argument_checks():
    import ct_pvae_amd as cp
    from ct_pvae_amd import _lib
    meas, mask, th = torch.zeros(2, 2), torch.ones(2), [0.0, 1.5]
    for bad in (-1, 65, 2.5, True):
        with pytest.raises(ValueError, match="^hmc_marginals: max_lag must be"):
            cp.hmc_marginals(meas, mask, th, 1e3, num_results=4, max_lag=bad)
    with pytest.raises(ValueError, match="bins must be"):                   # the grid is still checked, and first
        cp.hmc_marginals(meas, mask, th, 1e3, num_results=4, max_lag=-1, bins=0)
    for ok in (dict(max_lag=64), dict(cov=True), dict(max_lag=1, cov=True)):
        with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):
            cp.hmc_marginals(meas, mask, th, 1e3, num_results=4, **ok)
    lib = _lib.load()
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data

    def run(**bad):
        a = dict(state=p, N=2, n=8, outs=(p, p, p, p), bins=50, hist=p, mom=p, acc=p, max_lag=3, lag=p, ring=p, head=p, xx=p)
        a.update(bad)
        return lib.ctpvae_hmc_run_diagnostics_f32(a["state"], 2, 0, 1, a["N"], p, p, 2, p, p, 1e3, 1, p, p, p, 5, a["n"], 0, 0, 0, *a["outs"], 4,
                                                  0.005, 0.01, a["bins"], a["hist"], a["mom"], a["acc"], a["max_lag"], a["lag"], a["ring"],
                                                  a["head"], a["xx"], None)

    cases = [(dict(max_lag=-1), "max_lag"), (dict(max_lag=65), "max_lag"), (dict(lag=None), "lag, ring and head"),
             (dict(ring=None), "lag, ring and head"), (dict(head=None), "lag, ring and head"), (dict(lag=p + 4), "aligned"),
             (dict(ring=p + 2), "aligned"), (dict(xx=p + 4), "aligned"), (dict(max_lag=0), "max_lag=0"),
             (dict(hist=None), "null state"), (dict(mom=p + 4), "aligned"), (dict(bins=255), "bins"), (dict(outs=(p, None, p, p)), "per-step"),
             (dict(state=None), "null pointer"), (dict(N=9), "pixels"), (dict(n=0), "transitions"), (dict(n=10 ** 6), "transitions")]
    for bad, word in cases:
        assert run(**bad) == _lib.EINVAL, bad
        assert word in _lib.last_error(), (bad, _lib.last_error())


def test_hmc_diagnostics_kernel_uses_no_scratch():
    """The check test_hmc_marginals_kernel_uses_no_scratch makes, for hmc_diagnostics.hip under the Makefile's flags."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    csrc = os.path.join(ROOT, "ct_pvae_amd", "csrc")
    flags = re.search(r"^HIPFLAGS \?= (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "--offload-arch=gfx950" in flags
    out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "hmc_diagnostics.hip", "-o", os.devnull], cwd=csrc,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    static_lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr)]
    assert sum("hmc_diag_kernel" in n for n in names) == 1 and not any("hmc_stats_kernel" in n for n in names) and len(scratch) == len(names)
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
    assert all(v == 0 for v in static_lds)        # the largest admitted request leaves 224 bytes: no room for static LDS
    assert "hmc_diagnostics.hip" in open(os.path.join(csrc, "Makefile")).read().split("SRCS :=")[1].splitlines()[0]
