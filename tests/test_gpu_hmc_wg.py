"""The workgroup form of the HMC sampler (hmc_sample(form="workgroup"), csrc/hmc_wg.hip) on the GPU: bit for bit against the wave
form where a workgroup is one wave, and against the numpy restatement (tests/np_twin_hmc.py) where it is two to sixteen."""
import functools

import numpy as np
import pytest

from tests import np_twin_hmc as tw
from tests import np_twin_hmc_wg as wg

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import radon_oracle
    radon_oracle.build()
    return radon_oracle


@functools.lru_cache(maxsize=None)
def _twins(name):
    return wg.twin_runs(_oracle(), name, 8)


@functools.lru_cache(maxsize=None)
def _case(N, A, M, seed):
    return tw.target_case(_oracle(), N, A, M, seed, wg.C)


def _sample(pb, **kw):
    import torch

    import ct_pvae_amd as cp
    dev = torch.device("cuda", 0)
    meas, mask = torch.from_numpy(pb["meas"]).to(dev), torch.from_numpy(pb["mask"]).to(dev)
    kw.setdefault("prior", pb["prior"])
    samples, trace = cp.hmc_sample(meas, mask, pb["theta"], pb["pnm"], **kw)
    torch.cuda.synchronize()
    return samples.cpu().numpy(), {k: v.cpu().numpy() for k, v in trace.items()}


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    assert sorted(a[1]) == sorted(b[1])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("name", ["toy", "n5", "n8"])
def test_one_wave_workgroups_equal_the_wave_form_bit_for_bit(name):
    """With N <= 8 a workgroup is one wave and does the wave form's operations: 100 chains, 48 results after 16 burn-in steps, 24
    adaptation steps, 16 steps per launch -- samples, the three traces and step_size are array_equal between the forms."""
    pb = tw.problem(_oracle(), name)
    kw = dict(num_results=48, num_burnin_steps=16, num_adaptation_steps=24, chains_per_object=100, step_size=tw.STEP[name],
              seed=tw.SEEDS[name], steps_per_launch=16, initial_state=tw.random_starts(name, 100))
    wave = _sample(pb, **kw)
    assert not np.isnan(wave[0]).any() and wave[1]["is_accepted"].any() and len(np.unique(wave[1]["step_size"])) > 1
    _same(wave, _sample(pb, form="workgroup", **kw))


@pytest.mark.parametrize("name", list(wg.SHAPES))
def test_the_wide_shapes_against_the_twin(name):
    """64 chains from random simplex starts at the five wide shapes, 8 transitions of 5 leapfrog steps: log_accept_ratio, the decision,
    the sample and target_log_prob against the float64 twin within max(1e-5 scale, 8 max|twin32 - twin64|)
    (np_twin_hmc.check_against_twin), over the first transition with at most 5 % of the chains left out and over all eight with at most
    20 %; |sum_k O_k - 1| <= max(1e-5, 8 x the float32 twin's own worst).
    Seen on the MI355X (fraction left out; worst error / bar for log_accept_ratio, sample, target_log_prob; |sum O - 1|, twin32's):
      1 step:  w9 0, 0.12 / 0.04 / 0.03;  w12 0, 0.12 / 0.05 / 0.02;  w16 0, 0.19 / 0.06 / 0.03;  w23 0, 0.17 / 0.10 / 0.06;
               w32 0.031, 0.19 / 0.06 / 0.07
      8 steps: w9 0, 0.18 / 0.06 / 0.03;  w12 0, 0.14 / 0.05 / 0.02;  w16 0.016, 0.19 / 0.08 / 0.04;  w23 0.047, 0.20 / 0.12 / 0.07;
               w32 0.047, 0.19 / 0.11 / 0.08
      sums:    w9 7.9e-8 (1.7e-7);  w12 8.0e-8 (2.3e-7);  w16 9.3e-8 (3.3e-7);  w23 8.0e-8 (4.4e-7);  w32 1.1e-7 (8.0e-7)
    -- the fractions left out are exactly those of the float32 restatement against the float64 one (tests/test_hmc_wg_cpu.py), and
    the device sits well inside the factor 8."""
    pb, starts, t32, t64 = _twins(name)
    samples, tr = _sample(pb, form="workgroup", num_results=8, num_adaptation_steps=0, chains_per_object=wg.C, initial_state=starts,
                          step_size=wg.STEP, seed=wg.SEED, num_leapfrog_steps=wg.L)
    assert samples.shape == (8, wg.C, pb["N"] ** 2) and samples.dtype == np.float32
    assert not np.isnan(samples).any()
    got = dict(samples=samples, lar=tr["log_accept_ratio"], acc=tr["is_accepted"], target=tr["target_log_prob"])
    for n, cap in wg.CAPS.items():
        left, worst = tw.check_against_twin(wg.first(t32, n), wg.first(t64, n), wg.first(got, n))
        print(f"{name} x {n}: left out {left:.4f}, worst error / bar {worst}")
        assert left <= cap
    own = np.abs(t32["samples"].astype(np.float64).sum(-1) - 1.0).max()
    err = np.abs(samples.astype(np.float64).sum(-1) - 1.0).max()
    print(f"{name}: |sum O - 1| {err:.3g}, twin32's {own:.3g}")
    assert err <= max(1e-5, 8.0 * own)


def _init_state(N, theta, mask, meas, prior, starts, C):
    """ctpvae_hmc_wg_init_f32 on C chains of one object into a NaN-filled state of C + 1 rows (the last one a guard): the rows as numpy."""
    import torch

    from ct_pvae_amd import _lib, forward_functions
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    K, A = N * N, len(theta)
    T8, Tinv8 = forward_functions.rotate_tables(theta, N, N, dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    logw, alpha, lbeta = (up(a) for a in tw.prior_tables(*prior))
    assert alpha.shape == (len(logw), K)
    mask_d, meas_d, start = up(mask), up(meas), up(starts)
    assert mask_d.shape == (1, A) and meas_d.shape == (1, A, N) and start.shape == (C, K)
    state = torch.full((C + 1, 2 * K + 1), float("nan"), dtype=torch.float32, device=dev)
    assert lib.ctpvae_hmc_wg_state_floats(K) == state.shape[1]
    with torch.cuda.device(dev):
        _lib.check(lib.ctpvae_hmc_wg_init_f32(state.data_ptr(), C, C, N, T8.data_ptr(), Tinv8.data_ptr(), A, mask_d.data_ptr(),
                                              meas_d.data_ptr(), float(tw.TARGET_PNM), len(logw), logw.data_ptr(), alpha.data_ptr(),
                                              lbeta.data_ptr(), start.data_ptr(), 0.0123, forward_functions._stream_ptr()), "hmc_wg_init")
        torch.cuda.synchronize()
    return state.cpu().numpy()


@pytest.mark.parametrize("N,A,M,seed", list(wg.target_cases()))
def test_the_evaluator_against_the_twin(N, A, M, seed):
    """The state that ctpvae_hmc_wg_init_f32 stores for 64 chains, 32 of them started with one denormal pixel: x, dT/dx and T against
    the float64 twin AT THE DEVICE'S OWN x, per chain, within max(1e-5 scale, 8 |twin32 - twin64|) (np_twin_hmc.check_target); the
    step size, the step index and the guard row behind the state.  At most 2 of the 64 chains left out (the restatement leaves none at
    its own x, tests/test_hmc_wg_cpu.py: the allowance is for the band around FLT_MIN at the device's x).
    Seen on the MI355X over the 22 cases: no chain left out and none in the band in any case, all 32 boundary chains bound; worst
    error / bar 0.09 (x: N = 23, A = 3), 0.92 (dT/dx: N = 32, A = 3; 0.70 at N = 32, A = 1, 0.45 at N = 32, A = 33, at most 0.34
    elsewhere), 0.09 (T: N = 32, A = 3).  The high dT/dx ratios all belong to N = 32 (1,024 terms in every sum over the
    chain, added in another order than the restatement's) at few angles; why they come that close to the bar there has not been
    looked into."""
    model, theta, mask, meas, prior, starts = _case(N, A, M, seed)
    C, K = len(starts), N * N
    state = _init_state(N, theta, mask, meas, prior, starts, C)
    assert np.isnan(state[C]).all()                                    # the guard row
    assert not np.isnan(state[:C]).any()
    assert np.array_equal(state[:C, 2 * K - 1], np.full(C, np.float32(0.0123)))
    assert not state[:C, 2 * K].view(np.uint32).any()                  # the BITS of step index 0
    left, bound, band, worst = tw.check_target(model, starts, state[:C, :K - 1].copy(), state[:C, K - 1:2 * K - 2], state[:C, 2 * K - 2])
    print(f"N={N} A={A} M={M}: left out {left}, bound {bound}, in the band {band}, worst error / bar {worst}")
    assert left <= 2


def test_chunking_and_placement():
    """A run of w9 does not depend on how it is cut into launches, calls or groups of chains: array_equal throughout; no NaN is left in
    the (NaN-poisoned) outputs."""
    pb = wg.problem(_oracle(), "w9")
    kw = dict(form="workgroup", num_results=32, num_burnin_steps=16, num_adaptation_steps=24, step_size=wg.STEP, seed=3)
    one = _sample(pb, chains_per_object=100, **kw)
    assert not np.isnan(one[0]).any() and not any(np.isnan(v).any() for v in one[1].values())
    assert one[1]["is_accepted"].any() and not one[1]["is_accepted"].all()
    _same(one, _sample(pb, chains_per_object=100, steps_per_launch=4, **kw))       # 48 steps in launches of 4
    _same(one, _sample(pb, chains_per_object=100, **kw))                           # the same call twice
    part = _sample(pb, chains_per_object=10, first_chain=10, **kw)                 # chains 10..19 of the 100
    assert np.array_equal(one[0][:, 10:20], part[0])
    for k in ("log_accept_ratio", "is_accepted", "target_log_prob"):
        assert np.array_equal(one[1][k][:, 10:20], part[1][k]), k
    assert np.array_equal(one[1]["step_size"][10:20], part[1]["step_size"])
    _same(part, _sample(pb, chains_per_object=10, first_chain=10, chains_per_launch=3, **kw))      # launches of 3, 3, 3 and 1 chains
    # two objects in one call against two calls; launches of 3 chains then cut across the objects' 5
    rng = np.random.default_rng(7)
    meas2 = _oracle().poisson_measure(pb["meas"] * 0 + rng.uniform(0.05, 0.2, pb["meas"].shape).astype(np.float32), pb["mask"], 1e3, 6)
    both = dict(pb, meas=np.concatenate([pb["meas"], meas2]), mask=np.concatenate([pb["mask"], pb["mask"]]))
    two = _sample(both, chains_per_object=5, **kw)
    a, b = _sample(pb, chains_per_object=5, **kw), _sample(dict(pb, meas=meas2), chains_per_object=5, first_chain=5, **kw)
    assert np.array_equal(two[0], np.concatenate([a[0], b[0]], axis=1))
    for k in ("log_accept_ratio", "is_accepted", "target_log_prob"):
        assert np.array_equal(two[1][k], np.concatenate([a[1][k], b[1][k]], axis=1)), k
    assert np.array_equal(two[1]["step_size"], np.concatenate([a[1]["step_size"], b[1]["step_size"]]))
    assert not np.array_equal(a[0], b[0])
    _same(two, _sample(both, chains_per_object=5, chains_per_launch=3, **kw))


def test_step_size_adaptation_replays_on_the_host():
    """The final step_size at w12 equals, bit for bit, the host replay of the fp32 rule on the returned log_accept_ratio."""
    pb = wg.problem(_oracle(), "w12")
    _, tr = _sample(pb, form="workgroup", num_results=48, num_adaptation_steps=40, chains_per_object=wg.C, step_size=wg.STEP, seed=9,
                    initial_state=wg.random_starts("w12"))
    eps = np.full(wg.C, wg.STEP, np.float32)
    for s in range(40):
        eps = tw.adapt(eps, tr["log_accept_ratio"][s])
    assert np.array_equal(eps, tr["step_size"])
    assert len(np.unique(eps)) > 1


