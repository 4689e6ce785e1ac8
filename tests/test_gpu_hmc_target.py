"""The inner values of csrc/hmc.hip on the GPU: the chain state that ctpvae_hmc_init_f32 stores -- x (the inverse bijector of the
start), T(x) and dT/dx -- against the float64 restatement (tests/np_twin_hmc.py) at every object size, at the rounding ties of the
tap tables, with A N at and just above one pass of 64, and on starts where the clamp O' = max(O, FLT_MIN) binds; and the NaN rules
of the transition."""
import functools

import numpy as np
import pytest

from tests import np_twin_hmc as tw

pytestmark = pytest.mark.gpu
STEP = 0.0123


@functools.lru_cache(maxsize=None)
def _case(N, A, M, seed, C=64):
    from oracle import radon_oracle
    radon_oracle.build()
    return tw.target_case(radon_oracle, N, A, M, seed, C)


def _init_state(N, theta, mask, meas, prior, starts, C):
    """ctpvae_hmc_init_f32 on C chains of one object into a NaN-filled state of C + 1 rows (the last one a guard): the rows as numpy."""
    import torch

    from ct_pvae_amd import _lib, forward_functions
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    K, A = N * N, len(theta)
    T8, Tinv8 = forward_functions.rotate_tables(theta, N, N, dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    logw, alpha, lbeta = (up(a) for a in tw.prior_tables(*prior))
    assert alpha.shape == (len(logw), K)
    mask_d, meas_d = up(mask), up(meas)
    assert mask_d.shape == (1, A) and meas_d.shape == (1, A, N)
    start = None if starts is None else up(starts)
    assert start is None or start.shape == (C, K)
    state = torch.full((C + 1, 2 * K + 1), float("nan"), dtype=torch.float32, device=dev)
    assert lib.ctpvae_hmc_state_floats(K) == state.shape[1]
    with torch.cuda.device(dev):
        _lib.check(lib.ctpvae_hmc_init_f32(state.data_ptr(), C, C, N, T8.data_ptr(), Tinv8.data_ptr(), A, mask_d.data_ptr(), meas_d.data_ptr(),
                                           float(tw.TARGET_PNM), len(logw), logw.data_ptr(), alpha.data_ptr(), lbeta.data_ptr(),
                                           None if start is None else start.data_ptr(), STEP, forward_functions._stream_ptr()), "hmc_init")
        torch.cuda.synchronize()
    return state.cpu().numpy()


def _check_state(state, model, starts, C):
    K = model.K
    assert np.isnan(state[C]).all()                                    # the guard row
    assert not np.isnan(state[:C]).any()
    assert np.array_equal(state[:C, 2 * K - 1], np.full(C, np.float32(STEP)))
    assert not state[:C, 2 * K].view(np.uint32).any()                  # the BITS of step index 0
    return tw.check_target(model, starts, state[:C, :K - 1].copy(), state[:C, K - 1:2 * K - 2], state[:C, 2 * K - 2])


@pytest.mark.parametrize("N,A,M,seed", list(tw.target_cases()))
def test_the_evaluator_against_the_twin(N, A, M, seed):
    """64 chains per case, 32 of them started with one denormal pixel: x, dT/dx and T of the stored state against the float64 twin
    AT THE DEVICE'S OWN x, per chain, within max(1e-5 scale, 8 |twin32 - twin64|) (np_twin_hmc.check_target); the step size, the
    step index and the guard row after the state.  At most 20 % of the chains left out, at least 16 compared with a bound pixel.
    Seen on the MI355X over the 28 cases: worst error / bar 0.09 (x), 0.16 (dT/dx), 0.05 (T); left out 10 of 64 at N = 2, A = 11 and
    5 of 64 at N = 2, A = 32 (their T is still compared), none elsewhere; all 32 boundary chains bound in every case, none in the
    band; x of a denormal start is finite (the device's logf takes denormals), so the device differs from the twin nowhere in kind.
    Wrong kernels, tried on a scratch copy: without row_bcast:31 every case of N = 6, 7, 8 fails (x, by 1.2 to 3.6) and none of
    N <= 5, whose lanes end in row 1; `a * q.N + b` for the 255 sentinel fails 10 cases (N = 4: A = 3, 11, 16; N = 5: A = 11, 13;
    N = 6: A = 11; N = 7: A = 10, 11; N = 8: A = 8, 11; dT/dx, or NaN left in the state); rintf for roundf fails N = 2 at A = 11
    and 32 and N = 6 at A = 11 (dT/dx); `sp.O` for `bind ? FLT_MIN : sp.O` fails N = 2 at A = 11 and 32, through T on the chains
    whose gradient is left out and through nothing else (T off by 5e3): a bound pixel's value shows only on a ray with no other tap."""
    model, theta, mask, meas, prior, starts = _case(N, A, M, seed)
    C = len(starts)
    state = _init_state(N, theta, mask, meas, prior, starts, C)
    left, bound, band, worst = _check_state(state, model, starts, C)
    print(f"N={N} A={A} M={M}: left out {left}, bound {bound}, worst error / bar {worst}")
    assert left <= 0.2 * C and bound >= 16 and band == 0


@pytest.mark.parametrize("N", [4, 7])
def test_the_default_start_is_the_origin(N):
    """start = nullptr: x is exactly 0 and T, dT/dx are those of the twin at 0, under the evaluator's rule.
    Seen on the MI355X: worst error / bar 0.04 (dT/dx), 0.01 (T)."""
    A = -(-64 // N)
    C = 4
    model, theta, mask, meas, prior, _ = _case(N, A, 1 + (N + A) % 4, 100 * N + A, C)   # the evaluator case's problem
    state = _init_state(N, theta, mask, meas, prior, None, C)
    assert not state[:C, :N * N - 1].view(np.uint32).any()
    left, _, _, worst = _check_state(state, model, None, C)
    print(f"N={N}: worst error / bar {worst}")
    assert left == 0
    assert np.array_equal(state[:C], np.tile(state[:1], (C, 1)))


def test_a_nan_target_rejects_and_shrinks_the_step():
    """The header's NaN rules.  Two objects in one call, the second with a NaN measurement: its chains never accept (every sample is
    the start, bit for bit), their log_accept_ratio and target_log_prob are NaN, and their step size is eps / 1.01f ten times; the
    first object's chains are those of a call without the second, array for array."""
    import torch

    import ct_pvae_amd as cp
    from oracle import radon_oracle
    radon_oracle.build()
    dev = torch.device("cuda", 0)
    pb, pb2 = tw.problem(radon_oracle, "n3"), tw.problem(radon_oracle, "n3", seed=1)
    meas = np.concatenate([pb["meas"], pb2["meas"]])
    meas[1, 0, 0] = np.nan
    mask = np.concatenate([pb["mask"], pb2["mask"]])
    assert mask[1, 0] > 0
    cpo = 8
    starts = tw.random_starts("n3", 2 * cpo)
    kw = dict(prior=pb["prior"], chains_per_object=cpo, num_results=24, num_adaptation_steps=10, seed=4, step_size=tw.STEP["n3"])
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    s2, t2 = cp.hmc_sample(up(meas), up(mask), pb["theta"], pb["pnm"], initial_state=starts, **kw)
    s1, t1 = cp.hmc_sample(up(meas[:1]), up(mask[:1]), pb["theta"], pb["pnm"], initial_state=starts[:cpo], **kw)
    torch.cuda.synchronize()
    # the healthy object does not see its neighbour
    assert torch.equal(s2[:, :cpo], s1) and not torch.isnan(s1).any()
    for k in ("log_accept_ratio", "is_accepted", "target_log_prob"):
        assert torch.equal(t2[k][:, :cpo], t1[k]), k
    assert torch.equal(t2["step_size"][:cpo], t1["step_size"])
    assert t1["is_accepted"].any()
    # the poisoned one
    smp = s2[:, cpo:].cpu().numpy()
    assert not t2["is_accepted"][:, cpo:].any()
    assert np.array_equal(smp.view(np.uint32), np.tile(smp[:1], (len(smp), 1, 1)).view(np.uint32))
    assert np.abs(smp[0].astype(np.float64) - starts[cpo:]).max() <= 1e-6
    assert torch.isnan(t2["log_accept_ratio"][:, cpo:]).all() and torch.isnan(t2["target_log_prob"][:, cpo:]).all()
    eps = np.full(cpo, tw.STEP["n3"], np.float32)
    for _ in range(10):
        eps = tw.adapt(eps, np.full(cpo, np.nan, np.float32))
    assert np.array_equal(eps, t2["step_size"][cpo:].cpu().numpy()) and np.all(eps < np.float32(tw.STEP["n3"]))
