"""The HMC sampler without a GPU: the numpy restatement (tests/np_twin_hmc.py) against torch.autograd and against an analytic
target, hmc_sample's argument checks, and that the kernels of csrc/hmc.hip compile without scratch memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_hmc as tw
from tests.conftest import ROOT


class _TapeProjector(torch.autograd.Function):
    """The nearest rotate-and-sum as TensorFlow's tape sees it: forward F, backward the tf_compat rule B (not F's transpose)."""

    @staticmethod
    def forward(ctx, O, F, B):
        ctx.save_for_backward(B)
        return O @ F.T

    @staticmethod
    def backward(ctx, g):
        (B,) = ctx.saved_tensors
        return g @ B.T, None, None


def _torch_target(model, x):
    """T(x) of csrc/hmc.hip's header from the issue's formulas, written with torch ops: sigmoid and a cumulative PRODUCT for the
    bijector (the twin and the kernel work in logs), logsumexp for the mixture, the textbook Poisson log-probability."""
    K = model.K
    f = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    z = torch.sigmoid(x - torch.log(torch.arange(K - 1, 0, -1, dtype=torch.float64)))
    ones = torch.ones((x.shape[0], 1), dtype=torch.float64)
    r = torch.cat([ones, torch.cumprod(1 - z, dim=1)], dim=1)
    O = torch.cat([z, ones], dim=1) * r
    fldj = (torch.log(z) + torch.log(1 - z) + torch.log(r[:, :-1])).sum(-1)
    Oc = torch.clamp_min(O, float(tw.TINY))
    comp = (f(model.alpha) - 1) @ torch.log(Oc).T                        # [M][C]
    prior = torch.logsumexp(f(model.logw)[:, None] + comp - f(model.lbeta)[:, None], dim=0)
    proj = _TapeProjector.apply(Oc, f(model.F), f(model.B)).reshape(-1, model.A, model.N)
    lam, k = proj * f(model.mask)[..., None] * float(model.pnm), f(model.meas) * float(model.pnm)
    lik = (torch.where(k == 0, torch.zeros_like(k), k * torch.log(torch.where(k == 0, torch.ones_like(lam), lam)))
           - torch.lgamma(k + 1) - lam).sum((1, 2))
    return prior + lik + fldj, O


@pytest.mark.parametrize("name", list(tw.SHAPES))
def test_twin_gradient_is_autograd_of_the_formulas(oracle, name):
    """Pins the bijector's derivation (J^T by a reverse scan, grad fldj = 1 - (K - j) z_j) and the softmax form of the prior's
    gradient: the float64 twin against torch.autograd, <= 1e-9 relative to the largest entry."""
    pb = tw.problem(oracle, name)
    C = 16
    model = tw.Model(oracle, pb["theta"], pb["N"], pb["mask"], pb["meas"], pb["pnm"], *pb["prior"], chains_per_object=C)
    x0 = model.inverse(tw.random_starts(name, C), np.float64) + np.random.default_rng(0).normal(0, 0.3, (C, model.K - 1))
    T, g, O = model.target(x0)
    x = torch.from_numpy(x0).requires_grad_(True)
    Tt, Ot = _torch_target(model, x)
    Tt.sum().backward()
    scale = max(1.0, float(np.abs(g).max()))
    assert np.abs(T - Tt.detach().numpy()).max() <= 1e-9 * max(1.0, float(np.abs(T).max()))
    assert np.abs(O - Ot.detach().numpy()).max() <= 1e-12
    assert np.abs(g - x.grad.numpy()).max() <= 1e-9 * scale, (np.abs(g - x.grad.numpy()).max(), scale)
    if name == "n3":      # tf_compat is not the transpose here: the test would not notice a twin that used F^T otherwise
        assert not np.array_equal(model.B, model.F.T)


def test_twin_gradient_is_autograd_of_the_formulas_where_the_clamp_binds(oracle):
    """The same pin (<= 1e-9 relative to the largest entry) at a bound point: interior starts of n4 with one pixel set to 1e-42,
    below FLT_MIN.  clamp_min passes no gradient there, and the twin's w of the bound pixel is exactly 0."""
    pb = tw.problem(oracle, "n4")
    C = 16
    model = tw.Model(oracle, pb["theta"], pb["N"], pb["mask"], pb["meas"], pb["pnm"], *pb["prior"], chains_per_object=C)
    starts = tw.random_starts("n4", C)
    pix = np.arange(C) % (model.K - 1)     # not the last pixel: the restatement's 1 - sigmoid(t) is 0 there, where the twin works in logs
    starts[np.arange(C), pix] = np.float32(1e-42)
    x0 = model.inverse(starts, np.float64)
    T, g, O, w = model.target(x0, with_w=True)
    bound = O < tw.TINY
    assert np.array_equal(np.argwhere(bound), np.stack([np.arange(C), pix], 1))
    assert np.all(w[bound] == 0.0) and np.all(w[~bound] != 0.0)
    x = torch.from_numpy(x0).requires_grad_(True)
    Tt, Ot = _torch_target(model, x)
    Ot.retain_grad()
    Tt.sum().backward()
    assert np.all(Ot.grad.numpy()[bound] == 0.0) and np.all(Ot.grad.numpy()[~bound] != 0.0)
    assert np.all(np.isfinite(g))
    scale = max(1.0, float(np.abs(g).max()))
    assert np.abs(T - Tt.detach().numpy()).max() <= 1e-9 * max(1.0, float(np.abs(T).max()))
    assert np.abs(g - x.grad.numpy()).max() <= 1e-9 * scale, (np.abs(g - x.grad.numpy()).max(), scale)


@pytest.mark.parametrize("N,A,M,seed", list(tw.target_cases()))
def test_the_evaluator_cases_leave_the_reference_something_to_compare(oracle, N, A, M, seed):
    """The conditions of tests/test_gpu_hmc_target.py for the restatement alone (float32 against float64 at the float32 inverse
    bijector of the starts): at most 20 % of the 64 chains left out, at least 16 compared chains with a bound pixel, no chain in
    the band around FLT_MIN where the clamp decision is ambiguous."""
    model, _, _, _, _, starts = tw.target_case(oracle, N, A, M, seed)
    left, bound, band, _ = tw.check_target(model, starts, model.inverse(starts, np.float32))
    print(f"N={N} A={A} M={M}: left out {left}, bound {bound}, in the band {band}")
    assert left <= 0.2 * len(starts) and bound >= 16 and band == 0


def test_twin_samples_an_analytic_target(oracle):
    """Likelihood off and one Dirichlet(2, 3, 4, 5): the twin's chain means and second moments match the analytic ones under the GPU
    test's rule (512 chains, 200 burn-in + 300 kept steps, within 5 sqrt(Var / 512))."""
    alpha = np.array([2.0, 3.0, 4.0, 5.0])
    C = 512
    model = tw.Model(oracle, np.array([0.0, np.pi / 2], np.float32), 2, np.zeros((1, 2)), np.zeros((1, 2, 2)), 1e3, np.ones(1), alpha[None],
                     chains_per_object=C)
    out = tw.run(model, np.zeros((C, 3)), np.full(C, 6.5e-2, np.float32), np.arange(C), 21, 500, 5, num_adaptation_steps=400)
    s = out["samples"][200:]
    a0 = alpha.sum()
    m1, m2 = alpha / a0, alpha * (alpha + 1) / (a0 * (a0 + 1))
    m4 = m2 * (alpha + 2) * (alpha + 3) / ((a0 + 2) * (a0 + 3))
    assert np.all(np.abs(s.mean((0, 1)) - m1) <= 5 * np.sqrt((m2 - m1 ** 2) / C))
    assert np.all(np.abs((s ** 2).mean((0, 1)) - m2) <= 5 * np.sqrt((m4 - m2 ** 2) / C))
    assert 0.5 < out["acc"].mean() <= 1.0 and len(np.unique(out["eps"])) > 1


@pytest.mark.parametrize("name", list(tw.SHAPES))
def test_twin32_against_twin64_stays_under_the_caps(oracle, name):
    """The seeds of tests/test_gpu_hmc.py: float32 against float64 of the restatement alone leaves out at most 5 % of 256 chains
    after one step and 20 % after twenty (the GPU tests apply the same caps to the device)."""
    _, _, t32, t64 = tw.twin_runs(oracle, name, 256, 20, tw.SEEDS[name])
    first = lambda d: {k: v[:1] for k, v in d.items() if k not in ("eps", "x")}   # noqa: E731
    assert tw.check_against_twin(first(t32), first(t64))[0] <= 0.05
    assert tw.check_against_twin(t32, t64)[0] <= 0.20


def test_twin32_against_twin64_at_the_extremes_stays_under_the_cap(oracle):
    """The seed of test_the_documented_extremes_against_the_twin: 64 chains, two transitions of 32 leapfrog steps, at most 5 % left out."""
    _, _, t32, t64 = tw.twin_runs(oracle, "max", 64, 2, tw.SEEDS["max"], L=tw.EXTREME_L)
    assert tw.check_against_twin(t32, t64)[0] <= 0.05


def test_hmc_sample_argument_errors():
    import ct_pvae_amd as cp
    from ct_pvae_amd._lib import RadonLibraryError
    ok = dict(num_results=4)
    meas, mask, th = torch.zeros(2, 2), torch.ones(2), [0.0, 1.5]
    with pytest.raises(ValueError, match="64 pixels"):
        cp.hmc_sample(torch.zeros(2, 9), mask, th, 1e3, **ok)
    with pytest.raises(ValueError, match="square"):
        cp.hmc_sample(torch.zeros(3, 2), mask, th, 1e3, **ok)              # three measured angles, two in theta
    with pytest.raises(ValueError, match="concentrations must be"):
        cp.hmc_sample(meas, mask, th, 1e3, prior=(np.ones(1), np.ones((1, 6))), **ok)      # a 2 x 3 object's prior
    with pytest.raises(ValueError, match="256 angles"):
        cp.hmc_sample(torch.zeros(257, 2), torch.ones(257), np.zeros(257), 1e3, **ok)
    with pytest.raises(ValueError, match="mixture of 1 .. 4"):
        cp.hmc_sample(meas, mask, th, 1e3, prior=(np.full(5, 0.2), np.ones((5, 4))), **ok)
    with pytest.raises(ValueError, match="positive"):
        cp.hmc_sample(meas, mask, th, 1e3, prior=(np.ones(1), np.array([[1.0, 0.0, 1.0, 1.0]])), **ok)
    for bad in ([0.5, 0.5, 0.0, 0.0], [0.5, 0.7, -0.1, -0.1], [0.5, 0.5, float("nan"), 0.0], [0.5, 0.5, float("inf"), 0.0]):
        with pytest.raises(ValueError, match="initial_state"):
            cp.hmc_sample(meas, mask, th, 1e3, initial_state=[bad], **ok)
    with pytest.raises(ValueError, match="chain id"):
        cp.hmc_sample(meas, mask, th, 1e3, first_chain=2 ** 32 - 2, chains_per_object=3, **ok)
    with pytest.raises(ValueError, match="steps_per_launch"):
        cp.hmc_sample(meas, mask, th, 1e3, steps_per_launch=10 ** 6, **ok)
    with pytest.raises(RadonLibraryError, match="no CPU path"):
        cp.hmc_sample(meas, mask, th, 1e3, **ok)
    w, a = cp.toy_dist()
    assert w.shape == (2,) and a.shape == (2, 4) and abs(float(w.sum()) - 1) < 1e-6


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from ct_pvae_amd import _lib
    lib = _lib.load()
    null = [None] * 5
    assert lib.ctpvae_hmc_state_floats(4) == 9 and lib.ctpvae_hmc_state_floats(64) == 129
    assert lib.ctpvae_hmc_state_floats(65) == _lib.EINVAL
    assert lib.ctpvae_hmc_run_f32(None, 1, 0, 1, 2, None, None, 2, None, None, 1e3, 1, None, None, None, 5, 10, 0, 0, 0, *null) == _lib.EINVAL
    assert "null" in _lib.last_error()
    buf = (np.zeros(4096, np.float32).ctypes.data,) * 3
    p = buf[0]
    for bad in (dict(N=9), dict(A=257), dict(M=5), dict(L=0), dict(n=10 ** 6), dict(C=3, cpo=2)):
        a = dict(C=2, cpo=1, N=2, A=2, M=1, L=5, n=8)
        a.update(bad)
        rc = lib.ctpvae_hmc_run_f32(p, a["C"], 0, a["cpo"], a["N"], p, p, a["A"], p, p, 1e3, a["M"], p, p, p, a["L"], a["n"], 0, 0, 0, p, p, p, p, None)
        assert rc == _lib.EINVAL, bad


def test_hmc_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "hmc.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert sum("hmc_kernel" in n for n in names) == 2 and len(scratch) == len(names)
    assert all(v == 0 for v in scratch), list(zip(names, scratch))
