"""The workgroup form of the HMC sampler (hmc_sample(form="workgroup"), csrc/hmc_wg.hip) without a GPU: that the restatement leaves
the GPU tests something to compare at their shapes, the argument checks of the call and of the entry points, and that the kernels
compile without scratch memory."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_hmc as tw
from tests import np_twin_hmc_wg as wg
from tests.conftest import ROOT

LDS = 160 * 1024


@pytest.mark.parametrize("name", list(wg.SHAPES))
def test_twin32_against_twin64_stays_under_the_caps(oracle, name):
    """The runs of tests/test_gpu_hmc_wg.py: float32 against float64 of the restatement alone leaves out at most 5 % of the 64 chains
    after one transition and 20 % after eight (the caps the GPU test applies to the device).  Seen: at worst 2 of 64 after one step and
    3 of 64 after eight; acceptance 0.68 .. 0.93, no NaN."""
    _, _, t32, t64 = wg.twin_runs(oracle, name, 8)
    assert not np.isnan(t32["samples"]).any() and not np.isnan(t64["lar"]).any()
    for n, cap in wg.CAPS.items():
        left = tw.check_against_twin(wg.first(t32, n), wg.first(t64, n))[0]
        print(f"{name} x {n}: left out {left:.4f}; acceptance {t64['acc'][:n].mean():.2f}")
        assert left <= cap


def test_the_evaluator_cases_are_the_issue_s():
    cases = list(wg.target_cases())
    assert len(cases) == 22
    assert [(N, A) for N, A, _, _ in cases] == [(9, 1), (9, 3), (9, 11), (9, 15), (12, 1), (12, 3), (12, 11), (12, 16), (12, 17), (16, 1),
                                                (16, 3), (16, 11), (16, 16), (16, 17), (23, 1), (23, 3), (23, 11), (23, 26), (32, 1),
                                                (32, 3), (32, 32), (32, 33)]
    assert {M for _, _, M, _ in cases} == {1, 2, 3, 4}


@pytest.mark.parametrize("N,A,M,seed", list(wg.target_cases()))
def test_the_evaluator_cases_leave_no_chain_out(oracle, N, A, M, seed):
    """np_twin_hmc.check_target at the restatement's own float32 x: no chain of the 64 is left out, none sits in the band around FLT_MIN
    (so whatever the device leaves out in tests/test_gpu_hmc_wg.py comes from its own x)."""
    model, _, _, _, _, starts = tw.target_case(oracle, N, A, M, seed)
    left, bound, band, _ = tw.check_target(model, starts, model.inverse(starts, np.float32))
    print(f"N={N} A={A} M={M}: left out {left}, bound {bound}, in the band {band}")
    assert left == 0 and band == 0


def test_hmc_sample_argument_errors_of_the_form():
    import ct_pvae_amd as cp
    from ct_pvae_amd._lib import RadonLibraryError
    ok = dict(num_results=4)
    wide = lambda A, N: (torch.zeros(A, N), torch.ones(A), np.zeros(A, np.float32), 1e3)   # noqa: E731
    with pytest.raises(ValueError, match="64 pixels"):                      # the default form keeps its limit
        cp.hmc_sample(*wide(2, 9), **ok)
    with pytest.raises(ValueError, match="64 pixels"):
        cp.hmc_sample(*wide(2, 9), form="wave", **ok)
    for bad in ("block", "", None, "Workgroup"):
        with pytest.raises(ValueError, match="form must be"):
            cp.hmc_sample(*wide(2, 2), form=bad, **ok)
    with pytest.raises(ValueError, match="32 x 32"):
        cp.hmc_sample(*wide(2, 33), form="workgroup", **ok)
    with pytest.raises(ValueError, match="2 x 2"):
        cp.hmc_sample(*wide(2, 1), form="workgroup", prior=(np.ones(1), np.ones((1, 1))), **ok)
    with pytest.raises(ValueError, match="256 angles"):
        cp.hmc_sample(*wide(257, 9), form="workgroup", prior=(np.ones(1), np.ones((1, 81))), **ok)
    with pytest.raises(ValueError, match=r"32 x 32 pixels at 47 angles need \d+ bytes of LDS"):          # before any launch: no device here
        cp.hmc_sample(*wide(47, 32), form="workgroup", prior=(np.ones(1), np.ones((1, 1024))), **ok)
    with pytest.raises(ValueError, match="steps_per_launch"):
        cp.hmc_sample(*wide(2, 9), form="workgroup", prior=(np.ones(1), np.ones((1, 81))), steps_per_launch=cp.mcmc.MAX_STEPS_PER_LAUNCH_WG + 1, **ok)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chains_per_launch"):
            cp.hmc_sample(*wide(2, 9), form="workgroup", prior=(np.ones(1), np.ones((1, 81))), chains_per_launch=bad, **ok)
    with pytest.raises(ValueError, match="chains_per_launch"):              # the wave form has no such cut
        cp.hmc_sample(*wide(2, 2), chains_per_launch=4, **ok)
    # a request that fits passes every check on the values and stops at the device
    with pytest.raises(RadonLibraryError, match="no CPU path"):
        cp.hmc_sample(*wide(46, 32), form="workgroup", prior=(np.ones(1), np.ones((1, 1024))), **ok)
    assert 8 <= cp.mcmc.MAX_STEPS_PER_LAUNCH_WG <= 512 and cp.mcmc.MAX_STEPS_PER_LAUNCH_WG & (cp.mcmc.MAX_STEPS_PER_LAUNCH_WG - 1) == 0
    assert "form" in cp.hmc_marginals.__doc__ and "workgroup" in cp.hmc_marginals.__doc__


def test_the_launches_of_the_workgroup_form_cover_the_chains():
    """_wg_pieces: every chain once, in order, at most cap per launch; a launch holds whole objects or chains of one object."""
    from ct_pvae_amd.mcmc import _wg_pieces
    for C, cpo, cap in ((10, 10, 3), (10, 5, 3), (12, 3, 7), (12, 3, 3), (8, 1, 3), (100, 100, 512), (6, 2, 4), (9, 3, 1), (64, 64, 64)):
        seen = []
        for c0, n, per, obj in _wg_pieces(C, cpo, cap):
            assert 1 <= n <= cap and n % per == 0 and obj == c0 // cpo
            assert per == cpo and c0 % cpo == 0 or (per == n and c0 // cpo == (c0 + n - 1) // cpo)
            seen += list(range(c0, c0 + n))
        assert seen == list(range(C)), (C, cpo, cap)
    assert list(_wg_pieces(100, 100, 512)) == [(0, 100, 100, 0)]


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from ct_pvae_amd import _lib
    lib = _lib.load()
    assert lib.ctpvae_hmc_wg_state_floats(4) == 9 and lib.ctpvae_hmc_wg_state_floats(1024) == 2049
    assert lib.ctpvae_hmc_wg_state_floats(3) == _lib.EINVAL and lib.ctpvae_hmc_wg_state_floats(1025) == _lib.EINVAL
    assert lib.ctpvae_hmc_state_floats(65) == _lib.EINVAL                  # the wave form's limits stay
    # the LDS request: an edge that fits and the next one, which does not
    assert 0 < lib.ctpvae_hmc_wg_lds_bytes(32, 46) <= LDS < lib.ctpvae_hmc_wg_lds_bytes(32, 47)
    assert 0 < lib.ctpvae_hmc_wg_lds_bytes(16, 168) <= LDS < lib.ctpvae_hmc_wg_lds_bytes(16, 169)
    assert lib.ctpvae_hmc_wg_lds_bytes(2, 2) < lib.ctpvae_hmc_wg_lds_bytes(3, 2) < lib.ctpvae_hmc_wg_lds_bytes(3, 3)
    for N, A in ((1, 2), (33, 2), (9, 0), (9, 257)):
        assert lib.ctpvae_hmc_wg_lds_bytes(N, A) == _lib.EINVAL, (N, A)
    # the admitted set holds every shape the tests run, 32 x 32 at 20 angles and 16 x 16 at 90
    shapes = list(wg.SHAPES.values()) + list(tw.SHAPES.values()) + [(N, A) for N, A, _, _ in wg.target_cases()] + [(32, 20), (16, 90)]
    assert all(0 < lib.ctpvae_hmc_wg_lds_bytes(N, A) <= LDS for N, A in shapes)

    null = [None] * 5
    assert lib.ctpvae_hmc_wg_run_f32(None, 1, 0, 1, 9, None, None, 2, None, None, 1e3, 1, None, None, None, 5, 8, 0, 0, 0, *null) == _lib.EINVAL
    assert "null" in _lib.last_error()
    assert lib.ctpvae_hmc_wg_init_f32(None, 1, 1, 9, None, None, 2, None, None, 1e3, 1, None, None, None, None, 1e-2, None) == _lib.EINVAL
    assert "null" in _lib.last_error()
    assert lib.ctpvae_hmc_wg_resident_chains(9, 2, None) == _lib.EINVAL
    keep = np.zeros(4096, np.float32)
    p = keep.ctypes.data
    out = ctypes.c_int(0)
    for bad in (dict(N=1), dict(N=33), dict(A=0), dict(A=257), dict(M=0), dict(M=5), dict(L=0), dict(L=33), dict(n=0), dict(n=513),
                dict(C=3, cpo=2), dict(C=0), dict(N=32, A=47), dict(N=23, A=87), dict(pnm=0.0)):
        a = dict(C=2, cpo=1, N=9, A=2, M=1, L=5, n=8, pnm=1e3)
        a.update(bad)
        rc = lib.ctpvae_hmc_wg_run_f32(p, a["C"], 0, a["cpo"], a["N"], p, p, a["A"], p, p, a["pnm"], a["M"], p, p, p, a["L"], a["n"], 0, 0, 0,
                                       p, p, p, p, None)
        assert rc == _lib.EINVAL, bad
        if "L" in bad or "n" in bad:
            continue
        rc = lib.ctpvae_hmc_wg_init_f32(p, a["C"], a["cpo"], a["N"], p, p, a["A"], p, p, a["pnm"], a["M"], p, p, p, None, 1e-2, None)
        assert rc == _lib.EINVAL, bad
        if set(bad) <= {"N", "A"}:
            assert lib.ctpvae_hmc_wg_resident_chains(a["N"], a["A"], ctypes.byref(out)) == _lib.EINVAL, bad
    assert lib.ctpvae_hmc_wg_init_f32(p, 2, 1, 9, p, p, 2, p, p, 1e3, 1, p, p, p, None, 0.0, None) == _lib.EINVAL      # the step size
    # the LDS refusal names N, A and the byte count
    need = lib.ctpvae_hmc_wg_lds_bytes(32, 47)
    assert lib.ctpvae_hmc_wg_run_f32(p, 2, 0, 1, 32, p, p, 47, p, p, 1e3, 1, p, p, p, 5, 8, 0, 0, 0, p, p, p, p, None) == _lib.EINVAL
    msg = _lib.last_error()
    assert "N=32" in msg and "A=47" in msg and str(need) in msg and "LDS" in msg
    # the wave entry points keep their limits
    assert lib.ctpvae_hmc_run_f32(p, 2, 0, 1, 9, p, p, 2, p, p, 1e3, 1, p, p, p, 5, 8, 0, 0, 0, p, p, p, p, None) == _lib.EINVAL


def test_hmc_wg_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "hmc_wg.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"Function Name: ", out.stderr)[1:]
    mine = [b for b in blocks if "hmc_wg_kernel" in b.split()[0]]
    assert len(mine) == 2
    for b in mine:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split()[0]
        assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) == 0, b.split()[0]      # no static LDS
        assert int(re.search(r" VGPRs: (\d+)", b).group(1)) <= 128, b.split()[0]                      # 1024 threads per workgroup
