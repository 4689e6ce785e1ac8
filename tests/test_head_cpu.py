"""Host side of the fused TruncatedNormal output head (ct_pvae_amd/output_head.py, csrc/head.hip): the generator's layout, the
acceptance rule of tests/np_twin_head.py (the float32 twin stays under the cap; the bar bites), the argument checks, the
compiler's resource report and the trainer's flag.  The kernels themselves: tests/test_gpu_head.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_head as th
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


@pytest.fixture(scope="module", params=list(th.RANGES))
def twin_case(request):
    return th.case(request.param, 8, 4096, 11)


@pytest.mark.parametrize("first_object", [0, 3, 1000003, 2 ** 34 // 35 - 1])
def test_host_uniforms_are_the_numpy_philox_bit_for_bit(lib, first_object):
    """pix = 35 is no multiple of 4 (objects start mid-block); the last first_object makes the flat index cross 2^32 * 4, where the
    block index spills into the second counter word."""
    from ct_pvae_amd import head_uniforms
    n, pix, seed, draw = 3, 35, 0x1234567887654321, 7
    if first_object > 2 ** 30:
        assert first_object * pix < 2 ** 34 < (first_object + n) * pix
    got = head_uniforms(n, pix, seed=seed, draw=draw, first_object=first_object)
    want = th.uniforms(n, pix, seed, draw, first_object)
    assert got.dtype == np.float32 and got.shape == (n, pix)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got > 0).all() and (got < 1).all()
    # the draw and the seed key the stream; a split batch draws what the whole batch draws
    assert not np.array_equal(got, head_uniforms(n, pix, seed=seed, draw=draw + 1, first_object=first_object))
    assert not np.array_equal(got, head_uniforms(n, pix, seed=seed + 1, draw=draw, first_object=first_object))
    assert np.array_equal(got[1:], head_uniforms(n - 1, pix, seed=seed, draw=draw, first_object=first_object + 1))


def test_head_tag_differs_from_the_other_streams():
    from tests import np_twin_hmc
    assert th.TAG not in (np_twin_hmc.TAG, 0)
    src = open(os.path.join(ROOT, "ct_pvae_amd", "csrc", "head.hip")).read()
    assert re.search(r"kHeadTag\s*=\s*0x%Xu" % th.TAG, src)


def test_float32_twin_stays_under_the_cap(twin_case):
    """The project's rule: the float32 composition is within R * bar of float64 per sample, R <= R_MAX -- the twin cannot quietly
    widen the bar the kernels are held to.  On these ranges no clamp acts, so no sample is left out."""
    assert int(twin_case["skip"].sum()) == 0
    for k, R in twin_case["R"].items():
        print(k, R)
        assert 1.0 <= R <= th.R_MAX, (k, R)


def test_kernel_expressions_obey_the_rule_in_numpy(twin_case):
    """csrc/head.hip's own expressions (two erfc, the complement's quantile, the closed-form backward) restated in numpy float32 are
    within 4 R bar of the float64 composition's values and AUTOGRAD gradients on every sample: the kernels' algebra, checked
    without a GPU."""
    c = twin_case
    got = th.kernel_form(c["alpha"], c["beta"], c["u"], c["g_x"], c["g_LP"])
    for k in ("x", "lp", "g_alpha", "g_beta"):
        worst = float(np.max(th.excess(got[k], c["want"][k], c["bar"][k])))
        print(k, worst, c["R"][k])
        assert worst <= th.MARGIN * c["R"][k], (k, worst)


def test_kernel_expressions_at_the_clamps_of_p():
    """The injected-u case of tests/test_gpu_head.py on the numpy restatement: both clamps of p are reached, values and gradients obey
    the bar, and where p is clamped nothing but g_x reaches alpha (g_LP = 0, pr' = 1), exactly."""
    import math
    n, pix = 2, 64
    u = np.tile(np.array([2.0 ** -25, 0.5, 1.0, 1 - 2.0 ** -24], np.float32), (n, pix // 4))
    for av, bv, clamped in ((2.75, 1 + math.log(0.5), (0, 2, 3)), (1.0, 1000.0, (2, 3))):
        alpha, beta = np.full((n, pix), av, np.float32), np.full((n, pix), bv, np.float32)
        c = th.case(None, n, pix, 5, u=u, operands_=(alpha, beta), skip_p=False)
        got = th.kernel_form(alpha, beta, u, c["g_x"], c["g_LP"])
        for k in ("x", "lp", "g_alpha", "g_beta"):
            keep = ~c["skip"] if k.startswith("g_") else np.ones_like(c["skip"])
            assert float(np.max(th.excess(got[k], c["want"][k], c["bar"][k])[keep])) <= th.MARGIN * c["R"][k], k
        ga0 = th.kernel_form(alpha, beta, u, c["g_x"], np.zeros(n, np.float32))["g_alpha"]
        cols = np.zeros((n, pix), bool)
        cols[:, [j for j in range(pix) if j % 4 in clamped]] = True
        cols &= ~c["skip"]
        assert cols.any() and np.array_equal(ga0[cols], c["g_x"][cols])


@pytest.mark.parametrize("defect,quantities", [("no_log_z", ("lp", "g_alpha", "g_beta")), ("unit_slope", ("g_alpha", "g_beta"))])
def test_the_bar_bites(twin_case, defect, quantities):
    """A float32 twin with one planted defect puts more than 1 % of the samples outside 4 R bar."""
    c = twin_case
    d = th.compose(c["alpha"], c["beta"], c["u"], torch.float32, defect=defect)
    got = dict(zip(("g_alpha", "g_beta"), th.gradients(d, c["g_x"], c["g_LP"])), lp=d["lp"].detach().numpy())
    for k in quantities:
        outside = float((th.excess(got[k], c["want"][k], c["bar"][k]) > th.MARGIN * c["R"][k]).mean())
        print(defect, k, outside)
        assert outside > 0.01, (defect, k, outside)


def test_bad_arguments_are_einval_before_any_hip_call(lib):
    L = lib.load()
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data
    # (host pointers: every call below is refused before the pointer is used or a HIP call is made)
    good_f = [p, p, 2, 8, 0, 1, 0, None, p, p, None, None]
    assert L.ctpvae_tn_head_fwd_f32(None, p, 2, 8, 0, 1, 0, None, p, p, None, None) == lib.EINVAL and "null" in lib.last_error()
    for i in (1, 8, 9):
        bad = list(good_f)
        bad[i] = None
        assert L.ctpvae_tn_head_fwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((2, 0), (2, -1), (3, 0), (4, -1), (4, 2 ** 63 - 1)):
        bad = list(good_f)
        bad[i] = v
        assert L.ctpvae_tn_head_fwd_f32(*bad) == lib.EINVAL
    assert L.ctpvae_tn_head_fwd_f32(p, p, 2 ** 16, 2 ** 15, 0, 1, 0, None, p, p, None, None) == lib.EINVAL     # n * pix = 2^31
    good_b = [p, p, 2, 8, 0, 1, 0, None, p, p, p, p, None]
    for i in (0, 1, 10, 11):
        bad = list(good_b)
        bad[i] = None
        assert L.ctpvae_tn_head_bwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((2, 0), (3, -3), (4, -1)):
        bad = list(good_b)
        bad[i] = v
        assert L.ctpvae_tn_head_bwd_f32(*bad) == lib.EINVAL
    assert L.ctpvae_tn_head_uniforms_host_f32(2, 8, 0, 1, 0, None) == lib.EINVAL and "null" in lib.last_error()
    for n, pix, fo in ((0, 8, 0), (2, 0, 0), (2, 8, -1), (2, 8, 2 ** 63 - 1)):
        assert L.ctpvae_tn_head_uniforms_host_f32(n, pix, fo, 1, 0, p) == lib.EINVAL
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL, "tn_head")
    assert ctypes.sizeof(ctypes.c_longlong) == 8


def test_python_wrapper_refuses_what_it_cannot_run(lib):
    from ct_pvae_amd import head_uniforms, truncated_normal_head
    a = torch.zeros(2, 1, 5, 7)
    with pytest.raises(TypeError):
        truncated_normal_head(a.numpy(), a, seed=0, draw=0)
    with pytest.raises(TypeError):
        truncated_normal_head(a.double(), a.double(), seed=0, draw=0)
    with pytest.raises(ValueError):
        truncated_normal_head(a[:, 0], a[:, 0], seed=0, draw=0)                       # not [n][1][X][Y]
    with pytest.raises(ValueError):
        truncated_normal_head(torch.zeros(2, 2, 5, 7)[:, :1], a, seed=0, draw=0)      # a channel half: not contiguous
    with pytest.raises(ValueError):
        truncated_normal_head(a, torch.zeros(2, 1, 7, 5), seed=0, draw=0)
    with pytest.raises(ValueError):
        truncated_normal_head(a, a, seed=0, draw=2 ** 32)
    with pytest.raises(ValueError):
        truncated_normal_head(a, a, seed=0, draw=0, first_object=-1)
    with pytest.raises(lib.RadonLibraryError):
        truncated_normal_head(a, a, seed=0, draw=0)                                   # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        head_uniforms(0, 5, seed=0, draw=0)


def test_head_kernels_use_no_scratch():
    """hipcc's own resource report for csrc/head.hip with the library's flags: no kernel spills registers."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "head.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    name, scratch = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
    assert any("tn_head_fwd_kernel" in k for k in scratch) and any("tn_head_bwd_kernel" in k for k in scratch), scratch
    assert all(v == 0 for v in scratch.values()), scratch


def test_fused_head_argument_rules():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args(["--normal"]).fused_head is False                               # off by default
    a = tr.get_args("--normal --fused_head".split())
    assert a.fused_head is True and a.head_seed == 1234
    assert tr.get_args("--normal --fused_head --head_seed 5".split()).head_seed == 5
    assert a.reproducible is False and tr.get_args("--normal --fused_head --reproducible".split()).reproducible is True
    with pytest.raises(ValueError):
        tr.get_args(["--fused_head"])                                                  # the Beta head is not fused
    with pytest.raises(ValueError):
        tr.find_loss_vae_unsup(None, None, None, None, None, 1.0, 1e-7, 1.0, 1.0, use_normal=False, fused_head=(0, 0, 0))
