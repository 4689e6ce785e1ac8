"""Host side of the fused Normal latent block (ct_pvae_amd/latents.py, csrc/latent.hip): the generator's layout and law, the
acceptance rule of tests/np_twin_latent.py (the float32 twin stays under the cap; the bar bites), the argument checks and the
trainer's flag.  The kernels themselves: tests/test_gpu_latent.py."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_latent as tl
from tests.conftest import ROOT

SEED = 0x1234567887654321


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


@pytest.fixture(scope="module", params=list(tl.RANGES))
def twin_case(request):
    return tl.case(request.param, 4, 4096, 2, 11, draw=3, level=1)


def test_float32_twin_stays_under_the_cap(twin_case):
    """The project's rule: the float32 composition is within R * bar of float64 per sample, R <= R_MAX -- the twin cannot quietly
    widen the bar the kernels are held to."""
    for k, R in twin_case["R"].items():
        print(k, R)
        assert 1.0 <= R <= tl.R_MAX, (k, R)


def test_kernel_expressions_obey_the_rule_in_numpy(twin_case):
    """csrc/latent.hip's own expressions (the closed-form backward, the sums over s ascending) restated in numpy float32 are within
    4 R bar of the float64 composition's values and AUTOGRAD gradients on every sample: the kernels' algebra, checked without a GPU."""
    c = twin_case
    got = tl.kernel_form(c["loc"], c["log_scale"], c["eps32"], c["g_z"], c["g_KL"])
    for k in ("z", "kl", "g_loc", "g_log_scale"):
        worst = float(np.max(tl.excess(got[k], c["want"][k], c["bar"][k])))
        print(k, worst, c["R"][k])
        assert worst <= tl.MARGIN * c["R"][k], (k, worst)


def test_the_bar_bites(twin_case):
    """Planted defects land outside 4 R bar: a float32 twin whose KL lacks -log(scale) (kl and g_log_scale, more than 1 % of the
    samples), a backward that forgets pr' (most samples below log_scale = 1) and a draw of the wrong sign."""
    c = twin_case
    d = tl.compose(c["loc"], c["log_scale"], c["eps32"], c["sqrt_reg"], c["ns"], torch.float32)
    d["kl"] = 0.5 * (d["scale"] * d["scale"] + d["loc"] * d["loc"] - 1.0)
    got = dict(zip(("g_loc", "g_log_scale"), tl.gradients(d, c["g_z"], c["g_KL"])), kl=tl.values(d)["kl"])
    for k in ("kl", "g_log_scale"):
        outside = float((tl.excess(got[k], c["want"][k], c["bar"][k]) > tl.MARGIN * c["R"][k]).mean())
        print("no log(scale)", k, outside)
        assert outside > 0.01, (k, outside)
    below = c["log_scale"] < 1
    wrong = c["want"]["g_log_scale"] / np.where(below, np.exp(c["log_scale"].astype(np.float64) - 1), 1.0)
    outside = float((tl.excess(wrong, c["want"]["g_log_scale"], c["bar"]["g_log_scale"]) > tl.MARGIN * c["R"]["g_log_scale"])[below].mean())
    print("no pr'", outside)
    assert outside > 0.5, outside
    flipped = tl.excess(-c["want"]["eps"], c["want"]["eps"], c["bar"]["eps"]) > tl.MARGIN * c["R"]["eps"]
    assert float(flipped.mean()) > 0.99


@pytest.mark.parametrize("length", [35, 99])
@pytest.mark.parametrize("first_object", [0, 3, 1000003, 2 ** 34 // 35 - 1])
def test_host_draws_are_the_numpy_philox_bit_for_bit(lib, length, first_object):
    """length = 35 and 99 are no multiples of 4 (objects start mid-block); the last first_object makes the flat index cross
    2^32 * 4 at length 35, where the block index spills into the second counter word."""
    from ct_pvae_amd import latent_draws
    n, ns, draw, level = 3, 3, 7, 2
    if first_object > 2 ** 30 and length == 35:
        assert first_object * length < 2 ** 34 < (first_object + n) * length
    got = latent_draws(n, length, ns=ns, seed=SEED, draw=draw, level=level, first_object=first_object)
    want = tl.draws(n, length, ns, SEED, draw, level, first_object)
    assert got.dtype == np.float32 and got.shape == (ns, n, length)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.abs(got) >= 2.0 ** -26).all() and (np.abs(got) <= 0.5).all()
    # equal keys give equal draws; the level, the sample, the draw and the seed each key the stream
    assert np.array_equal(got, latent_draws(n, length, ns=ns, seed=SEED, draw=draw, level=level, first_object=first_object))
    assert not np.array_equal(got, latent_draws(n, length, ns=ns, seed=SEED, draw=draw + 1, level=level, first_object=first_object))
    assert not np.array_equal(got, latent_draws(n, length, ns=ns, seed=SEED, draw=draw, level=level + 1, first_object=first_object))
    assert not np.array_equal(got, latent_draws(n, length, ns=ns, seed=SEED + 1, draw=draw, level=level, first_object=first_object))
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    # a split batch draws what the whole batch draws, for any ns: sample s does not depend on how many samples there are
    assert np.array_equal(got[:, 1:], latent_draws(n - 1, length, ns=ns, seed=SEED, draw=draw, level=level, first_object=first_object + 1))
    assert np.array_equal(got[:2], latent_draws(n, length, ns=2, seed=SEED, draw=draw, level=level, first_object=first_object))


def test_tail_probability_at_the_ends_of_the_word():
    """k = 0 gives t = 2^-26, k = 2^24 - 1 gives exactly 0.5 (k + 0.5 rounds to 2^24): never 0, so the quantile is finite; bit 31 is
    the sign; bits 0 .. 6 are unused."""
    w = np.array([0, 0x7F, 0x80, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x7FFFFF80], np.uint32)
    v = tl.tail(w)
    assert v.tolist() == [2.0 ** -26, 2.0 ** -26, 3 * 2.0 ** -26, 0.5, -2.0 ** -26, -0.5, 0.5]
    e = tl.eps_of(v)
    assert np.isfinite(e).all() and abs(e[0]) < 5.6 and e[0] > 0 and e[4] == -e[0] and e[3] == 0


def test_latent_tag_differs_from_the_other_streams():
    """The fourth counter word: 0x4C in the top byte, whatever level and s are, against the head's, hmc's and poisson's words."""
    from tests import np_twin_head, np_twin_hmc
    for other in (np_twin_head.TAG, np_twin_hmc.TAG, 0):
        assert other >> 24 != tl.TAG >> 24
    src = open(os.path.join(ROOT, "ct_pvae_amd", "csrc", "latent.hip")).read()
    assert re.search(r"kLatentTag\s*=\s*0x%Xu" % tl.TAG, src)


def test_draws_follow_the_standard_normal_law(lib):
    """2 * 10^5 draws of a fixed seed: the mean, the variance and P(|eps| > 2) each within 5 standard errors of N(0, 1); all finite,
    |eps| <= 5.6."""
    from ct_pvae_amd import latent_draws
    n = 200000
    eps = tl.eps_of(latent_draws(4, n // 8, ns=2, seed=20240521, draw=0, level=0)).ravel()
    assert eps.size == n and np.isfinite(eps).all() and np.abs(eps).max() <= 5.6
    p2 = math.erfc(2 / math.sqrt(2))
    stats = {"mean": (eps.mean(), 0.0, 1 / math.sqrt(n)), "variance": (eps.var(), 1.0, math.sqrt(2 / n)),
             "P(|eps| > 2)": ((np.abs(eps) > 2).mean(), p2, math.sqrt(p2 * (1 - p2) / n))}
    for k, (got, want, se) in stats.items():
        print(f"{k}: {got:.6f} vs {want:.6f}, {abs(got - want) / se:.2f} standard errors")
        assert abs(got - want) <= 5 * se, k


def test_bad_arguments_are_einval_before_any_hip_call(lib):
    L = lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # (host pointers: every call below is refused before the pointer is used or a HIP call is made)
    #         skip B  len ns reg  fo seed draw level eps z  kl kl_elem eps_out stream
    good_f = [p, 2, 8, 2, 1e-7, 0, 1, 0, 0, None, p, p, None, None, None]
    for i in (0, 10, 11):
        bad = list(good_f)
        bad[i] = None
        assert L.ctpvae_latent_fwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((1, 0), (1, -1), (2, 0), (3, 0), (3, 65536), (5, -1), (5, 2 ** 63 - 1), (8, 256)):
        bad = list(good_f)
        bad[i] = v
        assert L.ctpvae_latent_fwd_f32(*bad) == lib.EINVAL, (i, v)
    bad = list(good_f)
    bad[1:4] = [2 ** 15, 2 ** 15, 2]                                                       # ns * B * len = 2^31
    assert L.ctpvae_latent_fwd_f32(*bad) == lib.EINVAL and "31 bits" in lib.last_error()
    #         skip B  len ns reg  fo seed draw level eps g_z g_kl g_skip stream
    good_b = [p, 2, 8, 2, 1e-7, 0, 1, 0, 0, None, p, p, p, None]
    for i in (0, 12):
        bad = list(good_b)
        bad[i] = None
        assert L.ctpvae_latent_bwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((1, 0), (2, -3), (3, 0), (3, 65536), (5, -1), (8, 256)):
        bad = list(good_b)
        bad[i] = v
        assert L.ctpvae_latent_bwd_f32(*bad) == lib.EINVAL, (i, v)
    assert L.ctpvae_latent_draws_host_f32(2, 8, 2, 0, 1, 0, 0, None) == lib.EINVAL and "null" in lib.last_error()
    for n, length, ns, fo, level in ((0, 8, 2, 0, 0), (2, 0, 2, 0, 0), (2, 8, 0, 0, 0), (2, 8, 65536, 0, 0), (2, 8, 2, -1, 0),
                                     (2, 8, 2, 2 ** 63 - 1, 0), (2, 8, 2, 0, 256), (2 ** 15, 2 ** 15, 2, 0, 0)):
        assert L.ctpvae_latent_draws_host_f32(n, length, ns, fo, 1, 0, level, p) == lib.EINVAL, (n, length, ns, fo, level)
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL, "latent")


def test_python_wrapper_refuses_what_it_cannot_run(lib):
    from ct_pvae_amd import latent_draws, normal_latents
    a = torch.zeros(2, 4, 5, 7)
    kw = dict(ns=2, seed=0, draw=0, level=0)
    with pytest.raises(TypeError):
        normal_latents(a.numpy(), **kw)
    with pytest.raises(TypeError):
        normal_latents(a.double(), **kw)
    with pytest.raises(ValueError):
        normal_latents(a[:, 0], **kw)                                        # not [B][2C][H][W]
    with pytest.raises(ValueError):
        normal_latents(torch.zeros(2, 3, 5, 7), **kw)                        # odd channel count
    with pytest.raises(ValueError):
        normal_latents(torch.zeros(2, 8, 5, 7)[:, :4], **kw)                 # a channel half: not contiguous
    for bad in (dict(ns=0), dict(ns=65536), dict(level=-1), dict(level=256), dict(draw=2 ** 32), dict(draw=-1)):
        with pytest.raises(ValueError):
            normal_latents(a, **dict(kw, **bad))
    with pytest.raises(ValueError):
        normal_latents(a, first_object=-1, **kw)
    with pytest.raises(ValueError):
        normal_latents(a, _eps=torch.zeros(2, 2, 5, 7), **kw)                # _eps must be [ns * B][C][H][W]
    with pytest.raises(lib.RadonLibraryError):
        normal_latents(a, **kw)                                              # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        latent_draws(0, 5, **kw)
    with pytest.raises(ValueError):
        latent_draws(2, 5, ns=2, seed=0, draw=0, level=256)


def test_fused_latents_argument_rules():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args(["--normal"]).fused_latents is False                              # off by default
    a = tr.get_args("--normal --fused_latents".split())
    assert a.fused_latents is True and a.fused_head is False and a.head_seed == 1234
    assert tr.get_args("--normal --fused_head --fused_latents".split()).fused_head is True
    with pytest.raises(ValueError):
        tr.get_args(["--fused_latents"])                                                 # the Beta latents are not fused
    with pytest.raises(ValueError):
        tr.get_args("--normal --det --fused_latents".split())
    for bad in (dict(use_normal=False), dict(use_normal=True, deterministic=True)):
        with pytest.raises(ValueError):
            tr.find_loss_vae_unsup(None, None, None, None, None, 1.0, 1e-7, 1.0, 1.0, fused_latents=(0, 0, 0), **bad)
    # the constructor checks again (arguments built without get_args), before it touches the device
    for flags in ("--nsa 20 --td 6 -b 3", "--nsa 20 --td 6 -b 3 --normal --det"):
        args = tr.get_args(flags.split())
        args.fused_latents = True
        with pytest.raises(ValueError):
            tr.PVAETrainer(args, torch.device("cpu"))
