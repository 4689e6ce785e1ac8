"""Host side of the fused Beta latent block (ct_pvae_amd/beta_latents.py, csrc/beta_latent.hip): the layout of the counter word, the
KL twin against torch's float64 kl_divergence, its closed-form gradient against float64 autograd, the trigamma restatement, the
acceptance rule of tests/np_twin_beta_latent.py (the float32 twin stays under the cap), the argument checks, the trainer's flag and
the kernels' register report.  The kernels themselves: tests/test_gpu_beta_latent.py.

Measured here (the figures the tests print; none of them sets a bound): KL twin against torch float64, worst relative 2.8e-13
(bound 1e-12); closed-form gradient against float64 autograd where the comparison is well-posed, worst relative 2.2e-7 (bound 1e-6;
over ALL samples 6.3e-6, which is torch's float64 trigamma, see the test); trigamma against scipy's polygamma, worst relative 1.05e-15
(bound 1e-14); the restated lgamma / digamma of the kernel within 0.23 / 0.29 of their counted rounding bounds; the float32 twin's
R is 1.0 for every quantity on all four ranges."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy import special

from tests import np_twin_beta as tb
from tests import np_twin_beta_latent as tbl
from tests import np_twin_hmc
from tests.conftest import ROOT

F, D = np.float32, np.float64
SEED = 0x1234567887654321
LEVELS, SAMPLES, GAMMAS, ATTEMPTS = (0, 255), (0, 1, 31, 32, 2047), (0, 1), (0, 15)


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def _numpy_words(n, length, fo, draw, level, s, gamma, attempt):
    e = (np.uint64(fo) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(length) + np.arange(length, dtype=np.uint64)[None, :]
    word = 0x51000000 | level << 16 | s << 5 | gamma << 4 | attempt
    return np_twin_hmc.philox(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), np.uint64(draw), np.uint64(word), SEED)


def test_words_are_the_numpy_philox_at_every_corner_of_the_counter_word(lib):
    """beta_latent_words against the numpy Philox with the word written out here, at the corners of (level, s, gamma, attempt), and with
    first_object * len beyond 2^32 so that hi32(e) is not 0; the twin's words() is the same array."""
    from ct_pvae_amd import beta_latent_words
    n, length, draw = 2, 7, 9
    for fo in (0, 3, (2 ** 32) // 7 - 1, 5 * 2 ** 32):                   # the third: e crosses 2^32 inside the call
        e_last = (fo + n) * length
        for level, s, gamma, attempt in itertools.product(LEVELS, SAMPLES, GAMMAS, ATTEMPTS):
            got = beta_latent_words(n, length, seed=SEED, draw=draw, level=level, s=s, gamma=gamma, attempt=attempt, first_object=fo)
            assert got.dtype == np.uint32 and got.shape == (n, length, 4)
            assert np.array_equal(got, _numpy_words(n, length, fo, draw, level, s, gamma, attempt)), (fo, level, s, gamma, attempt)
        assert fo == 0 or fo == 3 or e_last > 2 ** 32
    w = tbl.words(n, length, SEED, draw, 3, 5, first_object=7)
    for gamma, attempt in ((0, 0), (1, 0), (0, 15), (1, 7)):
        assert np.array_equal(w[:, :, gamma, attempt],
                              beta_latent_words(n, length, seed=SEED, draw=draw, level=3, s=5, gamma=gamma, attempt=attempt, first_object=7))
    # other seed, draw, level, s: other words
    base = beta_latent_words(n, length, seed=SEED, draw=draw, level=1, s=1, gamma=0, attempt=0)
    for kw in (dict(seed=SEED + 1), dict(draw=draw + 1), dict(level=2), dict(s=2), dict(gamma=1), dict(attempt=1)):
        args = dict(dict(seed=SEED, draw=draw, level=1, s=1, gamma=0, attempt=0), **kw)
        assert not np.array_equal(base, beta_latent_words(n, length, **args)), kw


def test_fourth_counter_words_are_distinct():
    """The words of all corners are pairwise distinct, and none is a word the head can form (0x42000000 | gamma << 8 | attempt) or one of
    the other streams' (the Normal latents' 0x4C...... , dropout's 0x44......, 0x00544E48, 0x00484D43, 0)."""
    corners = [tbl.word3(*c) for c in itertools.product(LEVELS, SAMPLES, GAMMAS, ATTEMPTS)]
    assert len(set(corners)) == len(corners) == 40
    everything = {tbl.word3(level, s, g, k) for level in (0, 1, 255) for s in range(tbl.MAX_NS) for g in (0, 1) for k in range(16)}
    assert len(everything) == 3 * tbl.MAX_NS * 32                                       # the fields do not overlap
    head = {tb.TAG | (g << 8) | k for g in (0, 1) for k in range(16)}
    assert not head & everything and not head & set(corners)
    assert all(w >> 24 == 0x51 for w in everything)
    assert all(w >> 24 not in (0x42, 0x44, 0x4C, 0x00) for w in everything)
    assert tbl.word3(255, 2047, 1, 15) == 0x51FFFFFF


def _positive_operands(kind, n=4096, seed=21):
    loc, ls = tbl.operands(kind, 1, n, seed)
    return tb._pr(loc, D)[0].ravel(), tb._pr(ls, D)[0].ravel()


@pytest.mark.parametrize("kind", list(tbl.RANGES))
def test_kl_twin_is_torch_float64_kl_divergence(kind):
    a, b = _positive_operands(kind)
    ta, tb_ = torch.from_numpy(a), torch.from_numpy(b)
    want = torch.distributions.kl_divergence(torch.distributions.Beta(ta, tb_),
                                             torch.distributions.Beta(torch.full_like(ta, 0.5), torch.full_like(ta, 0.5))).numpy()
    got = tbl.kl(a, b)
    rel = np.abs(got - want) / np.abs(want)
    print(f"{kind}: KL twin against torch float64: worst relative {rel.max():.3e}, largest KL {want.max():.3e}")
    assert np.isfinite(got).all() and rel.max() <= 1e-12


@pytest.mark.parametrize("kind", list(tbl.RANGES))
def test_closed_form_gradient_is_float64_autograd_of_the_kl(kind):
    """The closed form (only trigammas: the digamma terms cancel exactly) is the reference; float64 autograd of the expression is held
    to it within 1e-6 relative, per sample.  WHICH samples: h_a = (a - 1/2) psi'(a) + m psi'(a + b) changes sign inside every range (the
    KL term's minimum along a), and torch's float64 trigamma -- what autograd differentiates the digammas with -- is good to 4.9e-10
    relative only (measured against scipy and mpmath; its series stops at 1/42x^7 from x = 6 on).  Where the two terms of h cancel to
    less than 1e-3 of their size S = |(a - 1/2) psi'(a)| + |m psi'(a + b)| that error alone exceeds 4.9e-7 of h and a relative comparison
    with autograd measures torch, not the closed form (over all samples the worst is 6.3e-6, at a = 3.09, b = 39.9 with |h| = 3.2e-5 and
    S = 2.0; mpmath puts the closed form there within 9.4e-12).  So autograd is compared where |h| >= 1e-3 S -- at least 99.5 % of every
    range here, worst 2.2e-7; 52 samples left out in all --, and EVERY one of the 4096 samples of both gradients, those near the sign
    change included, is held to mpmath (40 digits) within 1e-13 S, the float64 rounding of the two terms."""
    import mpmath
    a, b = _positive_operands(kind)
    ta, tb_ = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    k = ((float(np.log(np.pi)) - (torch.lgamma(ta) + torch.lgamma(tb_) - torch.lgamma(ta + tb_)))
         + (ta - 0.5) * torch.digamma(ta) + (tb_ - 0.5) * torch.digamma(tb_) + (1 - ta - tb_) * torch.digamma(ta + tb_))
    ga, gb = torch.autograd.grad(k.sum(), (ta, tb_))
    ha, hb = tbl.kl_grad(a, b)
    m, p1ab = (1.0 - a) - b, special.polygamma(1, a + b)
    worst, kept, left_out = 0.0, 1.0, 0
    for h, g, c in ((ha, ga.numpy(), a), (hb, gb.numpy(), b)):
        S = np.abs((c - 0.5) * special.polygamma(1, c)) + np.abs(m * p1ab)
        keep = np.abs(h) >= 1e-3 * S
        worst, kept = max(worst, float(np.max(np.abs(h - g)[keep] / np.abs(h)[keep]))), min(kept, float(keep.mean()))
        with mpmath.workdps(40):                                          # all 4096 samples, none strided over
            exact = np.array([float((mpmath.mpf(float(x)) - 0.5) * mpmath.polygamma(1, float(x))
                                    + (1 - mpmath.mpf(float(x)) - mpmath.mpf(float(y))) * mpmath.polygamma(1, mpmath.mpf(float(x)) + mpmath.mpf(float(y))))
                              for x, y in zip(c, b if c is a else a)])
        assert exact.shape == h.shape and (np.abs(h - exact) <= 1e-13 * S).all()
        left_out += int((~keep).sum())
    print(f"{kind}: closed-form gradient against float64 autograd where |h| >= 1e-3 S ({kept:.3f} of the samples; "
          f"{left_out} left out, held to mpmath like all the others): worst relative {worst:.3e}")
    assert kept >= 0.95 and worst <= 1e-6
    # the float32 results stay finite over the whole operand range the kernel can meet
    aa, bb = np.meshgrid(np.geomspace(1.2e-7, 300, 60), np.geomspace(1.2e-7, 300, 60))
    assert np.isfinite(tbl.kl(aa, bb).astype(F)).all() and all(np.isfinite(g.astype(F)).all() for g in tbl.kl_grad(aa, bb))


def test_trigamma_restatement_is_polygamma():
    x = np.geomspace(1e-7, 1e5, 20001)
    rel = np.abs(tbl.trigamma_kernel(x) - special.polygamma(1, x)) / special.polygamma(1, x)
    print(f"trigamma restatement against scipy: worst relative {rel.max():.3e}")
    assert rel.max() <= 1e-14
    assert np.isnan(tbl.trigamma_kernel(np.array([np.nan]))).all()


def test_lgamma_digamma_restatement_is_scipy():
    """beta_head.h's beta_lgamma_digamma, restated operation by operation in the twin, against scipy's gammaln and digamma over
    x in [1e-7, 1e5].  Both functions have zeros (x = 1, 2; x = 1.4616), so the bound is absolute: the twin's lgamma_digamma_bounds,
    which counts the restatement's own roundings (its docstring names them).  Measured: worst 0.23 of the bound for lgamma (7.1e-15
    absolute, at the zeros), 0.29 for digamma (whose error is 9.5 * 2^-53 / x for small x: the recurrence's).  The KL term built
    from it is the scipy twin's within kl_float64_bound, the float64 term of the kl bar."""
    x = np.geomspace(1e-7, 1e5, 20001)
    lg, psi = tbl.lgamma_digamma_kernel(x)
    bound_lg, bound_psi = tbl.lgamma_digamma_bounds(x)
    r_lg = np.abs(lg - special.gammaln(x)) / bound_lg
    r_psi = np.abs(psi - special.digamma(x)) / bound_psi
    print(f"lgamma / digamma restatement against scipy: worst {r_lg.max():.3f} / {r_psi.max():.3f} of the bound; "
          f"lgamma absolute {np.abs(lg - special.gammaln(x)).max():.3e}")
    assert r_lg.max() <= 1.0 and r_psi.max() <= 1.0
    lgn, psin = tbl.lgamma_digamma_kernel(np.array([np.nan]))
    assert np.isnan(lgn).all() and np.isnan(psin).all()
    for kind in tbl.RANGES:
        a, b = _positive_operands(kind)
        r = np.abs(tbl.kl_kernel(a, b) - tbl.kl(a, b)) / tbl.kl_float64_bound(a, b)
        print(f"{kind}: the kernel's form of kl against the scipy twin: worst {r.max():.3f} of the float64 term of its bar")
        assert r.max() <= 1.0


def test_z_bar_is_np_twin_betas_bar_of_x():
    """np_twin_beta_latent.z_bar restates np_twin_beta.bars' bar of x (so that callers wanting values alone skip the gradients' dlg
    evaluations): equal bits on every range."""
    for kind in tbl.RANGES:
        loc, ls = tbl.operands(kind, 2, 257, 31)
        sch = tb.search(loc, ls, tbl.words(2, 257, SEED, 1, 2, 0), F)
        ref = tb.compose(loc, ls, (sch["zn"], sch["ub"]), D)
        want = tb.bars(ref, np.zeros((2, 257)), np.zeros(2))["x"]
        assert np.array_equal(tbl.z_bar(ref), want), kind


@pytest.fixture(scope="module", params=list(tbl.RANGES))
def twin_case(request):
    return tbl.case(request.param, 2, 1024, 2, 11, draw=3, level=1, first_object=5)


def test_float32_twin_stays_under_the_cap(twin_case):
    """The project's rule: the float32 composition is within R * bar of float64 per sample, R <= R_MAX -- the twin cannot quietly widen
    the bar the kernels are held to."""
    for k, R in twin_case["R"].items():
        print(k, R)
        assert 1.0 <= R <= tbl.R_MAX, (k, R)


def test_the_bars_bite(twin_case):
    """A relative error of 1e-4 in the KL term, or of 1e-3 in its gradient, misses the bar on most samples: the bars are of the size of
    float32 rounding, not of the quantity."""
    c = twin_case
    e = tb.excess(c["want"]["kl"] * (1 + 1e-4), c["want"]["kl"], c["bar"]["kl"])
    assert np.median(e) > tbl.MARGIN * c["R"]["kl"]
    only_kl = tbl.bars(c["ref"], None, c["g_KL"])
    g = tbl.gradients(c["ref"], None, c["g_KL"])[0]
    e = tb.excess(g * (1 + 1e-3), g, only_kl["g_loc"])
    assert np.median(e) > tbl.MARGIN * tbl.R_MAX


def test_ordered_sum_is_a_sum():
    row = np.random.default_rng(0).standard_normal(4100).astype(F)
    assert abs(float(tbl.ordered_sum(row)) - float(row.astype(D).sum())) <= 4100 * tbl.U * float(np.abs(row).sum())
    assert tbl.ordered_sum(np.array([1.5], F)) == F(1.5)


# ---- argument rules ---------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(lib):
    L = lib.load()
    p = 16                                                               # any non-null address: every refusal comes before a launch
    good_f = [p, 2, 8, 2, 0, 1, 0, 0, p, p, None, None, None]
    for i in (0, 8):
        bad = list(good_f)
        bad[i] = None
        assert L.ctpvae_beta_latent_fwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((1, 0), (2, -3), (3, 0), (3, 2049), (4, -1), (4, 2 ** 63 - 1), (7, 256)):
        bad = list(good_f)
        bad[i] = v
        assert L.ctpvae_beta_latent_fwd_f32(*bad) == lib.EINVAL, (i, v)
    bad = list(good_f)
    bad[1], bad[2] = 2 ** 15, 2 ** 15                                    # ns * B * len >= 2^31
    assert L.ctpvae_beta_latent_fwd_f32(*bad) == lib.EINVAL and "31 bits" in lib.last_error()
    good_b = [p, 2, 8, 2, 0, 1, 0, 0, None, None, p, None]
    for i in (0, 10):
        bad = list(good_b)
        bad[i] = None
        assert L.ctpvae_beta_latent_bwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((1, 0), (2, -3), (3, 0), (3, 2049), (4, -1), (7, 256)):
        bad = list(good_b)
        bad[i] = v
        assert L.ctpvae_beta_latent_bwd_f32(*bad) == lib.EINVAL, (i, v)
    assert L.ctpvae_beta_latent_words_host_u32(2, 8, 0, 1, 0, 0, 0, 0, 0, None) == lib.EINVAL and "null" in lib.last_error()
    for n, length, fo, level, s, gamma, attempt in ((0, 8, 0, 0, 0, 0, 0), (2, 0, 0, 0, 0, 0, 0), (2, 8, -1, 0, 0, 0, 0), (2, 8, 2 ** 63 - 1, 0, 0, 0, 0),
                                                    (2, 8, 0, 256, 0, 0, 0), (2, 8, 0, 0, 2048, 0, 0), (2, 8, 0, 0, -1, 0, 0), (2, 8, 0, 0, 0, 2, 0),
                                                    (2, 8, 0, 0, 0, 0, 16), (2 ** 16, 2 ** 15, 0, 0, 0, 0, 0)):
        assert L.ctpvae_beta_latent_words_host_u32(n, length, fo, 1, 0, level, s, gamma, attempt, p) == lib.EINVAL, (n, length, fo, level, s)


def test_python_wrapper_refuses_what_it_cannot_run(lib):
    from ct_pvae_amd import beta_latent_words, beta_latents
    a = torch.zeros(2, 4, 5, 7)
    kw = dict(ns=2, seed=0, draw=0, level=0)
    with pytest.raises(TypeError):
        beta_latents(a.numpy(), **kw)
    with pytest.raises(TypeError):
        beta_latents(a.double(), **kw)
    with pytest.raises(ValueError):
        beta_latents(a[:, 0], **kw)                                          # not [B][2C][H][W]
    with pytest.raises(ValueError):
        beta_latents(torch.zeros(2, 3, 5, 7), **kw)                          # odd channel count
    with pytest.raises(ValueError):
        beta_latents(torch.zeros(2, 8, 5, 7)[:, :4], **kw)                   # a channel half: not contiguous
    for bad in (dict(ns=0), dict(ns=2049), dict(level=-1), dict(level=256), dict(draw=2 ** 32), dict(draw=-1)):
        with pytest.raises(ValueError):
            beta_latents(a, **dict(kw, **bad))
    with pytest.raises(ValueError):
        beta_latents(a, first_object=-1, **kw)
    with pytest.raises(lib.RadonLibraryError):
        beta_latents(a, **kw)                                                # CPU tensors: there is no CPU path
    with pytest.raises(lib.RadonLibraryError):
        beta_latents(a, want_kl=False, **kw)
    wkw = dict(seed=0, draw=0, level=0, s=0, gamma=0, attempt=0)
    for bad in (dict(level=256), dict(s=2048), dict(s=-1), dict(gamma=2), dict(attempt=16)):
        with pytest.raises(ValueError):
            beta_latent_words(2, 5, **dict(wkw, **bad))
    with pytest.raises(ValueError):
        beta_latent_words(0, 5, **wkw)


def test_fused_beta_latents_argument_rules():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).fused_beta_latents is False                                   # off by default
    a = tr.get_args(["--fused_beta_latents"])
    assert a.fused_beta_latents is True and a.fused_beta_head is False and a.head_seed == 1234
    both = tr.get_args("--fused_beta_latents --fused_beta_head --fused_blocks --dp 0.1".split())
    assert both.fused_beta_head is True and both.fused_blocks is True
    with pytest.raises(ValueError):
        tr.get_args("--normal --fused_beta_latents".split())
    with pytest.raises(ValueError):
        tr.get_args("--det --fused_beta_latents".split())
    with pytest.raises(ValueError, match="fused_beta_latents"):
        tr.get_args(["--fused_latents"])                                                 # still refused; the message names the new flag
    for bad in (dict(use_normal=True), dict(use_normal=False, deterministic=True)):
        with pytest.raises(ValueError):
            tr.find_loss_vae_unsup(None, None, None, None, None, 1.0, 1e-7, 1.0, 1.0, fused_beta_latents=(0, 0, 0), **bad)
    with pytest.raises(ValueError, match="fused_beta_latents"):
        tr.find_loss_vae_unsup(None, None, None, None, None, 1.0, 1e-7, 1.0, 1.0, fused_latents=(0, 0, 0), use_normal=False)
    # the constructor checks again (arguments built without get_args), before it touches the device
    for flags in ("--nsa 20 --td 6 -b 3 --normal", "--nsa 20 --td 6 -b 3 --det"):
        args = tr.get_args(flags.split())
        args.fused_beta_latents = True
        with pytest.raises(ValueError):
            tr.PVAETrainer(args, torch.device("cpu"))


def test_kernels_compile_for_gfx950_without_scratch():
    """hipcc's own resource report (-Rpass-analysis) for csrc/beta_latent.hip with the library's flags: both kernels are there and
    neither uses scratch (the library's float64 lgamma alone costs the forward 128 registers and a spill: beta_head.h's
    beta_lgamma_digamma)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    csrc = os.path.join(ROOT, "ct_pvae_amd", "csrc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "beta_latent.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "beta_latent" in name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == 2 and any("fwd" in k for k in scratch) and any("bwd" in k for k in scratch), scratch
    assert all(v == 0 for v in scratch.values()), scratch
