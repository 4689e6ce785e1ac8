"""Host side of the fused Beta output head (ct_pvae_amd/beta_head.py, csrc/beta_head.hip, beta_head.h): the stream's layout, the
twins and the acceptance rule of tests/np_twin_beta.py (the float32 twin stays under the cap; the bar bites; the float64 dlg against
mpmath; the gradient IS the implicit one), the argument checks, the compiler's resource report and the trainer's flag.  The kernels
themselves: tests/test_gpu_beta_head.py."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import special

from tests import np_twin_beta as tb
from tests.conftest import ROOT

F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


@pytest.fixture(scope="module", params=list(tb.RANGES))
def twin_case(request):
    return tb.case(request.param, 4, 4096, 11)


@pytest.mark.parametrize("first_object", [0, 3, 1000003, 2 ** 32 // 35 - 1])
def test_host_words_are_the_numpy_philox_word_for_word(lib, first_object):
    """Both gammas, attempts 0, 1 and 15; the last first_object carries e past 2^32 inside the call (the second counter word)."""
    from ct_pvae_amd import beta_head_words
    n, pix, seed, draw = 3, 35, 0x1234567887654321, 7
    if first_object > 2 ** 24:
        assert first_object * pix < 2 ** 32 < (first_object + n) * pix
    want = tb.words(n, pix, seed, draw, first_object, gammas=(0, 1), attempts=(0, 1, 15))
    seen = set()
    for j in (0, 1):
        for i, k in enumerate((0, 1, 15)):
            got = beta_head_words(n, pix, seed=seed, draw=draw, first_object=first_object, gamma=j, attempt=k)
            assert got.dtype == np.uint32 and got.shape == (n, pix, 4)
            assert np.array_equal(got, want[:, :, j, i])
            seen.add(got.tobytes())
    assert len(seen) == 6                                   # every (gamma, attempt) is a block of its own
    got = beta_head_words(n, pix, seed=seed, draw=draw, first_object=first_object, gamma=1, attempt=15)
    assert not np.array_equal(got, beta_head_words(n, pix, seed=seed, draw=draw + 1, first_object=first_object, gamma=1, attempt=15))
    assert not np.array_equal(got, beta_head_words(n, pix, seed=seed + 1, draw=draw, first_object=first_object, gamma=1, attempt=15))
    assert np.array_equal(got[1:], beta_head_words(n - 1, pix, seed=seed, draw=draw, first_object=first_object + 1, gamma=1, attempt=15))


def test_beta_tag_differs_from_the_other_streams():
    from tests import np_twin_head, np_twin_hmc
    used = (np_twin_head.TAG, np_twin_hmc.TAG, 0)
    assert all((tb.TAG | (j << 8) | k) not in used for j in (0, 1) for k in range(16))
    assert tb.TAG >> 24 not in (0x4C, 0x44)                  # the latents' and the dropout's tag families
    src = open(os.path.join(ROOT, "ct_pvae_amd", "csrc", "beta_head.h")).read()
    assert re.search(r"kBetaTag\s*=\s*0x%Xu" % tb.TAG, src)
    assert re.search(r"kDlgMaxTerms\s*=\s*%d;" % tb.KERNEL_MAX_TERMS, src)


def test_float32_twin_stays_under_the_cap(twin_case):
    """The project's rule: the float32 twin is within R * bar of float64 per sample, R <= R_MAX."""
    print("left out", int(twin_case["skip"].sum()))
    assert twin_case["skip"].mean() <= 0.01
    for k, R in twin_case["R"].items():
        print(k, R)
        assert 1.0 <= R <= tb.R_MAX, (k, R)


def test_the_bar_bites():
    """A float32 twin with one planted defect puts more than 1 % of the trainer range's samples outside 4 R bar: dlg off by 1e-4 of
    itself; lp's path through x let through the clamp; y taken as 1 - x."""
    c = tb.case("trainer", 4, 4096, 11)
    twin = tb.compose(c["alpha"], c["beta"], c["draws"], F)
    for defect in ("dlg_1e-4", "no_gate"):
        got = dict(zip(("g_alpha", "g_beta"), tb.gradients(twin, c["g_x"], c["g_LP"], defect=defect)))
        for k in got:
            outside = float((tb.excess(got[k], c["want"][k], c["bar"][k]) > tb.MARGIN * c["R"][k]).mean())
            print(defect, k, outside)
            assert outside > 0.01, (defect, k, outside)
    d = tb.compose(c["alpha"], c["beta"], c["draws"], F, defect="one_minus_x")
    outside = float((tb.excess(d["lp"], c["want"]["lp"], c["bar"]["lp"]) > tb.MARGIN * c["R"]["lp"]).mean())
    print("one_minus_x lp", outside)
    assert outside > 0.01


def test_float64_dlg_against_mpmath():
    """-diff(P regularised, c) / (g p(g)) at 50 digits on the grid c x quantile; the twin's series / continued fraction stay within 1e-10
    relative.  Where the quantile itself underflows float64 (tiny c) the point is given in log space, lg = (log q + lgamma(c + 1)) / c,
    the quantile's leading term -- any lg is a valid point."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    worst, iters = 0.0, []
    for c in (1e-6, 1e-3, 0.3, 1, 2, 8, 50, 1000, 1e5):
        for q in (1e-6, 0.01, 0.5, 0.99, 1 - 1e-6):
            g = special.gammaincinv(c, q)
            lg = float(np.log(g)) if g > 1e-300 else float((np.log(q) + special.gammaln(c + 1)) / c)
            cm, lgm = mp.mpf(c), mp.mpf(lg)
            gm = mp.exp(lgm)
            dP = mp.diff(lambda cc: mp.gammainc(cc, 0, gm, regularized=True), cm)
            dens = mp.exp(cm * lgm - gm - mp.loggamma(cm))
            want = -dP / dens
            got = float(tb.dlg(c, lg, count=iters))
            rel = float(abs((got - want) / want))
            worst = max(worst, rel)
            assert rel <= 1e-10, (c, q, got, float(want), rel)
    print(f"worst relative error {worst:.2e}; most iterations {max(iters)} (at c = 1e5; the kernel's bound is {tb.KERNEL_MAX_TERMS})")
    # the kernel's hard bound covers every concentration up to 4e4 (the test ranges end at 40)
    iters = []
    cs = np.array([40.0, 1e3, 4e4])
    for q in (0.3, 0.5, 0.7):
        tb.dlg(cs, np.log(special.gammaincinv(cs, q)), count=iters)
    assert max(iters) <= tb.KERNEL_MAX_TERMS, iters
    # ... and beyond it the bounded sum says so: NaN, not a truncated value
    lg5 = float(np.log(special.gammaincinv(2e5, 0.5)))
    assert np.isnan(tb.dlg(2e5, lg5, max_terms=tb.KERNEL_MAX_TERMS)) and np.isfinite(tb.dlg(2e5, lg5))


def test_hand_written_digamma_against_scipy():
    x = np.concatenate([10.0 ** np.linspace(-7, 5, 400), np.linspace(0.5, 12, 400)])
    got, want = tb.digamma_kernel(x), special.digamma(x)
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-14


@pytest.mark.parametrize("kind", list(tb.RANGES))
def test_float32_and_float64_search_agree(kind):
    """The accepted attempt of the float32 and of the float64 attempt loop differ on at most 1e-4 of the gammas, and only where the
    float64 acceptance margin of the earlier of the two attempts is inside its own float32 bar."""
    n, pix = 16, 8192
    al, be = tb.operands(kind, n, pix, 3)
    w = tb.words(n, pix, 5, 3)
    s32, s64 = tb.search(al, be, w, F), tb.search(al, be, w, D)
    dis = s32["k"] != s64["k"]
    print(kind, "disagree", int(dis.sum()), "of", dis.size, "refused at least once", float((s64["k"] > 0).mean()))
    assert dis.mean() <= 1e-4
    first = np.minimum(s32["k"], s64["k"])[..., None]
    m = np.take_along_axis(s64["margin"], first, axis=-1)[..., 0]
    b = np.take_along_axis(s64["bar"], first, axis=-1)[..., 0]
    assert (np.abs(m[dis]) <= tb.MARGIN * b[dis]).all()
    assert float((s64["k"] > 0).mean()) <= 0.05            # the refusal rate the cap of 16 attempts rests on


def test_gradient_is_the_implicit_one():
    """The float64 gradient of compose against a central difference of compose in alpha and beta at fixed UNIFORMS OF THE IMPLICIT FORM:
    move c, solve P(c', g') = P(c, g) for g' (scipy's gammaincinv), re-evaluate x and lp at log g'.  Concentrations in [0.05, 50]; the
    pixels are independent (f_i = x_i g_x_i + G lp_i), so all move at once."""
    rng = np.random.default_rng(0)
    n, pix = 2, 600
    conc = np.exp(rng.uniform(np.log(0.05), np.log(50.0), (2, n, pix)))
    raw = np.where(conc >= 1, conc, 1 + np.log(np.maximum(conc - tb.EPS32, 1e-3))).astype(F)
    alpha, beta = raw[0], raw[1]
    # draws in the bulk of each gamma: quantiles in [0.02, 0.98] given directly in log space
    q = rng.uniform(0.02, 0.98, (n, pix, 2))
    c0 = tb.compose(alpha, beta, (np.zeros((n, pix, 2), F), np.full((n, pix, 2), 0.5, F)), D, sr=1e-3)
    cc = c0["c"]
    assert cc.min() >= 0.049 and cc.max() <= 50.1
    lg0 = np.log(special.gammaincinv(cc, q))
    P = special.gammainc(cc, np.exp(lg0))
    g_x, g_LP = tb.cotangents(n, pix, 2)
    ref = tb.compose(alpha, beta, (c0["zn"], c0["ub"]), D, sr=1e-3, lg=lg0)
    ga, gb = tb.gradients(ref, g_x, g_LP)
    keep = ref["passes"] & (ref["x"] > 1.1e-3) & (ref["y"] > 1.1e-3)         # clear of the clamp: the difference must not straddle it
    assert keep.mean() > 0.5

    def f(which, sign):
        h = 1e-5 * cc[..., which]
        c2 = cc.copy()
        c2[..., which] += sign * h
        lg2 = lg0.copy()
        lg2[..., which] = np.log(special.gammaincinv(c2[..., which], P[..., which]))
        # compose takes raw operands: above 1 the raw operand IS the concentration; below, invert pr in float64 and pass it as a
        # float64 `lg`-given composition whose concentrations are patched in
        r = tb.compose(alpha, beta, (c0["zn"], c0["ub"]), D, sr=1e-3, lg=lg2)
        a, b = (c2[..., 0], c2[..., 1])
        lp = ((a - 1) * np.log(r["xc"]) + (b - 1) * np.log(r["yc"])) - ((special.gammaln(a) + special.gammaln(b)) - special.gammaln(a + b))
        return r["x"] * g_x + g_LP[:, None].astype(D) * lp, h

    for which, got in ((0, ga), (1, gb)):
        (fp, h), (fm, _) = f(which, +1), f(which, -1)
        fd = (fp - fm) / (2 * h) * ref["dc"][..., which]
        err = np.abs(got - fd)[keep] / np.maximum(1.0, np.abs(fd)[keep])
        print("alpha" if which == 0 else "beta", "worst |closed form - central difference| / max(1, |fd|)", float(err.max()))
        assert err.max() <= 1e-5
    # torch's own Beta.rsample derivative is ANOTHER estimator: per sample it differs from the implicit gamma gradient
    xs, conc_t = torch.tensor(ref["x"]), torch.tensor(cc)
    dx_torch = torch._dirichlet_grad(torch.stack([xs, 1 - xs], -1), conc_t, conc_t.sum(-1, keepdim=True).expand(n, pix, 2).contiguous())
    dx_implicit = ref["x"] * ref["y"] * tb.dlg(cc[..., 0], lg0[..., 0])
    assert dx_torch.shape == (n, pix, 2) and not np.allclose(dx_torch[..., 0].numpy(), dx_implicit, rtol=1e-3)


def test_bad_arguments_are_einval_before_any_hip_call(lib):
    L = lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # (host pointers: every call below is refused before the pointer is used or a HIP call is made)
    good_f = [p, p, 2, 8, 0, 1, 0, 1e-7, p, p, None, None, None]
    for i in (0, 1, 8, 9):
        bad = list(good_f)
        bad[i] = None
        assert L.ctpvae_beta_head_fwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((2, 0), (2, -1), (3, 0), (4, -1), (4, 2 ** 63 - 1), (7, 0.0), (7, -1e-7), (7, 0.5), (7, float("nan"))):
        bad = list(good_f)
        bad[i] = v
        assert L.ctpvae_beta_head_fwd_f32(*bad) == lib.EINVAL, (i, v)
    assert L.ctpvae_beta_head_fwd_f32(p, p, 2 ** 16, 2 ** 15, 0, 1, 0, 1e-7, p, p, None, None, None) == lib.EINVAL     # n * pix = 2^31
    good_b = [p, p, 2, 8, 0, 1, 0, 1e-7, None, None, p, p, None]
    for i in (0, 1, 10, 11):
        bad = list(good_b)
        bad[i] = None
        assert L.ctpvae_beta_head_bwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for i, v in ((2, 0), (3, -3), (4, -1), (7, 0.75)):
        bad = list(good_b)
        bad[i] = v
        assert L.ctpvae_beta_head_bwd_f32(*bad) == lib.EINVAL
    assert L.ctpvae_beta_head_words_host_u32(2, 8, 0, 1, 0, 0, 0, None) == lib.EINVAL and "null" in lib.last_error()
    for n, pix, fo, j, k in ((0, 8, 0, 0, 0), (2, 0, 0, 0, 0), (2, 8, -1, 0, 0), (2, 8, 2 ** 63 - 1, 0, 0), (2, 8, 0, 2, 0), (2, 8, 0, 0, 16),
                             (2, 8, 0, -1, 0), (2, 8, 0, 0, -1)):
        assert L.ctpvae_beta_head_words_host_u32(n, pix, fo, 1, 0, j, k, p) == lib.EINVAL


def test_python_wrapper_refuses_what_it_cannot_run(lib):
    from ct_pvae_amd import beta_head, beta_head_words
    a = torch.zeros(2, 1, 5, 7)
    with pytest.raises(TypeError):
        beta_head(a.numpy(), a, seed=0, draw=0)
    with pytest.raises(TypeError):
        beta_head(a.double(), a.double(), seed=0, draw=0)
    with pytest.raises(ValueError):
        beta_head(a[:, 0], a[:, 0], seed=0, draw=0)                       # not [n][1][X][Y]
    with pytest.raises(ValueError):
        beta_head(torch.zeros(2, 2, 5, 7)[:, :1], a, seed=0, draw=0)      # a channel half: not contiguous
    with pytest.raises(ValueError):
        beta_head(a, torch.zeros(2, 1, 7, 5), seed=0, draw=0)
    with pytest.raises(ValueError):
        beta_head(a, a, seed=0, draw=2 ** 32)
    with pytest.raises(ValueError):
        beta_head(a, a, seed=0, draw=0, first_object=-1)
    for sr in (0.0, 0.5, -1.0, float("nan")):
        with pytest.raises(ValueError):
            beta_head(a, a, seed=0, draw=0, sqrt_reg=sr)
    with pytest.raises(lib.RadonLibraryError):
        beta_head(a, a, seed=0, draw=0)                                   # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        beta_head_words(0, 5, seed=0, draw=0, gamma=0, attempt=0)
    with pytest.raises(ValueError):
        beta_head_words(1, 5, seed=0, draw=0, gamma=2, attempt=0)
    with pytest.raises(ValueError):
        beta_head_words(1, 5, seed=0, draw=0, gamma=0, attempt=16)


def test_beta_head_kernels_use_no_scratch_and_spill_no_vgpr():
    """hipcc's own resource report for csrc/beta_head.hip with the library's flags."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "beta_head.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    name, scratch, spills = None, {}, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m:
            spills[name] = int(m.group(1))
    assert any("beta_head_fwd_kernel" in k for k in scratch) and any("beta_head_bwd_kernel" in k for k in scratch), scratch
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(v == 0 for v in spills.values()), spills


def test_fused_beta_head_argument_rules():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).fused_beta_head is False                                    # off by default
    a = tr.get_args(["--fused_beta_head"])
    assert a.fused_beta_head is True and a.head_seed == 1234 and a.use_normal is False
    assert tr.get_args("--fused_beta_head --det --head_seed 5".split()).head_seed == 5  # allowed with --det
    with pytest.raises(ValueError):
        tr.get_args("--fused_beta_head --normal".split())
    with pytest.raises(ValueError):
        tr.get_args(["--fused_head"])                                                  # unchanged: the TruncatedNormal head needs --normal
    with pytest.raises(ValueError):
        tr.find_loss_vae_unsup(None, None, None, None, None, 1.0, 1e-7, 1.0, 1.0, use_normal=True, fused_beta_head=(0, 0, 0))
    assert "--fused_beta_head" in subprocess.run([sys.executable, "-m", "ct_pvae_amd.trainer", "--help"], cwd=ROOT, capture_output=True,
                                                 text=True).stdout
