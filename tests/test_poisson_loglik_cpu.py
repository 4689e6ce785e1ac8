"""noise="poisson" without a GPU: the evaluation form's error against float64 (and the textbook form's, which it replaces), the
edge cases of the definition, the ABI, argument checks, and the register / trap gates over the new kernels.

The per-sample rule of tests/np_twin_poisson.py (|got - ref| <= MARGIN * R * bar, the rule the GPU tests hold the kernels to) is
checked here from the other side: the float32 twin stays within R_MAX bars of the float64 reference on every operand kind, the
operand kinds sit on the seams they are named after, reference_dlogp is float64 autograd of reference_logp's formula, and four
wrong twins -- a lost series term, a lost logf(lam / k) branch, a lost mask factor, a lost k == 0 case -- are refused.

Seen here (seven kinds x pnm in {1, 1e2, 1e4, 1e6} at (5, 12, 184), and (3, 20, 9001) with one kind per pnm): the twin's worst
excess is 0.41 .. 0.92 for lp and 0.18 .. 0.81 for dlp, so R = 1 everywhere.  The series without 1 / (360 k^3) reaches 12.3 bars on
seam_k (allowed: 4) while the older bar_from_twin rule passes it at 0.2 of its bar; log1pf taken everywhere reaches 1.06e3 bars on
small_k."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_poisson as tw
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ctpvae_radon.h")
NEW_SYMBOLS = ("ctpvae_poisson_loglik_fwd_f32", "ctpvae_poisson_loglik_bwd_f32", "ctpvae_rotate_fwd_compact_noise_f32",
               "ctpvae_siddon_fwd_loglik_noise_f32")


def table_operands(pnm, n=200_000, seed=0):
    """mask = 1 / 20, proj in [0, 120), measurements drawn from the model itself (counts / pnm)."""
    rng = np.random.default_rng(seed)
    proj = (rng.random((1, 1, n)) * 120.0).astype(np.float32)
    mask = np.full((1, 1), 1.0 / 20.0, np.float32)
    lam = proj.astype(np.float64) * np.float64(mask[0, 0]) * pnm
    x = (rng.poisson(lam) / pnm).astype(np.float32)
    return proj, mask, x


@pytest.mark.parametrize("pnm", [1.0, 1e2, 1e4])
def test_stable_form_against_float64(pnm):
    proj, mask, x = table_operands(pnm)
    want = tw.reference_logp(proj, mask, x, pnm)
    e_twin, ok_twin = tw.errors(tw.twin_logp(proj, mask, x, pnm), want)
    e_naive, _ = tw.errors(tw.naive_logp(proj, mask, x, pnm), want)
    print(f"pnm {pnm:g}: max abs error twin {e_twin:.3e} naive {e_naive:.3e} median |lp| {np.median(np.abs(want)):.2f}")
    assert ok_twin
    # this test prints 2.0e-6 / 1.3e-5 / 1.0e-4 at pnm 1 / 1e2 / 1e4.  The error is the rounding of lam and k themselves, carried into
    # lp by d lp / d lam = (k - lam) / lam: ~ 2^-23 |k - lam|, and draws reach |k - lam| ~ 4.5 sqrt(k) ~ 1e3 at k ~ 6e4
    assert e_twin <= 2e-4
    if pnm >= 1e2:
        assert e_naive >= 10.0 * e_twin


def test_twin_on_non_integer_measurements():
    rng = np.random.default_rng(1)
    proj = (rng.random((2, 5, 4000)) * 120.0).astype(np.float32)
    mask = rng.uniform(0.02, 0.08, (2, 5)).astype(np.float32)
    x = (rng.random((2, 5, 4000)) * 6.0).astype(np.float32)
    # Per sample, |got - want| <= atol + rtol |want| (never an error divided by the largest |lp|: one badly mismatched sample would
    # carry every other).  k and lam are independent here, so |k - lam| reaches 1e5 and so does |lp|.  The error is the rounding of
    # lam and k carried through d lp / d lam = (k - lam) / lam: err <= c 2^-24 |k - lam| with c = 6 (two roundings in lam, one in k,
    # the quotient, the logarithm, the difference), while |lp| >= (k - lam)^2 / (4 max(k, lam)).  atol is the bound at the mode
    # (2e-4, the test above); atol + rtol |lp| covers c 2^-24 d for every d = |k - lam| once atol * rtol >= (c 2^-24)^2 max(k, lam)
    # = 1.2e-8 at max(k, lam) = 9.6e4: rtol = 1e-4.
    atol, rtol = 2e-4, 1e-4
    for pnm in (1.0, 1e2, 1e4):
        want = tw.reference_logp(proj, mask, x, pnm)
        ratio, e, ok = tw.worst_excess(tw.twin_logp(proj, mask, x, pnm), want, atol, rtol)
        print(f"pnm {pnm:g}: non-integer k, max abs error {e:.3e}, worst |err| / (atol + rtol |lp|) {ratio:.3f}, max |lp| "
              f"{np.abs(want[np.isfinite(want)]).max():.3e}")
        assert ok and ratio <= 1.0


def test_edge_cases_of_the_definition():
    one = np.ones((1, 1), np.float32)

    def lp(proj, x, pnm=10.0, m=one):
        a = np.float32([[[proj]]]), m, np.float32([[[x]]]), pnm
        return float(tw.twin_logp(*a)[0, 0, 0]), float(tw.reference_logp(*a)[0, 0, 0]), float(tw.twin_dlogp(*a)[0, 0, 0])
    assert lp(2.5, 0.0)[:2] == (-25.0, -25.0) and lp(2.5, 0.0)[2] == -10.0        # k = 0: -lam, gradient -mask pnm
    assert lp(0.0, 0.0)[:2] == (0.0, 0.0)                                         # lam = 0, k = 0
    got = lp(3.0, 0.0, m=np.zeros((1, 1), np.float32))                            # a masked-out angle
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.0
    assert lp(0.0, 0.7)[:2] == (-np.inf, -np.inf)                                 # lam = 0, k > 0
    assert np.isnan(lp(-1.0, 0.7)[0]) and np.isnan(lp(-1.0, 0.7)[1])              # lam < 0
    assert np.isnan(lp(-1.0, 0.0)[0]) and np.isnan(lp(-1.0, 0.0)[1])
    assert lp(1.0, -0.5)[:2] == (-np.inf, -np.inf)                                # k < 0: outside the support
    t, r, g = lp(0.37, 0.41)                                                      # non-integer k = 4.1, lam = 3.7
    assert abs(t - r) <= 2e-6 and abs(g - 10.0 * (4.1 - 3.7) / 3.7) <= 1e-4
    # the derivative against a float64 central difference of the reference
    h = 1e-4
    a = lambda p: tw.reference_logp(np.float64([[[p]]]).astype(np.float32), one, np.float32([[[1.25]]]), 10.0)[0, 0, 0]
    fd = (a(2.0 + h) - a(2.0 - h)) / (np.float64(np.float32(2.0 + h)) - np.float64(np.float32(2.0 - h)))
    assert abs(lp(2.0, 1.25)[2] - fd) <= 1e-3 * abs(fd)


def test_new_symbols_in_header_library_and_table():
    from ct_pvae_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ctpvae_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    macro = int(re.search(r"#define\s+CTPVAE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert _lib.load().ctpvae_abi_version() == _lib.ABI_VERSION == macro == 3400
    assert _lib.NOISE == {"gaussian": 0, "poisson": 1}
    assert re.search(r"#define\s+CTPVAE_NOISE_POISSON\s+1\b", open(HEADER).read())
    # the twins take exactly one argument more than the calls they extend
    assert len(_lib.SIGNATURES["ctpvae_rotate_fwd_compact_noise_f32"][1]) == len(_lib.SIGNATURES["ctpvae_rotate_fwd_compact_f32"][1]) + 1
    assert len(_lib.SIGNATURES["ctpvae_siddon_fwd_loglik_noise_f32"][1]) == len(_lib.SIGNATURES["ctpvae_siddon_fwd_loglik_f32"][1]) + 1


def test_entry_points_refuse_bad_arguments():
    from ct_pvae_amd import _lib
    lib = _lib.load()
    assert lib.ctpvae_poisson_loglik_fwd_f32(None, None, None, 1, 1, 1, None, None, None) == _lib.EINVAL
    assert lib.ctpvae_poisson_loglik_bwd_f32(None, None, None, None, 1, 1, 1, None, None, None) == _lib.EINVAL


def test_unknown_noise_and_trainable_pnm_raise():
    import ct_pvae_amd as cp
    x = torch.zeros((1, 8, 8, 1))
    m, y = torch.zeros((1, 4)), torch.zeros((1, 4, 12))
    for model in ("rotate", "siddon"):
        with pytest.raises(ValueError, match="noise must be"):
            cp.calculate_log_prob_M_given_R(x, m, y, 1.0, 1e-7, theta=np.zeros(4), noise="laplace", model=model)
        with pytest.raises(ValueError, match="is data"):
            cp.calculate_log_prob_M_given_R(x, m, y, torch.tensor(1.0, requires_grad=True), 1e-7, theta=np.zeros(4), noise="poisson",
                                            model=model)
    with pytest.raises(ValueError, match="is data"):
        cp.poisson_log_prob(torch.zeros((1, 4, 12)), m, y, torch.tensor(1.0, requires_grad=True))
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).noise == "gaussian" and tr.get_args(["--noise", "poisson"]).noise == "poisson"
    with pytest.raises(SystemExit):
        tr.get_args(["--noise", "laplace"])


LIKELIHOOD_SOURCES = ("loglik.hip", "rotate_cplan.hip", "siddon.hip")


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    return hipcc


def test_no_likelihood_kernel_spills_registers():
    """hipcc's resource report over the sources that hold the new and the re-instantiated likelihood kernels: 0 scratch, and the
    Poisson instantiations are there."""
    csrc = os.path.join(ROOT, "ct_pvae_amd", "csrc")
    bad, names = [], []
    for src in LIKELIHOOD_SOURCES:
        out = subprocess.run([_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                             cwd=csrc, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        name = None
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                names.append(name)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and int(m.group(1)) > 0:
                bad.append((src, name, int(m.group(1))))
    assert not bad, f"kernels with scratch (register spills): {bad}"
    assert any("poisson_loglik_fwd_kernel" in n for n in names) and any("poisson_loglik_bwd_kernel" in n for n in names)
    # rotate_fwd_compact_kernel<NS, EPI = 3 | 4, SELM>: 2 x 2 x 3; siddon_fwd_poisson_kernel<USE_LDS, NS>: 3
    assert sum(bool(re.search(r"rotate_fwd_compact_kernelILi[12]ELi[34]ELi[012]E", n)) for n in set(names)) == 12
    assert sum("siddon_fwd_poisson_kernel" in n for n in set(names)) == 3


def test_no_device_trap_in_the_poisson_kernels():
    csrc = os.path.join(ROOT, "ct_pvae_amd", "csrc")
    pat = re.compile(r"poisson_loglik|rotate_fwd_compact_kernelILi[12]ELi[34]E|siddon_fwd_poisson_kernel")
    seen = 0
    for src in LIKELIHOOD_SOURCES:
        out = subprocess.run([_hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                              "--cuda-device-only", "-S", src, "-o", "-"], cwd=csrc, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        for m in re.finditer(r"^(_ZN6ctpvae\w+):(.*?)s_endpgm", out.stdout, re.S | re.M):
            if pat.search(m.group(1)):
                seen += 1
                assert "s_trap" not in m.group(2), m.group(1)
    assert seen == 2 + 12 + 3


# ---- the per-sample rule (tests/np_twin_poisson.py bar_logp / bar_dlogp) ------------------------------------------------------------
RULE_PNMS = (1.0, 1e2, 1e4, 1e6)
RULE_SHAPE = (5, 12, 184)
RULE_BIG = (3, 20, 9001)                    # the GPU test's launch past one grid
RULE_BIG_CASES = ((1.0, "near"), (1e2, "seam_k"), (1e4, "seam_u"), (1e6, "small_k"))      # one kind per pnm
RULE_SEED = 11
WHAT = ("logp", "dlogp")


def rule_excess(what, fn, a):
    want, bar = getattr(tw, "reference_" + what)(*a), getattr(tw, "bar_" + what)(*a)
    return tw.worst_excess_bar(fn(*a), want, bar)


def twin_within_the_bars(kind, shape, pnm):
    a = tw.operands(kind, shape, pnm, RULE_SEED) + (pnm,)
    r = {}
    for what in WHAT:
        r[what], same = rule_excess(what, getattr(tw, "twin_" + what), a)
        assert same, f"{kind} {what}: the twin's non-finite samples differ in kind from the reference's"
    print(f"[poisson] twin vs float64, {kind} pnm {pnm:g} {shape}: R lp {max(1.0, r['logp']):.2f} dlp {max(1.0, r['dlogp']):.2f} "
          f"(worst excess lp {r['logp']:.2f} dlp {r['dlogp']:.2f})")
    for what in WHAT:
        assert max(1.0, r[what]) <= tw.R_MAX, f"{kind} {what}: the twin misses its own bar by {r[what]:.2f} > R_MAX"
    # the exact zeros of the rule: a masked-out sample without counts
    m = np.broadcast_to(a[1][..., None], a[0].shape)
    zero = (m == 0) & (a[2] == 0)
    assert (tw.bar_logp(*a)[zero] == 0).all() and (tw.bar_dlogp(*a)[zero] == 0).all()
    assert (tw.twin_logp(*a)[zero] == 0).all() and (tw.twin_dlogp(*a)[zero] == 0).all()


@pytest.mark.parametrize("pnm", RULE_PNMS)
@pytest.mark.parametrize("kind", tw.KINDS)
def test_twin_within_the_bars_of_the_reference(kind, pnm):
    twin_within_the_bars(kind, RULE_SHAPE, pnm)


@pytest.mark.parametrize("pnm,kind", RULE_BIG_CASES)
def test_twin_within_the_bars_past_one_grid(pnm, kind):
    twin_within_the_bars(kind, RULE_BIG, pnm)


@pytest.mark.parametrize("shape", [(2, 3, 65), RULE_SHAPE, RULE_BIG], ids=lambda s: "x".join(map(str, s)))
def test_operands_are_what_they_say(shape):
    """Conditions, not measurements: each kind puts the stated share of its samples where its name says, in float32 as the twin (and
    the kernel) evaluates k, lam and u."""
    F = np.float32
    assert tw.KINDS == ("near", "far", "zero", "tiny", "seam_k", "seam_u", "small_k")
    for pnm in RULE_PNMS:
        def klu(kind):
            proj, mask, x = tw.operands(kind, shape, pnm, RULE_SEED)
            assert proj.dtype == mask.dtype == x.dtype == F and proj.shape == x.shape == shape and mask.shape == shape[:2]
            if kind in tw.SEAM_KINDS:
                assert set(np.unique(mask)) <= set(F(tw.MASKS[1:])) and (mask > 0).all()
            k, lam = x * F(pnm), (proj * mask[..., None]) * F(pnm)
            with np.errstate(all="ignore"):
                return k, lam, (lam - k) / k
        k, lam, u = klu("seam_k")
        assert (k < 8).mean() >= 0.4 and (k >= 8).mean() >= 0.4
        assert (np.abs(k.astype(np.float64) - 8.0) <= 1e-5 * 8.0).mean() >= 0.3
        assert k.reshape(-1)[0] == 8 and (k < 8).any() and (lam > 0).all()
        k, lam, u = klu("seam_u")
        assert (u < F(-0.5)).mean() >= 0.4 and (u >= F(-0.5)).mean() >= 0.4
        assert (np.abs(u.astype(np.float64) + 0.5) < 1e-5).mean() >= 0.3
        k, lam, u = klu("small_k")
        assert (k < 8).all() and (k > 0).all() and (k != np.round(k)).all()
        assert (u < F(-0.5)).mean() >= 0.25
    proj, mask, x = tw.operands("near", shape, 1.0, RULE_SEED)      # pnm 1: all three regimes of k in one launch
    k = x * F(1.0)
    assert (k == 0).mean() > 0.2 and ((k > 0) & (k < 8)).mean() > 0.2 and (k >= 8).mean() > 0.2
    for kind in tw.KINDS[:4]:               # delegated: the Gaussian file's operands, bit for bit
        for got, want in zip(tw.operands(kind, shape, 1e4, 3), tw.tg.operands(kind, shape, 1e4, 3)):
            np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        tw.operands("other", (1, 1, 1), 1e4, 0)


@pytest.mark.parametrize("pnm", RULE_PNMS)
def test_reference_dlogp_is_float64_autograd_of_reference_logp(pnm):
    """d / d proj of xlogy(k, lam) - lgamma(k + 1) - lam (reference_logp's formula; k == 0: -lam) by float64 torch autograd, on the
    samples with lam > 0.

    Autograd returns m pnm k / lam - m pnm, the reference m pnm (k - lam) / lam: two float64 evaluations of the same number whose
    operations each round a value no larger than m pnm (k / lam + 1) -- three on either side, so they differ by at most
    8 * 2^-53 * m pnm (k / lam + 1) per sample."""
    worst = 0.0
    for kind in tw.KINDS:
        proj, mask, x = tw.operands(kind, (4, 5, 8), pnm, seed=2)
        p = torch.from_numpy(proj.astype(np.float64)).requires_grad_(True)
        m = torch.from_numpy(mask.astype(np.float64))[..., None]
        k = torch.from_numpy(x.astype(np.float64)) * float(np.float32(pnm))
        lam = p * m * float(np.float32(pnm))
        lp = torch.where(k == 0, -lam, torch.xlogy(k, torch.where(k == 0, torch.ones_like(lam), lam)) - torch.lgamma(k + 1) - lam)
        on = (lam > 0).numpy()
        assert on.any()
        # the same formula (a check of the expression, not of float64: torch's and scipy's lgamma and log differ by a few ulp of
        # the three terms, 1e-16 relative -- any other formula differs by 1e-2 and more)
        kn, ln = k.numpy()[on], lam.detach().numpy()[on]
        terms = np.abs(kn * np.log(ln)) + np.abs(torch.lgamma(k + 1).numpy()[on]) + ln + 1.0
        assert (np.abs(lp.detach().numpy()[on] - tw.reference_logp(proj, mask, x, pnm)[on]) <= 1e-12 * terms).all()
        lp.sum().backward()
        got, want = tw.reference_dlogp(proj, mask, x, pnm)[on], p.grad.numpy()[on]
        assert np.isfinite(want).all()
        allowed = 8.0 * 2.0 ** -53 * np.broadcast_to(m.numpy() * float(np.float32(pnm)), on.shape)[on] * (kn / ln + 1.0)
        ratio = float((np.abs(got - want) / allowed).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{kind}: {ratio:.3f}"
    print(f"[poisson] reference_dlogp vs float64 autograd, pnm {pnm:g}: worst |difference| / allowed {worst:.3f}")


WRONG_TWINS = (("logp", "without_c2", tw.twin_logp_without_c2, "seam_k"), ("logp", "always_log1p", tw.twin_logp_always_log1p, "small_k"),
               ("dlogp", "without_mask", tw.twin_dlogp_without_mask, "near"), ("dlogp", "general_at_zero", tw.twin_dlogp_general_at_zero, "zero"))


@pytest.mark.parametrize("pnm", RULE_PNMS)
@pytest.mark.parametrize("what,name,fn,kind", WRONG_TWINS, ids=[w[1] for w in WRONG_TWINS])
def test_the_rule_refuses_wrong_twins(what, name, fn, kind, pnm):
    """Negative controls: each wrong twin exceeds MARGIN * R * bar on at least one sample of the kind named for it, or differs in
    kind there, while the correct twin passes on the same operands.  The series without its second term passes the older
    bar_from_twin rule on those operands -- which is why that rule is not enough."""
    a = tw.operands(kind, RULE_SHAPE, pnm, RULE_SEED) + (pnm,)
    want, bar = getattr(tw, "reference_" + what)(*a), getattr(tw, "bar_" + what)(*a)
    R = tw.twin_ratio(getattr(tw, "twin_" + what)(*a), want, bar)
    right, right_same = tw.worst_excess_bar(getattr(tw, "twin_" + what)(*a), want, bar)
    worst, same = tw.worst_excess_bar(fn(*a), want, bar)
    print(f"[poisson] negative control '{name}', {kind} pnm {pnm:g}: worst excess {worst:.3g}, same kinds {same}, against MARGIN R = "
          f"{tw.MARGIN * R:.1f}; the correct twin {right:.2f}")
    assert R <= tw.R_MAX and right_same and right <= tw.MARGIN * R
    assert worst > tw.MARGIN * R or not same, f"the rule accepts '{name}' on {kind}"
    if name == "without_c2":
        _, atol, rtol, _, _ = tw.bar_from_twin(*a)
        old, _, old_same = tw.worst_excess(fn(*a), want, atol, rtol)
        print(f"[poisson] negative control '{name}', {kind} pnm {pnm:g}: worst |err| / (atol + rtol |want|) under bar_from_twin {old:.2f}")
        assert old_same and old <= 1.0, "bar_from_twin was expected to pass the series without its second term"
