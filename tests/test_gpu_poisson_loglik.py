"""noise="poisson" on a real MI355X: the exact Poisson log-probability, elementwise and fused into both projectors' training calls.

Rule (the per-sample tests, second half of this file): for EVERY sample of lp and of d lp / d proj, |got - ref| <= MARGIN * R * bar --
ref the float64 reference of tests/np_twin_poisson.py, bar the first-order float32 error bar of that sample (bar_logp / bar_dlogp:
each term names the rounding it stands for), R >= 1 the float32 numpy twin's own worst excess on the same operands (against the
reference, never against the device; <= 16 by tests/test_poisson_loglik_cpu.py), MARGIN = 4.  No sample is left out; where the bar
is 0 (mask == 0 with k == 0; an upstream gradient of 0) the value is exactly 0; samples whose reference is not finite agree in kind
(NaN with NaN, the same infinity).  Every test prints n, the non-finite count, R, the worst excess and the allowance before it
asserts (run with -s).

    a  the elementwise kernels (poisson_log_prob and its backward, under a standard-normal upstream with one zero in ten): 7 operand
       kinds -- near / far / zero / tiny, and seam_k, seam_u, small_k aimed at the seams k = 8 (lgammaf | Stirling series) and
       u = -0.5 (logf(lam / k) | log1pf(u)) of csrc/loglik_math.h -- x pnm in {1, 1e2, 1e4, 1e6} x 3 shapes, and 540 060 elements
       -- past 2048 x 256, the second trip of both kernels' grid-stride loop and mask[k / P] beyond it -- for one kind per pnm
    b  edge samples in one launch: lam == 0 with and without counts, lam < 0, k < 0, k exactly 8 and the float below it, lam = k / 2
       exactly and the float below it, k = 1e7 with lam = k (1 +- 1e-4), each under the masks 1, 0.5, 1 / 180 and 0
    c  the lp / dlp planes the fused launches store, against the reference on the ray-sums the same launch returned: the compact
       plan (model="rotate"; all 180 angles and 20 of them, 5 foam objects of 128 x 128) and the ray-driven projector in each form
       its Poisson store has (0 global memory, 1 one slice in LDS, 2 a slice pair in LDS); measurements next to the rate on even
       angles, far from it on odd ones, whole angles masked out

Seen on the MI355X: no sample of any case outside the rule, no defect; R = 1 in every case, so the allowance is 4 bars throughout.
Worst |err| / bar -- elementwise lp 1.07 (seam_k, pnm 1e4), dlp 1.37 (tiny, pnm 1e2); past one grid lp 1.17, dlp 0.98; edge launch
lp 0.70, dlp 0.18, the -inf / +inf / NaN samples equal in kind; compact plan lp 0.76, dlp 0.72; ray-driven forms 0 / 1 / 2 lp 0.83,
dlp 0.73.  (A library built without the series' 1 / (360 k^3) term failed the rule in every one of these groups.)

The older acceptance (first half of this file, unchanged): for EVERY sample |got - want| <= atol + rtol |want|, want = the float64 reference (tests/np_twin_poisson.py: TFP's
formula with scipy's gammaln) on the oracle's ray-sums -- the nearest forward and the ray-driven forward equal the oracle bit for
bit (asserted), so the ray-sum is no source of difference.  atol and rtol are the float32 numpy twin's own error on the same
operands times 4 (np_twin_poisson.bar_from_twin): the kernel differs from the twin only in ocml's logf / log1pf / lgammaf, a few
ulp each against numpy's and scipy's.  Non-finite samples (-inf, NaN) must agree exactly.  Every figure is printed before it is
asserted (run with -s to read them).  Gradients: float64 torch autograd of the formula at 1e-4, the bar of the
Gaussian test."""
import math

import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib, phantoms
from ct_pvae_amd import helper_functions as hf
from tests import np_twin_poisson as tw

pytestmark = pytest.mark.gpu
PNMS = [1.0, 1e2, 1e4]
EPS = 1.2e-7
RULE_PNMS = (1.0, 1e2, 1e4, 1e6)
SHAPES = ((1, 1, 1), (2, 3, 65), (5, 12, 184))
BIG = (3, 20, 9001)                     # 540 060 elements > 2048 x 256
BIG_CASES = ((1.0, "near"), (1e2, "seam_k"), (1e4, "seam_u"), (1e6, "small_k"))       # one kind per pnm


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def assert_within_twin_bar(got, proj, mask, x, pnm, what):
    want, atol, rtol, e_abs, e_rel = tw.bar_from_twin(proj, mask, x, pnm)
    ratio, err, same = tw.worst_excess(got, want, atol, rtol)
    nonfinite = int((~np.isfinite(want)).sum())
    print(f"[poisson] {what} pnm {pnm:g}: n {want.size} non-finite {nonfinite} E_twin abs {e_abs:.3e} rel {e_rel:.3e} -> bar atol "
          f"{atol:.3e} rtol {rtol:.3e}; GPU max abs err {err:.3e}, worst |err| / bar {ratio:.3f}, median |lp| "
          f"{np.median(np.abs(want[np.isfinite(want)])):.2f}")
    assert same, f"{what}: -inf / NaN samples differ from the reference"
    assert ratio <= 1.0, f"{what}: a sample misses atol + rtol |want| by a factor {ratio:.2f}"
    return want


def autograd_f64(proj, mask, x, pnm, up):
    """d sum(up * lp) / d proj by float64 torch autograd of the formula (k = 0 samples: lp = -lam)."""
    p = torch.from_numpy(np.asarray(proj, np.float64)).requires_grad_(True)
    m = torch.from_numpy(np.asarray(mask, np.float64))[..., None]
    k = torch.from_numpy(np.asarray(x, np.float64)) * pnm
    lam = p * m * pnm
    lp = torch.where(k == 0, -lam, torch.xlogy(k, torch.where(k == 0, torch.ones_like(lam), lam)) - torch.lgamma(k + 1) - lam)
    (lp * torch.from_numpy(np.asarray(up, np.float64))).sum().backward()
    return p.grad.numpy()


def foam_sinograms(B, model, seed=0):
    """Foam phantoms and their dense 180-angle ray-sums from the CPU oracle; the device's equal them bit for bit."""
    from oracle import radon_oracle as orc
    orc.build()
    img = phantoms.foam_batch(B, 128, seed=seed, supersample=2)
    theta = np.ascontiguousarray(phantoms.dense_theta(180), dtype=np.float32)
    if model == "siddon":
        sino = np.ascontiguousarray(np.swapaxes(orc.siddon_project(img, theta, pad=True), 0, 1))
    else:
        sino = orc.project_tf_fast(img[..., None], theta, pad=True, integrate_vae=True)[..., 0]
    got = cp.project_tf_fast(torch.from_numpy(img[..., None]).to(dev()), theta, pad=True, dim=2, integrate_vae=True, model=model)
    np.testing.assert_array_equal(to_np(got)[..., 0], sino)
    return img, theta, sino


def sampled(sino, pnm, seed=3):
    """masks (20 of 180 angles, the rest masked out) and measurements from the library's own Poisson sampler."""
    mask, meas = cp.create_all_masks(x_train_sinograms=torch.from_numpy(sino).to(dev()), num_angles=sino.shape[1],
                                     poisson_noise_multiplier=pnm, num_sparse_angles=20, random=True, train=True, seed=seed)
    return to_np(mask), to_np(meas)


@pytest.mark.parametrize("pnm", PNMS)
@pytest.mark.parametrize("kind", ["sampled", "non_integer"])
def test_elementwise_forward_and_backward(pnm, kind):
    d = dev()
    _, _, sino = foam_sinograms(3, "rotate")
    rng = np.random.default_rng(int(pnm) + 7)
    if kind == "sampled":
        mask, meas = sampled(sino, pnm)
        assert (mask == 0).any() and (meas[mask == 0] == 0).all()       # masked angles are in
        # the reconstruction being scored is not the truth: a perturbed one
        proj = (sino * rng.uniform(0.8, 1.25, sino.shape)).astype(np.float32)
    else:
        mask = rng.uniform(0.02, 0.08, sino.shape[:2]).astype(np.float32)
        meas = (rng.random(sino.shape, dtype=np.float32) * np.float32(3.0))
        proj = sino
    pt = torch.from_numpy(proj).to(d).requires_grad_(True)
    lp = cp.poisson_log_prob(pt, torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), pnm)
    assert_within_twin_bar(to_np(lp), proj, mask, meas, pnm, f"elementwise {kind}")
    if kind == "sampled":                                               # the masked angles score exactly 0
        assert (to_np(lp)[mask == 0] == 0).all()
    # gradient, on the samples with a positive rate (lam = 0 with k = 0 has the one-sided derivative -mask pnm by definition)
    up = rng.standard_normal(sino.shape).astype(np.float32)
    (lp * torch.from_numpy(up).to(d)).sum().backward()
    got = to_np(pt.grad)
    want = autograd_f64(proj, mask, meas, pnm, up)
    ok = np.isfinite(want) & ((proj * mask[..., None]) > 0)
    err = float(np.abs(got[ok] - want[ok]).max() / np.abs(want[ok]).max())
    print(f"[poisson] elementwise {kind} pnm {pnm:g}: gradient rel err vs float64 autograd {err:.3e}")
    assert err <= 1e-4
    zero_rate = (proj * mask[..., None] == 0) & (meas == 0)
    np.testing.assert_array_equal(got[zero_rate], (-(mask[..., None] * np.float32(pnm)) * up)[zero_rate])
    # run to run
    lp2 = cp.poisson_log_prob(pt.detach(), torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), pnm)
    assert torch.equal(lp2, lp.detach())


def test_edge_cases_on_the_device():
    d = dev()
    proj = torch.tensor([[[2.5, 0.0, 0.0, -1.0, -1.0, 1.0, 3.0]]], device=d)
    meas = torch.tensor([[[0.0, 0.0, 0.7, 0.7, 0.0, -0.5, 0.0]]], device=d)
    lp = to_np(cp.poisson_log_prob(proj, torch.ones((1, 1), device=d), meas, 10.0))[0, 0]
    assert lp[0] == -25.0 and lp[1] == 0.0 and lp[2] == -np.inf and np.isnan(lp[3]) and np.isnan(lp[4]) and lp[5] == -np.inf
    assert lp[6] == -30.0
    masked = to_np(cp.poisson_log_prob(proj[..., :1], torch.zeros((1, 1), device=d), meas[..., :1], 10.0))
    assert masked[0, 0, 0] == 0.0


def fused_and_two_step(model, B, reduce, sub, pnm, x_np, theta, mask, meas, up_seed=5):
    """(value, gradient) of the public call and of the two-step path on gathered operands, elementwise upstream for reduce=None."""
    d = dev()
    outs = []
    mt, yt = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    idx = None if sub is None else torch.as_tensor(np.asarray(to_np(sub) if isinstance(sub, torch.Tensor) else sub)).long()
    rows = theta.size if idx is None else idx.numel()
    rng = np.random.default_rng(up_seed)
    up = torch.from_numpy(rng.standard_normal((B, rows, meas.shape[2], 1) if reduce is None else (B,)).astype(np.float32)).to(d)
    for fused in (True, False):
        x = torch.from_numpy(x_np[..., None]).to(d).requires_grad_(True)
        if fused:
            out = cp.calculate_log_prob_M_given_R(x, mt, yt, pnm, EPS, theta=theta, angles_i=sub, pad=True, reduce=reduce, model=model,
                                                  noise="poisson")
        else:
            th = theta if idx is None else theta[idx.numpy()]
            m2 = mt if idx is None else mt[:, idx.to(d)].contiguous()
            y2 = yt if idx is None else yt[:, idx.to(d)].contiguous()
            proj = cp.project_tf_fast(x, th, pad=True, dim=2, integrate_vae=True, model=model)
            out = cp.poisson_log_prob(proj[..., 0], m2, y2, pnm).unsqueeze(-1)
            lp_two = out.detach()
            if reduce == "per_object":
                out = out.sum(dim=(1, 2, 3))
        (out * up).sum().backward()
        outs.append((out.detach(), x.grad.detach()))
    return outs, lp_two


@pytest.mark.parametrize("model", ["rotate", "siddon"])
@pytest.mark.parametrize("angles", ["dense", "host", "device"])
def test_fused_equals_two_steps(oracle, model, angles):
    B, pnm = 5, 1e4
    img, theta, sino = foam_sinograms(B, model, seed=2)
    mask, meas = sampled(sino, pnm)
    host = np.random.default_rng(11).permutation(180)[:20].astype(np.int32)
    sub = {"dense": None, "host": host, "device": torch.from_numpy(host).to(dev())}[angles]
    if model == "rotate":       # this geometry takes the fused launch
        plan = cp.forward_functions._cached_plan(theta, 128, 128, True, dev(), "nearest", "tf_compat")
        assert plan.poisson_fused(None if sub is None else 20)
    # reduce=None, elementwise upstream: values and gradients bit for bit
    (f, t), lp_two = fused_and_two_step(model, B, None, sub, pnm, img, theta, mask, meas)
    assert torch.equal(f[0], t[0]) and torch.equal(f[1], t[1])
    sel = slice(None) if sub is None else host
    assert_within_twin_bar(to_np(f[0])[..., 0], sino[:, sel], mask[:, sel], meas[:, sel], pnm, f"fused {model} {angles}")
    # per-object sums: the library's fixed order over the two-step log-probabilities; the gradient has its factor applied after the
    # sum over angles instead of before (the Gaussian call's bar: 1e-5 of the largest entry)
    (f, t), lp_two = fused_and_two_step(model, B, "per_object", sub, pnm, img, theta, mask, meas)
    np.testing.assert_array_equal(to_np(f[0]), oracle.loglik_object_sums(to_np(lp_two)[..., 0], 0))
    gerr = float((f[1] - t[1]).abs().max() / t[1].abs().max())
    print(f"[poisson] fused {model} {angles}: per-object gradient vs two-step {gerr:.3e}")
    assert gerr <= 1e-5
    # run to run: no atomics on any Poisson path
    (f2, _), _ = fused_and_two_step(model, B, "per_object", sub, pnm, img, theta, mask, meas)
    assert torch.equal(f2[0], f[0]) and torch.equal(f2[1], f[1])


@pytest.mark.parametrize("case", ["tiled_384", "u16_plan", "few_angles"])
def test_fallback_geometries(oracle, case, monkeypatch):
    """Geometries without a fused Poisson epilogue take project_tf_fast -> poisson_log_prob -> the fixed-order sums."""
    d = dev()
    rng = np.random.default_rng(4)
    N, A, B = (384, 6, 2) if case == "tiled_384" else (128, 90, 3) if case == "u16_plan" else (128, 20, 3)
    theta = np.ascontiguousarray(np.linspace(0, np.pi, A, endpoint=False), dtype=np.float32)
    if case == "u16_plan":      # a plan forced to the u16 format in the cache the public call reads
        from ct_pvae_amd import forward_functions as ff
        real = ff.RotatePlan

        def forced(*a, **k):
            k["plan_format"] = "u16"
            return real(*a, **k)
        monkeypatch.setattr(ff, "RotatePlan", forced)
        theta = theta + np.float32(1e-3)      # a fresh cache entry
    img = rng.random((B, N, N), dtype=np.float32)
    sino = oracle.project_tf_fast(img[..., None], theta, pad=True, integrate_vae=True)[..., 0]
    pnm = 1e2
    mask, meas = sampled(sino, pnm)
    plan = cp.forward_functions._cached_plan(theta, N, N, True, d, "nearest", "tf_compat")
    assert not plan.poisson_fused(None)
    assert plan.tiled == (case == "tiled_384")
    with pytest.raises(ValueError, match="poisson"):
        plan.forward_loglik(torch.from_numpy(img).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d),
                            torch.tensor(pnm, device=d), EPS, noise="poisson")
    x = torch.from_numpy(img[..., None]).to(d).requires_grad_(True)
    lp = cp.calculate_log_prob_M_given_R(x, torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), pnm, EPS, theta=theta, pad=True,
                                         noise="poisson")
    assert_within_twin_bar(to_np(lp)[..., 0], sino, mask, meas, pnm, f"fallback {case}")
    sums = cp.calculate_log_prob_M_given_R(x, torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), pnm, EPS, theta=theta,
                                           pad=True, noise="poisson", reduce="per_object")
    np.testing.assert_array_equal(to_np(sums), oracle.loglik_object_sums(to_np(lp)[..., 0], 1 if case == "tiled_384" else 0))
    sums.sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


def test_the_references_toy():
    """ctvae/toy_mcmc_v2_functions.py:41: O 2 x 2, pad=False, dim=2, theta = [0, pi / 2]; the ray-sums are [.4, .6] and [.7, .3]."""
    d = dev()
    O = np.float32([[0.1, 0.3], [0.6, 0.0]])
    theta = np.float32([0.0, np.pi / 2])
    x = torch.from_numpy(O[None, ..., None]).to(d).requires_grad_(True)
    proj = cp.project_tf_fast(x, theta, pad=False, dim=2, integrate_vae=True)
    rays = to_np(proj)[0, ..., 0]
    np.testing.assert_allclose(np.sort(rays.reshape(-1)), np.float32([0.3, 0.4, 0.6, 0.7]), rtol=1e-6)
    pnm = 10.0
    counts = np.float32([[[5.0, 2.0], [9.0, 0.0]]])                    # integer counts M * pnm
    mask = np.ones((1, 2), np.float32)
    lp = cp.calculate_log_prob_M_given_R(x, torch.from_numpy(mask).to(d), torch.from_numpy(counts / np.float32(pnm)).to(d), pnm, EPS,
                                         theta=theta, pad=False, noise="poisson")
    assert_within_twin_bar(to_np(lp)[..., 0], rays[None], mask, counts / np.float32(pnm), pnm, "toy")
    lam = np.float64(rays[None]) * pnm
    want = counts * np.log(lam) - np.vectorize(math.lgamma)(counts + 1.0) - lam
    np.testing.assert_allclose(to_np(lp)[..., 0], want, rtol=0, atol=5e-6)
    lp.sum().backward()
    # d / d O of sum lp: every pixel lies on one ray per angle; d lp / d ray = pnm (k - lam) / lam
    dray = pnm * (counts[0] - lam[0]) / lam[0]
    # (which ray each pixel feeds is read off the projector's own transpose)
    inc = []
    for a in range(2):
        for j in range(2):
            e = torch.zeros((1, 2, 2, 1), device=d)
            e[0, a, j, 0] = 1.0
            inc.append(to_np(torch.autograd.grad(proj, x, e, retain_graph=True)[0])[0, ..., 0])
    want_g = sum(w * np.float64(i) for w, i in zip(dray.reshape(-1), inc))
    np.testing.assert_allclose(to_np(x.grad)[0, ..., 0], want_g, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("model", ["rotate", "siddon"])
def test_trainer_step_with_poisson_noise(model, monkeypatch):
    from ct_pvae_amd import trainer as tr
    args = tr.get_args(f"--nsa 20 --td 8 -b 3 --ns 2 --api 20 --pnm 1e4 --random --normal -i 2 --train --model {model} --noise poisson".split())
    t = tr.PVAETrainer(args, dev())
    seen = []
    real = tr.calculate_log_prob_M_given_R

    def spy(*a, **k):
        out = real(*a, **k)
        g, = torch.autograd.grad(out.sum(), a[0], retain_graph=True)       # the reconstruction gradient the step back-propagates
        seen.append((k.get("noise"), bool(torch.isfinite(out).all()), bool(torch.isfinite(g).all()), float(g.abs().max())))
        return out
    monkeypatch.setattr(tr, "calculate_log_prob_M_given_R", spy)
    loss = t.train_step()
    assert math.isfinite(loss)
    assert len(seen) == 1 and seen[0][:3] == ("poisson", True, True) and seen[0][3] > 0
    assert all(torch.isfinite(p).all() for p in t.params)
    with pytest.raises(ValueError, match="train_pnm"):
        tr.PVAETrainer(tr.get_args(f"--nsa 20 --td 8 -b 3 --train --model {model} --noise poisson --train_pnm".split()), dev())


# ---- the per-sample rule: |got - ref| <= MARGIN * R * bar for every sample (tests/np_twin_poisson.py) -------------------------------
def held(what, got, a, tag, up=None):
    """The rule for one output plane.  what: logp / dlogp; a = (proj, mask, x, pnm) on the host; up: an upstream gradient that
    multiplies the reference and the bar.  Samples whose reference is not finite agree in kind; where the bar is 0 (mask == 0 with
    k == 0; a zero upstream) the value is exactly 0.  Returns the worst excess (in units of the bar)."""
    want, bar = getattr(tw, "reference_" + what)(*a), getattr(tw, "bar_" + what)(*a)
    R = tw.twin_ratio(getattr(tw, "twin_" + what)(*a), want, bar)
    if up is not None:
        with np.errstate(invalid="ignore"):
            want, bar = want * up.astype(np.float64), bar * np.abs(up.astype(np.float64))
    worst, same = tw.worst_excess_bar(got, want, bar)
    print(f"[poisson] {tag} {what}: n {want.size} non-finite {int((~np.isfinite(want)).sum())} R {R:.2f} worst |err| / bar {worst:.2f} "
          f"(allowed {tw.MARGIN * R:.2f})")
    assert same, f"{tag} {what}: non-finite samples differ in kind from the reference"
    exact = np.isfinite(want) & (bar == 0)
    assert (np.asarray(got)[exact] == 0).all(), f"{tag} {what}: a sample whose bar is 0 is not exactly 0"
    assert worst <= tw.MARGIN * R, f"{tag} {what}: a sample misses MARGIN R bar: {worst:.2f} > {tw.MARGIN * R:.2f}"
    return worst


def upstream(shape, seed):
    """standard normal, one value in ten exactly 0"""
    rng = np.random.default_rng(seed)
    up = rng.standard_normal(shape).astype(np.float32)
    up[rng.random(shape) < 0.1] = 0.0
    return up


def run_elementwise(kind, pnm, shape, seed):
    d = dev()
    proj, mask, x = tw.operands(kind, shape, pnm, seed)
    a = (proj, mask, x, pnm)
    tag = f"elementwise {kind} pnm {pnm:g} {shape}"
    up = upstream(shape, seed + 1)
    pt = torch.from_numpy(proj).to(d).requires_grad_(True)
    lp = cp.poisson_log_prob(pt, torch.from_numpy(mask).to(d), torch.from_numpy(x).to(d), pnm)
    (lp * torch.from_numpy(up).to(d)).sum().backward()
    torch.cuda.synchronize()
    held("logp", to_np(lp), a, tag)
    g = to_np(pt.grad)
    held("dlogp", g, a, tag, up=up)
    # the exact zeros, spelled out: a masked-out sample without counts scores 0 and pulls nothing; a zero upstream pulls nothing
    # (unless it meets an infinite derivative: 0 * inf is NaN on both sides, compared in kind above)
    masked = np.broadcast_to(mask[..., None] == 0, shape) & (x == 0)
    assert (to_np(lp)[masked] == 0).all() and (g[masked] == 0).all(), f"{tag}: a masked-out sample without counts is not exactly 0"
    quiet = (up == 0) & np.isfinite(tw.reference_dlogp(*a))
    assert (g[quiet] == 0).all(), f"{tag}: a gradient under a zero upstream is not exactly 0"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pnm", RULE_PNMS)
@pytest.mark.parametrize("kind", tw.KINDS)
def test_elementwise_kernels_per_sample(kind, pnm, shape):
    run_elementwise(kind, pnm, shape, seed=11)


@pytest.mark.parametrize("pnm,kind", BIG_CASES)
def test_elementwise_kernels_past_one_grid(pnm, kind):
    """540 060 elements: the second trip of the grid-stride loop of the forward and the backward kernel, and mask[k / P] past it
    (the arithmetic regimes are the small shapes' job: one kind per pnm here)."""
    assert BIG[0] * BIG[1] * BIG[2] > 2048 * 256
    run_elementwise(kind, pnm, BIG, seed=11)


def test_edge_samples_in_one_launch():
    """lam == 0 with counts (lp -inf, dlp +inf) and without; a negative rate (lp NaN, dlp finite) with and without counts; negative
    counts (lp -inf, dlp finite); k exactly 8 and the float below it (the two sides of kPoissonStirlingMin); lam = k / 2 exactly and
    the float below it (the two sides of u < -0.5); k = 1e7 with lam = k (1 +- 1e-4); an ordinary sample -- each under the masks 1,
    0.5, 1 / 180 and 0.  pnm = 4: products with it are exact, so the mask-1 row holds exactly the values named.  Nothing traps."""
    d = dev()
    pnm = 4.0
    F = np.float32
    below = lambda v: np.nextafter(F(v), F(0.0))
    pairs = [(0.0, 0.7), (0.0, 0.0), (-1.0, 0.7), (-1.0, 0.0), (1.0, -0.5), (1.5, 2.0), (1.5, below(2.0)), (1.0, 2.0), (below(1.0), 2.0),
             (F(2.5e6) * F(1.0 + 1e-4), 2.5e6), (F(2.5e6) * F(1.0 - 1e-4), 2.5e6), (3.0, 3.0)]
    proj = np.tile(F([p for p, _ in pairs]), (1, 4, 1))
    x = np.tile(F([v for _, v in pairs]), (1, 4, 1))
    mask = F([[1.0, 0.5, 1.0 / 180.0, 0.0]])
    a = (proj, mask, x, pnm)
    k, lam = x[0, 0] * F(pnm), proj[0, 0] * F(pnm)
    assert k[5] == 8 and k[6] == below(8.0) and lam[7] * 2 == k[7] and lam[8] == below(4.0) and k[9] == k[10] == 1e7
    lp_ref, dlp_ref = tw.reference_logp(*a), tw.reference_dlogp(*a)
    assert (lp_ref[0, :3, 0] == -np.inf).all() and (dlp_ref[0, :3, 0] == np.inf).all()
    assert (lp_ref[0, :, 1] == 0).all() and (dlp_ref[0, :, 1] == -(mask[0] * F(pnm))).all()
    assert np.isnan(lp_ref[0, :3, 2:4]).all() and np.isfinite(dlp_ref[0, :3, 2:4]).all()
    assert (lp_ref[0, :, 4] == -np.inf).all() and np.isfinite(dlp_ref[0, :3, 4]).all()
    assert np.isfinite(lp_ref[0, :3, 5:]).all() and np.isfinite(dlp_ref[0, :3, 5:]).all()
    pt = torch.from_numpy(proj).to(d).requires_grad_(True)
    lp = cp.poisson_log_prob(pt, torch.from_numpy(mask).to(d), torch.from_numpy(x).to(d), pnm)
    lp.sum().backward()
    torch.cuda.synchronize()                                                         # (a trap would surface here)
    held("logp", to_np(lp), a, "edge")
    held("dlogp", to_np(pt.grad), a, "edge")


# ---- the planes the fused launches store ------------------------------------------------------------------------------------------------
def masks_and_measurements(sino, pnm, seed):
    """mask [B][A] from the twin's non-zero values with whole rows of zeros; measurements next to the rate on even angles
    (Poisson(sino mask pnm) / pnm: `near`), far from it on odd ones (uniform in [0, 3): `far`)."""
    rng = np.random.default_rng(seed)
    B, A, P = sino.shape
    mask = rng.choice(np.float32(tw.MASKS[1:]), size=(B, A)).astype(np.float32)
    mask[:, ::3] = 0.0
    mask[0, :] = np.roll(mask[0, :], 1)
    loc = sino.astype(np.float64) * mask[..., None]
    meas = (rng.poisson(loc * pnm) / pnm).astype(np.float32)
    meas[:, 1::2] = (rng.random((B, A, P)) * 3.0).astype(np.float32)[:, 1::2]
    return mask, meas


def check_planes(tag, sino, lp, dlp, mask, meas, pnm):
    """lp and d lp / d ray-sum of a projector launch against the reference on the launch's own ray-sums."""
    assert torch.isfinite(sino).all()
    a = (to_np(sino), mask, meas, pnm)
    worst = held("logp", to_np(lp), a, tag), held("dlogp", to_np(dlp), a, tag)
    quiet = np.broadcast_to(mask[..., None] == 0, a[0].shape) & (meas == 0)
    assert quiet.any() and (to_np(lp)[quiet] == 0).all() and (to_np(dlp)[quiet] == 0).all(), f"{tag}: a masked-out sample is not exactly 0"
    return worst


@pytest.mark.parametrize("pnm", [1e2, 1e4])
@pytest.mark.parametrize("angles", ["dense", "subset"])
def test_planes_of_the_compact_plan_launch(angles, pnm):
    """model="rotate": the compact plan's Poisson epilogue, all 180 angles and 20 of them (any order, dense operands read at the plan
    angle), 5 foam objects of 128 x 128."""
    d = dev()
    B = 5
    theta = np.ascontiguousarray(phantoms.dense_theta(180), dtype=np.float32)
    plan = cp.forward_functions._cached_plan(theta, 128, 128, True, d, "nearest", "tf_compat")
    x = torch.from_numpy(phantoms.foam_batch(B, 128, seed=2, supersample=2)).to(d)
    dense = plan.forward(x)
    mask, meas = masks_and_measurements(to_np(dense), pnm, seed=int(pnm))
    pt = torch.tensor(pnm, dtype=torch.float32, device=d)
    mt, yt = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    if angles == "dense":
        assert plan.poisson_fused(None)
        sub = np.arange(180)
        sino, lp, dlp = plan.forward_loglik(x, mt, yt, pt, EPS, with_dlp=True, noise="poisson")
    else:
        assert plan.poisson_fused(20)
        sub = np.random.default_rng(11).permutation(180)[:20].astype(np.int32)
        assert (mask[:, sub] == 0).any() and (mask[:, sub] > 0).any() and (sub % 2 == 0).any() and (sub % 2 == 1).any()
        sino, lp, dlp = plan.forward_loglik(x, mt, yt, pt, EPS, with_dlp=True, angles_i=torch.from_numpy(sub).to(d), dense_inputs=True,
                                            noise="poisson")
    assert tuple(lp.shape) == tuple(dlp.shape) == (B, len(sub), plan.PW)
    assert torch.equal(sino, dense[:, torch.from_numpy(sub).to(d).long()])
    check_planes(f"compact plan {angles} pnm {pnm:g}", sino, lp, dlp, np.ascontiguousarray(mask[:, sub]), np.ascontiguousarray(meas[:, sub]), pnm)


# the ray-driven projector's Poisson store exists in three forms (csrc/siddon.hip siddon_fwd_poisson_kernel): 0 = the slice read from
# global memory (it does not fit LDS), 1 = one slice in LDS, 2 = a slice pair in LDS.  (form, grid, objects, SIDDON_NS or None)
SIDDON_CASES = ((0, (160, 258), 1, None), (1, (33, 47), 4, 1), (2, (33, 47), 4, 2))


@pytest.mark.parametrize("form,grid,B,ns", SIDDON_CASES, ids=[f"form{c[0]}" for c in SIDDON_CASES])
@pytest.mark.parametrize("pad", [True, False])
def test_planes_of_the_siddon_launch(pad, form, grid, B, ns):
    d = dev()
    A = 7 if form else 4
    rng = np.random.default_rng(7)
    img = rng.random((B,) + grid, dtype=np.float32)
    theta = np.ascontiguousarray(rng.uniform(0.0, np.pi, A), dtype=np.float32)
    theta[:2] = [0.0, np.pi / 2]                                    # rays along the grid lines
    x = torch.from_numpy(img).to(d)
    st = hf._siddon_loglik_state(theta, B, grid[0], grid[1], pad, d)
    dense = to_np(cp.project_tf_fast(x[..., None], theta, pad=pad, dim=2, integrate_vae=True, model="siddon"))[..., 0]
    for pnm in (1e2, 1e4):
        mask, meas = masks_and_measurements(dense, pnm, seed=form)
        pt = torch.tensor(pnm, dtype=torch.float32, device=d)
        mt, yt = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
        for sub in (None, [A - 1, 0, 0, 2, 1]):
            rows = np.arange(A) if sub is None else np.asarray(sub)
            try:
                if ns is not None:
                    _lib.tune("SIDDON_NS", ns)
                got_form = _lib.load().ctpvae_siddon_fwd_form(B, grid[0], grid[1], len(rows), st.dx, _lib.SIDDON_STORE["poisson"])
                sino, lp, dlp = hf._siddon_loglik_forward(st, x, mt, yt, pt, EPS, None if sub is None else st.sel(sub), want_sino=True,
                                                          want_dlp=True, noise=_lib.NOISE["poisson"])
            finally:
                _lib.tune("SIDDON_NS")
            assert got_form == form, (got_form, form)
            np.testing.assert_array_equal(to_np(sino), dense[:, rows])
            check_planes(f"siddon form {form} {grid} pad {pad} {'dense' if sub is None else 'subset'} pnm {pnm:g}", sino, lp, dlp,
                         np.ascontiguousarray(mask[:, rows]), np.ascontiguousarray(meas[:, rows]), pnm)
