"""noise="poisson" on a real MI355X: the exact Poisson log-probability, elementwise and fused into both projectors' training calls.

Acceptance: for EVERY sample |got - want| <= atol + rtol |want|, want = the float64 reference (tests/np_twin_poisson.py: TFP's
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
from ct_pvae_amd import phantoms
from tests import np_twin_poisson as tw

pytestmark = pytest.mark.gpu
PNMS = [1.0, 1e2, 1e4]
EPS = 1.2e-7


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
