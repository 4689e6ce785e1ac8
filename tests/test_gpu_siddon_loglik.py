"""calculate_log_prob_M_given_R(model="siddon") on a real MI355X: the likelihood training call on the ray-driven projector,
against the CPU oracle (given the same host theta) and against the two-step GPU path it fuses.

Bars: ray-sums bit-equal (same fp32 expressions, correctly rounded / and sqrt); log-probabilities within 1e-5 (max-norm
relative, the project's bar -- the remainder is the device's logf) of the oracle AND bit-equal to the two-step path (the same
functions of loglik_math.h in the same order); gradients within 1e-5 of the largest entry (the per-slice factor multiplies
after the sum over angles instead of before it); d / d pnm within 1e-4 relative (its reduction uses atomics: no fixed order)."""
import numpy as np
import pytest
import torch

import ct_pvae_amd as cp
from ct_pvae_amd import _lib, phantoms
from ct_pvae_amd import helper_functions as hf

pytestmark = pytest.mark.gpu

REL = 1e-5
PNM, EPS = 1e4, 1.2e-7


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def to_np(t):
    return t.detach().cpu().numpy()


def operands(B, shape, A_all, pad, seed, foam=True):
    """Images, a dense theta, dense mask / measurements on the host (float32)."""
    rng = np.random.default_rng(seed)
    if foam and shape == (128, 128):
        img = phantoms.foam_batch(B, 128, seed=seed, supersample=2)
    else:
        img = rng.random((B,) + shape, dtype=np.float32)
    theta = phantoms.dense_theta(A_all) if A_all >= 20 else rng.uniform(0.0, np.pi, A_all)
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    dx = _lib.load().ctpvae_siddon_dx(shape[0], shape[1], 1 if pad else 0)
    mask = rng.uniform(0.02, 0.08, (B, A_all)).astype(np.float32)
    meas = (rng.random((B, A_all, dx), dtype=np.float32) * np.float32(0.05 * 0.5 * max(shape)))
    return img, theta, mask, meas, dx


def raw_forward(img, theta, mask, meas, pad, sub=None, want_sino=True, want_dlp=True):
    """The ONE forward launch, with the ray-sums requested: (sino, lp, dlp) device tensors [B][rows][dx]."""
    d = dev()
    x = torch.from_numpy(img).to(d)
    st = hf._siddon_loglik_state(theta, x.shape[0], x.shape[1], x.shape[2], pad, d)
    sel = st.sel(sub) if sub is not None else None
    pnm = torch.tensor(PNM, dtype=torch.float32, device=d)
    return hf._siddon_loglik_forward(st, x, torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), pnm, EPS, sel,
                                     want_sino=want_sino, want_dlp=want_dlp)


def check_forward(oracle, img, theta, mask, meas, pad, sub):
    """ray-sums == oracle; lp within REL of the oracle and bit-equal to the two-step GPU path; returns lp (device)."""
    d = dev()
    th_sub = theta if sub is None else theta[np.asarray(sub)]
    m_sub = mask if sub is None else mask[:, np.asarray(sub)]
    x_sub = meas if sub is None else meas[:, np.asarray(sub)]
    sino, lp, dlp = raw_forward(img, theta, mask, meas, pad, sub)
    want_sino = np.swapaxes(oracle.siddon_project(img, th_sub, pad=pad), 0, 1)
    np.testing.assert_array_equal(to_np(sino), want_sino)
    want_lp = oracle.loglik(want_sino, m_sub, x_sub, PNM, EPS)
    err = rel_err(to_np(lp), want_lp)
    print(f"lp rel err vs oracle {err:.3e} (B={img.shape[0]} grid={img.shape[1:]} rows={len(th_sub)})")
    assert err <= REL
    assert torch.isfinite(dlp).all()
    # the public call: no ray-sums stored, same log-probabilities; and the two-step path's bits
    xt = torch.from_numpy(img[..., None]).to(d)
    got = cp.calculate_log_prob_M_given_R(xt, torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d), PNM, EPS, theta=theta,
                                          angles_i=sub, pad=pad, model="siddon")
    assert tuple(got.shape) == (img.shape[0], len(th_sub), want_sino.shape[2], 1)
    assert torch.equal(got[..., 0], lp)
    proj = cp.project_tf_fast(xt, th_sub, pad=pad, dim=2, integrate_vae=True, model="siddon")
    two = cp.gaussian_poisson_log_prob(proj[..., 0], torch.from_numpy(m_sub).to(d), torch.from_numpy(x_sub).to(d), PNM, EPS)
    assert torch.equal(got[..., 0], two)
    return lp


@pytest.mark.parametrize("B", [1, 2, 3, 5, 50])
def test_forward_128_subset_and_full_list(oracle, B):
    img, theta, mask, meas, dx = operands(B, (128, 128), 180, True, seed=B)
    assert dx == 184
    sub = np.random.default_rng(100 + B).permutation(180)[:20]
    lp_sub = check_forward(oracle, img, theta, mask, meas, True, sub)
    # a subset call's rows are rows `sub` of the dense call's (rays are independent)
    _, lp_all, _ = raw_forward(img, theta, mask, meas, True, None, want_sino=False, want_dlp=False)
    assert torch.equal(lp_sub, lp_all[:, torch.from_numpy(sub).to(lp_all.device)])
    # all 20 of a 20-angle list
    th20 = np.ascontiguousarray(theta[sub])
    check_forward(oracle, img, th20, np.ascontiguousarray(mask[:, sub]), np.ascontiguousarray(meas[:, sub]), True, None)


@pytest.mark.parametrize("pad", [True, False])
def test_forward_ragged_small_grid(oracle, pad):
    img, theta, mask, meas, dx = operands(3, (33, 47), 7, pad, seed=7)
    theta[:2] = [0.0, np.pi / 2]          # rays along the grid lines: the degenerate rays' pass
    check_forward(oracle, img, theta, mask, meas, pad, None)
    check_forward(oracle, img, theta, mask, meas, pad, [6, 0, 0, 3, 1])


def test_forward_grid_whose_pair_does_not_fit_lds(oracle):
    img, theta, mask, meas, dx = operands(5, (184, 184), 11, True, seed=11)
    check_forward(oracle, img, theta, mask, meas, True, None)
    check_forward(oracle, img, theta, mask, meas, True, [10, 2, 7])


@pytest.mark.parametrize("ns", [1, 2, 4, 8])
def test_every_forward_form_gives_the_same_bits(oracle, ns):
    """SIDDON_NS steers the dispatch as for create_sinograms: one slice / a slice pair per workgroup in LDS, 4 / 8 slices per walk."""
    img, theta, mask, meas, dx = operands(5, (128, 128), 180, True, seed=5)
    sub = [3, 170, 44, 44, 91, 0, 179]
    _, want, want_d = raw_forward(img, theta, mask, meas, True, sub, want_sino=False)
    with _lib.tuned("SIDDON_NS", ns):
        lp = check_forward(oracle, img, theta, mask, meas, True, sub)
        _, _, dlp = raw_forward(img, theta, mask, meas, True, sub, want_sino=False)
    assert torch.equal(lp, want) and torch.equal(dlp, want_d)
    small = operands(3, (33, 47), 7, True, seed=9)
    with _lib.tuned("SIDDON_NS", ns):
        check_forward(oracle, *small[:4], True, [5, 1, 6])


def test_angle_index_forms_and_range_check():
    d = dev()
    img, theta, mask, meas, dx = operands(3, (128, 128), 180, True, seed=3)
    x, m, y = torch.from_numpy(img[..., None]).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    sub = np.array([7, 7, 150, 2, 99, 0], dtype=np.int64)

    def call(ai):
        return cp.calculate_log_prob_M_given_R(x, m, y, PNM, EPS, theta=theta, angles_i=ai, pad=True, model="siddon")
    want = call(sub)
    for ai in (list(sub), torch.from_numpy(sub), torch.from_numpy(sub.astype(np.int32)).to(d), torch.from_numpy(sub).to(d)):
        assert torch.equal(call(ai), want)
    for bad in ([0, 180], [-1, 3]):
        with pytest.raises(ValueError, match="outside"):
            call(bad)
    # a device-resident index cannot be read without a synchronisation: the kernels clamp it into the table
    assert torch.equal(call(torch.tensor([500, -4], dtype=torch.int32, device=d)), call([179, 0]))
    with pytest.raises(ValueError):
        cp.calculate_log_prob_M_given_R(x, m[:, :20], y, PNM, EPS, theta=theta, pad=True, model="siddon")


@pytest.mark.parametrize("B", [1, 5, 50])
def test_per_object_sums(oracle, B):
    d = dev()
    img, theta, mask, meas, dx = operands(B, (128, 128), 180, True, seed=20 + B)
    sub = np.random.default_rng(B).permutation(180)[:20]
    x, m, y = torch.from_numpy(img[..., None]).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    lp = cp.calculate_log_prob_M_given_R(x, m, y, PNM, EPS, theta=theta, angles_i=sub, pad=True, model="siddon")
    sums = cp.calculate_log_prob_M_given_R(x, m, y, PNM, EPS, theta=theta, angles_i=sub, pad=True, model="siddon", reduce="per_object")
    assert tuple(sums.shape) == (B,)
    np.testing.assert_array_equal(to_np(sums), oracle.loglik_object_sums(to_np(lp)[..., 0], 0))


def fused_grad(x, m, y, theta, sub, pad, upstream, reduce=None, pnm=PNM):
    xr = x.detach().clone().requires_grad_(True)
    out = cp.calculate_log_prob_M_given_R(xr, m, y, pnm, EPS, theta=theta, angles_i=sub, pad=pad, model="siddon", reduce=reduce)
    upstream(out).backward()
    return xr.grad


def two_step_grad(x, m, y, theta, sub, pad, upstream, pnm=PNM):
    xr = x.detach().clone().requires_grad_(True)
    idx = slice(None) if sub is None else torch.as_tensor(np.asarray(sub), device=x.device).long()
    th = theta if sub is None else theta[np.asarray(sub)]
    proj = cp.project_tf_fast(xr, th, pad=pad, dim=2, integrate_vae=True, model="siddon")
    lp = cp.gaussian_poisson_log_prob(proj[..., 0], m[:, idx].contiguous(), y[:, idx].contiguous(), pnm, EPS).unsqueeze(-1)
    upstream(lp).backward()
    return xr.grad


@pytest.mark.parametrize("B,shape,A_all,n_sub,pad", [(1, (128, 128), 180, 20, True), (5, (128, 128), 180, 20, True),
                                                    (50, (128, 128), 180, 20, True), (3, (33, 47), 7, 4, True),
                                                    (3, (33, 47), 7, 4, False), (5, (184, 184), 11, 3, True)])
def test_reconstruction_gradient(oracle, B, shape, A_all, n_sub, pad):
    d = dev()
    img, theta, mask, meas, dx = operands(B, shape, A_all, pad, seed=40 + B)
    if A_all < 20:
        theta[:2] = [0.0, np.pi / 2]
    rng = np.random.default_rng(B)
    sub = rng.permutation(A_all)[:n_sub]
    if A_all < 20:
        sub[0] = 0                       # an angle with degenerate rays
    x, m, y = torch.from_numpy(img[..., None]).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    w = torch.from_numpy(rng.uniform(0.5, 2.0, B).astype(np.float32)).to(d)
    e = torch.from_numpy(rng.standard_normal((B, n_sub, dx, 1)).astype(np.float32)).to(d)
    _, _, dlp = raw_forward(img, theta, mask, meas, pad, sub, want_sino=False)
    ups = {"per_object": (lambda lp: (lp.sum(dim=(1, 2, 3)) * w).sum(), w.view(B, 1, 1).expand(B, n_sub, dx)),
           "scalar": (lambda lp: lp.sum(), torch.ones((B, n_sub, dx), device=d)),
           "elementwise": (lambda lp: (lp * e).sum(), e[..., 0])}
    for name, (up, g) in ups.items():
        got = fused_grad(x, m, y, theta, sub, pad, up)
        assert tuple(got.shape) == tuple(x.shape) and torch.isfinite(got).all()
        two = two_step_grad(x, m, y, theta, sub, pad, up)
        e2 = float((got - two).abs().max() / two.abs().max())
        want = oracle.siddon_backproject(to_np(g * dlp), theta[sub], shape[0], shape[1])
        eo = rel_err(to_np(got)[..., 0], want)
        print(f"{name}: grad vs two-step {e2:.3e}, vs oracle transpose of upstream x dlp {eo:.3e} (B={B} grid={shape})")
        assert e2 <= REL and eo <= REL
        # the same call on theta[sub] with gathered operands: the same bits; and run to run
        gathered = fused_grad(x, m[:, torch.from_numpy(sub).to(d)].contiguous(), y[:, torch.from_numpy(sub).to(d)].contiguous(),
                              np.ascontiguousarray(theta[sub]), None, pad, up)
        assert torch.equal(got, gathered)
        assert torch.equal(got, fused_grad(x, m, y, theta, sub, pad, up))
    # reduce="per_object": the gradient bits of lp.sum(dim=(1, 2, 3)) under the same weights
    got = fused_grad(x, m, y, theta, sub, pad, lambda s: (s * w).sum(), reduce="per_object")
    assert torch.equal(got, fused_grad(x, m, y, theta, sub, pad, ups["per_object"][0]))
    # the dense list, no index operand
    got = fused_grad(x, m, y, theta, None, pad, ups["per_object"][0])
    two = two_step_grad(x, m, y, theta, None, pad, ups["per_object"][0])
    assert float((got - two).abs().max() / two.abs().max()) <= REL


@pytest.mark.parametrize("reduce", [None, "per_object"])
def test_trainable_pnm(reduce):
    d = dev()
    B = 5
    img, theta, mask, meas, dx = operands(B, (128, 128), 180, True, seed=60)
    sub = np.random.default_rng(6).permutation(180)[:20]
    x, m, y = torch.from_numpy(img[..., None]).to(d), torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    w = torch.linspace(0.5, 2.0, B, device=d)
    p1 = torch.tensor(PNM, device=d, requires_grad=True)
    p2 = torch.tensor(PNM, device=d, requires_grad=True)
    up = (lambda s: (s * w).sum()) if reduce else (lambda lp: (lp.sum(dim=(1, 2, 3)) * w).sum())
    got = fused_grad(x, m, y, theta, sub, True, up, reduce=reduce, pnm=p1)
    two = two_step_grad(x, m, y, theta, sub, True, lambda lp: (lp.sum(dim=(1, 2, 3)) * w).sum(), pnm=p2)
    ep = abs(float(p1.grad) - float(p2.grad)) / abs(float(p2.grad))
    print(f"d/d pnm fused {float(p1.grad):.6e} two-step {float(p2.grad):.6e} rel {ep:.3e}")
    assert np.isfinite(float(p1.grad)) and ep <= 1e-4
    assert float((got - two).abs().max() / two.abs().max()) <= REL


def test_adjointness_in_float64():
    """<A_sel x, g> = <x, A_sel^T g> at the training shape, products and sums in float64."""
    d = dev()
    B = 50
    img, theta, mask, meas, dx = operands(B, (128, 128), 180, True, seed=70)
    sub = np.random.default_rng(70).permutation(180)[:20]
    sino, _, _ = raw_forward(img, theta, mask, meas, True, sub, want_dlp=False)
    g = torch.from_numpy(np.random.default_rng(71).standard_normal((B, 20, dx)).astype(np.float32)).to(d)
    st = hf._siddon_loglik_state(theta, B, 128, 128, True, d)
    back = hf._siddon_backward_scaled(st, g, st.sel(sub))
    lhs = float((sino.double() * g.double()).sum())
    rhs = float((torch.from_numpy(img).to(d).double() * back.double()).sum())
    print(f"<A x, g> = {lhs:.10e}, <x, A^T g> = {rhs:.10e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    # the per-slice factor, read with a stride: stride 0 = one factor for the batch
    two = torch.tensor([2.0, 99.0], device=d)
    assert torch.equal(hf._siddon_backward_scaled(st, g, st.sel(sub), two, 0), 2.0 * back)


def test_forward_and_backward_replay_from_a_hip_graph():
    d = dev()
    B = 10
    img, theta, mask, meas, dx = operands(B, (128, 128), 180, True, seed=80)
    sub = np.random.default_rng(80).permutation(180)[:20]
    m, y = torch.from_numpy(mask).to(d), torch.from_numpy(meas).to(d)
    pnm = torch.tensor(PNM, device=d)
    w = torch.linspace(0.5, 2.0, B, device=d)
    x = torch.from_numpy(img[..., None]).to(d).requires_grad_(True)

    def step():
        with torch.autograd.set_multithreading_enabled(False):
            sums = cp.calculate_log_prob_M_given_R(x, m, y, pnm, EPS, theta=theta, angles_i=sub, pad=True, model="siddon",
                                                   reduce="per_object")
            gx, = torch.autograd.grad(sums, x, w)
        return sums, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # warm-up: tables, workspaces, the prepared transpose, the uploaded subset
        step()
    torch.cuda.synchronize()
    x2 = torch.rand_like(x)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sums_g, gx_g = step()
    with torch.no_grad():
        x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    got_s, got_g = sums_g.clone(), gx_g.clone()
    want_s, want_g = step()
    assert torch.equal(got_s, want_s) and torch.equal(got_g, want_g)


def test_trainer_on_the_ray_driven_model(monkeypatch):
    import math
    from ct_pvae_amd import trainer as tr
    args = tr.get_args("--nsa 20 --td 8 -b 3 --ns 2 --api 20 --pnm 1e4 --random --normal -i 3 --train --model siddon".split())
    t = tr.PVAETrainer(args, dev())
    seen = []
    real = tr.calculate_log_prob_M_given_R

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(([v.detach().clone() if isinstance(v, torch.Tensor) else v for v in a], dict(k), out.detach().clone()))
        return out
    monkeypatch.setattr(tr, "calculate_log_prob_M_given_R", spy)
    for _ in range(3):
        assert math.isfinite(t.train_step())
    assert len(seen) == 3
    for a, k, out in seen:
        assert k["model"] == "siddon" and k["reduce"] == "per_object" and tuple(out.shape) == (6,)
        direct = cp.calculate_log_prob_M_given_R(*a, theta=k["theta"], angles_i=k["angles_i"], pad=k["pad"], model="siddon",
                                                 reduce="per_object")
        assert torch.equal(direct, out)
