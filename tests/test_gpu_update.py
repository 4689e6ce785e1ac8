"""The update stage on the GPU (csrc/update.hip, ct_pvae_amd/update.py): the norms in their documented order, the five float32 lines bit
for bit against tests/np_twin_update.py over five consecutive steps, and the trainer's --fused_update."""
import math

import numpy as np
import pytest
import torch

from tests import np_twin_update as tw

pytestmark = pytest.mark.gpu

CLIP, LR, B1, B2, EPS = 100.0, 1e-3, 0.9, 0.999, 1e-7


def _dev():
    return torch.device("cuda", 0)


def _chunk():
    from ct_pvae_amd import update
    return update.chunk_len()


def _roles(C):
    """The tensor list (odd lengths, every length around a wave, a workgroup's quads and a chunk, one tensor of 70 chunks: launch 2 then
    fetches its partials in two rounds of 64) and what the gradient of each is drawn as."""
    lens = [1, 2, 3, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3, 70 * C - 5, 7]
    role = {2: "zero", 4: "zero", 6: "under", 8: "over", 11: "nan", 5: "inf", 12: "big", 13: "plain"}
    assert sum(lens) < 1_000_000
    return lens, role


def _gradient(lens, role, step):
    rng = np.random.default_rng(100 + step)
    parts = []
    for k, n in enumerate(lens):
        g = rng.standard_normal(n).astype(tw.F) * tw.F(10.0 ** rng.uniform(-3, 0))
        r = role.get(k)
        if r == "zero":
            g[:] = 0
        elif r in ("under", "over"):                      # l2 = clip (1 -+ 1e-4): far from clip in float32 ulps, near it as a case
            g = (g.astype(np.float64) * (CLIP * (0.9999 if r == "under" else 1.0001) / np.linalg.norm(g.astype(np.float64)))).astype(tw.F)
        elif r == "nan":
            g[::7] = np.nan
        elif r == "inf":
            g[n // 2] = np.inf if step % 2 else -np.inf
        elif r == "big":
            g *= tw.F(50.0)
        parts.append(g)
    return np.concatenate(parts)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _cat(params):
    return np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in params])


def _new_params(lens, seed, dev, shift=1):
    """Parameters as views of one allocation, `shift` elements in: their addresses take every 4-byte alignment."""
    values = (0.1 * np.random.default_rng(seed).standard_normal(sum(lens))).astype(tw.F)
    store = torch.from_numpy(np.concatenate([np.zeros(shift, tw.F), values])).to(dev)
    return list(store[shift:].split(lens)), store


def _check_step(fu, params, lens, g_host, flat, state, C):
    """One device step against the twin; `state` = (p, m, v) of the twin before the step, returned after it."""
    g_bits = _bits(flat)
    fu.step(flat)
    norms = fu.norms.cpu().numpy()
    assert tw.same_bits(norms, tw.tensor_norms(g_host, lens, C))                      # the documented order, bit for bit
    off = 0
    for k, n in enumerate(lens):                                                      # and the sum itself: one float32 ulp of the exact one
        g0 = np.where(np.isnan(g_host[off:off + n]), 0, g_host[off:off + n]).astype(np.float64)
        exact = math.sqrt(math.fsum((g0 * g0).tolist())) if np.isfinite(g0).all() else math.inf
        if math.isinf(exact):
            assert np.isposinf(norms[k])
        else:
            assert abs(float(norms[k]) - exact) <= float(np.spacing(tw.F(exact))), (k, norms[k], exact)
        off += n
    alpha = tw.adam_alpha(fu.t, LR, B1, B2)
    p, m, v = tw.twin_update(g_host, np.repeat(norms, lens), *state, alpha, CLIP, B1, B2, EPS)
    for name, want, got in (("p", p, _cat(params)), ("m", m, fu.m.cpu().numpy()), ("v", v, fu.v.cpu().numpy())):
        assert tw.same_bits(got, want), (name, fu.t, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.array_equal(_bits(flat), g_bits)                                        # the gradient buffer is read only
    return p, m, v


def test_five_steps_bit_for_bit_against_the_twin():
    from ct_pvae_amd import FusedUpdate
    dev, C = _dev(), _chunk()
    lens, role = _roles(C)
    params, _ = _new_params(lens, 1, dev)
    fu = FusedUpdate(params, lr=LR, beta1=B1, beta2=B2, eps=EPS, clip_norm=CLIP)
    state = (_cat(params), np.zeros(sum(lens), tw.F), np.zeros(sum(lens), tw.F))
    for step in range(1, 6):
        g_host = _gradient(lens, role, step)
        state = _check_step(fu, params, lens, g_host, torch.from_numpy(g_host).to(dev), state, C)
        norms = fu.norms.cpu().numpy()
        assert norms[2] == 0 and norms[4] == 0 and norms[6] < CLIP < norms[8] and np.isposinf(norms[5]) and np.isfinite(norms[11])
        assert fu.t == step
    assert np.isnan(state[0]).sum() == 1 and np.isfinite(state[0]).sum() == sum(lens) - 1     # the inf's own element, nothing else


def test_three_hundred_tensors_of_one_element():
    from ct_pvae_amd import FusedUpdate
    dev, C = _dev(), _chunk()
    lens = [1] * 300
    params = [torch.full((1,), 0.01 * k, device=dev) for k in range(300)]
    fu = FusedUpdate(params, lr=LR, beta1=B1, beta2=B2, eps=EPS, clip_norm=CLIP)
    state = (_cat(params), np.zeros(300, tw.F), np.zeros(300, tw.F))
    for step in (1, 2):
        g_host = (np.random.default_rng(step).standard_normal(300) * 200).astype(tw.F)
        g_host[::50] = np.nan
        g_host[7] = 0
        state = _check_step(fu, params, lens, g_host, torch.from_numpy(g_host).to(dev), state, C)
    assert tw.same_bits(fu.norms.cpu().numpy(), np.abs(np.where(np.isnan(g_host), 0, g_host)))


def test_identical_calls_give_identical_bits_at_any_alignment():
    """Two runs from equal states give equal bits -- also when the parameters and the gradient buffer sit at other 4-byte alignments
    (the 16-byte accesses are a matter of speed, not of values)."""
    from ct_pvae_amd import FusedUpdate
    dev, C = _dev(), _chunk()
    lens, role = _roles(C)
    out = []
    for shift in (1, 1, 0, 2):
        params, _ = _new_params(lens, 1, dev, shift=shift)
        if shift == 0:
            params = [p.clone() for p in params]                                    # every parameter an allocation of its own: all aligned
        fu = FusedUpdate(params, lr=LR, beta1=B1, beta2=B2, eps=EPS, clip_norm=CLIP)
        for step in (1, 2):
            g = torch.from_numpy(np.concatenate([np.zeros(shift, tw.F), _gradient(lens, role, step)])).to(dev)
            fu.step(g[shift:])
        out.append((_cat(params).view(np.uint32), _bits(fu.m), _bits(fu.v), _bits(fu.norms)))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


def test_a_reallocated_parameter_is_picked_up():
    from ct_pvae_amd import FusedUpdate
    dev, C = _dev(), _chunk()
    lens = [5, C + 1, 3]
    params = [torch.nn.Parameter(torch.from_numpy((0.1 * np.random.default_rng(k).standard_normal(n)).astype(tw.F)).to(dev))
              for k, n in enumerate(lens)]
    fu = FusedUpdate(params, lr=LR, beta1=B1, beta2=B2, eps=EPS, clip_norm=CLIP)
    state = (_cat(params), np.zeros(sum(lens), tw.F), np.zeros(sum(lens), tw.F))
    g_host = np.random.default_rng(9).standard_normal(sum(lens)).astype(tw.F)
    flat = torch.from_numpy(g_host).to(dev)
    state = _check_step(fu, params, lens, g_host, flat, state, C)
    old = params[1].data
    params[1].data = old.clone()                                                    # the parameter's memory moves
    assert params[1].data_ptr() != old.data_ptr()
    kept = _bits(old)
    _check_step(fu, params, lens, g_host, flat, state, C)                            # ... and the update follows it
    assert np.array_equal(_bits(old), kept)                                          # the memory it left is not written any more
    with pytest.raises(ValueError):
        fu.step(flat[:-1])
    with pytest.raises(ValueError):
        fu.step(flat.cpu())


# ---- the trainer's --fused_update ---------------------------------------------------------------------------------------------
RECIPE = "--nsa 10 --td 6 -b 3 --ns 1 --api 10 --pnm 1e4 --normal -i 3 --n_pixel 64 --num_angles 60 --train"


def _trainer(flags=""):
    from ct_pvae_amd import trainer as tr
    return tr.PVAETrainer(tr.get_args((RECIPE + " " + flags).split()), _dev())


def test_trainer_step_is_the_twin_on_the_bucket():
    t = _trainer("--fused_update")
    assert math.isfinite(t.train_step())                                            # (builds the FusedUpdate: step 1 from zero moments)
    fu, C = t.upd, _chunk()
    assert fu is not None and fu.t == 1 and fu.same_params(t.params) and (fu.lr, fu.eps, fu.clip_norm) == (1e-4, 1e-7, 100.0)
    assert all(p.grad is None or p.grad.data_ptr() != v.data_ptr() for p, v in zip(t.params, t._bucket.shaped))
    before = (_cat(fu.params), fu.m.cpu().numpy(), fu.v.cpu().numpy())
    assert math.isfinite(t.train_step())
    g_host = t._bucket.flat.cpu().numpy()
    norms = fu.norms.cpu().numpy()
    assert fu.t == 2 and tw.same_bits(norms, tw.tensor_norms(g_host, fu.numels, C))
    p, m, v = tw.twin_update(g_host, np.repeat(norms, fu.numels), *before, tw.adam_alpha(2, 1e-4, 0.9, 0.999), 100.0, 0.9, 0.999, 1e-7)
    assert tw.same_bits(_cat(fu.params), p) and tw.same_bits(fu.m.cpu().numpy(), m) and tw.same_bits(fu.v.cpu().numpy(), v)
    assert not np.array_equal(p, before[0]) and t.opt.state_dict()["state"] == {}    # the nets moved; torch's Adam took no step


def test_trainer_runs_with_equal_seeds_are_bit_equal():
    flags = "--fused_head --fused_latents --reproducible --fused_update"
    runs = []
    for _ in range(2):
        t = _trainer(flags)
        losses = [t.train_step() for _ in range(3)]
        runs.append((losses, _cat(t.params).view(np.uint32), _bits(t.upd.m), _bits(t.upd.v)))
    assert runs[0][0] == runs[1][0] and all(math.isfinite(x) for x in runs[0][0])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert np.array_equal(a, b)


def test_checkpoints_cross_the_flag_both_ways(tmp_path):
    with_flag, without = _trainer("--fused_update"), _trainer()
    for t in (with_flag, without):
        t.train_step(), t.train_step()
    a, b = str(tmp_path / "a" / "ckpt-1.pt"), str(tmp_path / "b" / "ckpt-1.pt")
    with_flag.save(a, [0.0, 0.0])
    without.save(b, [0.0, 0.0])
    # written with the flag, restored without it
    plain = _trainer()
    plain.restore(a)
    st = plain.opt.state_dict()["state"]
    assert plain.iter == 2 and len(st) == len(with_flag.upd.params) == len(plain.params)
    for k, (m, v) in enumerate(zip(with_flag.upd.m.split(with_flag.upd.numels), with_flag.upd.v.split(with_flag.upd.numels))):
        assert torch.equal(st[k]["exp_avg"].reshape(-1), m) and torch.equal(st[k]["exp_avg_sq"].reshape(-1), v)
        assert float(st[k]["step"]) == 2.0
    assert all(torch.equal(p, q) for p, q in zip(plain.params, with_flag.params))
    assert math.isfinite(plain.train_step()) and float(plain.opt.state_dict()["state"][0]["step"]) == 3.0
    # written without the flag, restored with it
    fused = _trainer("--fused_update")
    fused.restore(b)
    st = without.opt.state_dict()["state"]
    assert fused.iter == 2 and fused.upd is not None and fused.upd.t == 2 and fused.upd.same_params(fused.params)
    for k, (m, v) in enumerate(zip(fused.upd.m.split(fused.upd.numels), fused.upd.v.split(fused.upd.numels))):
        assert torch.equal(st[k]["exp_avg"].reshape(-1), m) and torch.equal(st[k]["exp_avg_sq"].reshape(-1), v)
    assert math.isfinite(fused.train_step()) and fused.upd.t == 3 and fused.upd.same_params(fused.params)


def test_train_pnm_is_one_more_tensor_of_length_one():
    # (--lr 0.5: an Adam step is about lr whatever the gradient's size, and float32 pnm = 1e4 has an ulp of 1e-3 -- the default 1e-4 cannot
    # move it under any Adam)
    t = _trainer("--fused_update --train_pnm --lr 0.5")
    before = float(t.pnm.detach())
    assert math.isfinite(t.train_step())
    assert t.upd.params[-1] is t.pnm and t.upd.numels[-1] == 1 and len(t.upd.params) == len(t.params) + 1
    after = float(t.pnm.detach())
    assert after != before and math.isfinite(after) and abs(after - before) <= 0.5 * 1.01
