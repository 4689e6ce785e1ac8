"""The fused Normal latent block on the device (ct_pvae_amd/latents.py, csrc/latent.hip) against the float64 composition of
tests/np_twin_latent.py fed the host's draws, under that file's per-sample rule |got - ref| <= 4 R bar; the fixed order of the
per-object sum; batches cut with first_object; the trainer with --fused_latents."""
import math
import types

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, forward_functions, latent_draws, latents, normal_latents
from ct_pvae_amd import trainer as tr
from tests import np_twin_latent as tl

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789
DRAW = 5
#          B  C  H   W   ns first_object level
SHAPES = {"3x1x5x7": (3, 1, 5, 7, 2, 0, 0),          # len 35: unaligned quads
          "2x4x16x16": (2, 4, 16, 16, 2, 0, 1),
          "5x3x11x3+3": (5, 3, 11, 3, 3, 3, 2),      # len 99
          "1x2x64x33": (1, 2, 64, 33, 1, 0, 3)}      # len 4224: threads take a second quad
_cases = {}


def _dev():
    return torch.device("cuda", 0)


def run_latent(loc, log_scale, ns, first_object, level, chw, g_z=None, g_KL=None, eps=None, draw=DRAW, seed=SEED, sqrt_reg=tl.EPS32):
    """The device's results as numpy arrays: z, eps [ns][B][len], KL [B], kl [B][len], g_loc, g_log_scale [B][len] (None without
    cotangents).  z and KL through the autograd function, kl_elem and eps_out through the entry point (whose z and KL must be the
    function's, bit for bit)."""
    B, length = loc.shape
    C, H, W = chw
    assert C * H * W == length
    dev = _dev()
    skip = torch.from_numpy(np.stack([loc, log_scale], axis=1)).to(dev).reshape(B, 2 * C, H, W).requires_grad_(True)
    ed = torch.from_numpy(np.ascontiguousarray(eps, np.float32)).to(dev).reshape(ns * B, C, H, W) if eps is not None else None
    z, KL = normal_latents(skip, ns=ns, seed=seed, draw=draw, level=level, first_object=first_object, sqrt_reg=sqrt_reg, _eps=ed)
    assert z.shape == (ns * B, C, H, W) and KL.shape == (B,) and z.dtype == KL.dtype == torch.float32
    z2 = forward_functions._new_output((ns * B, length), torch.float32, dev)
    KL2 = forward_functions._new_output((B,), torch.float32, dev)
    kl_elem = forward_functions._new_output((B, length), torch.float32, dev)
    eps_out = forward_functions._new_output((ns * B, length), torch.float32, dev)
    _lib.check(_lib.load().ctpvae_latent_fwd_f32(skip.data_ptr(), B, length, ns, sqrt_reg, first_object, seed, draw, level,
                                                 ed.data_ptr() if ed is not None else None, z2.data_ptr(), KL2.data_ptr(),
                                                 kl_elem.data_ptr(), eps_out.data_ptr(), forward_functions._stream_ptr()), "latent_fwd")
    assert torch.equal(z2.view(torch.int32), z.detach().reshape(ns * B, length).view(torch.int32)) and torch.equal(KL2.view(torch.int32), KL.detach().view(torch.int32))   # (bits: a NaN equals itself)
    out = dict(z=z.detach().reshape(ns, B, length).cpu().numpy(), KL=KL.detach().cpu().numpy(), kl=kl_elem.cpu().numpy(),
               eps=eps_out.reshape(ns, B, length).cpu().numpy(), g_loc=None, g_log_scale=None)
    if g_z is not None:
        loss = ((z.reshape(ns, B, length) * torch.from_numpy(g_z).to(dev)).sum() + (KL * torch.from_numpy(g_KL).to(dev)).sum())
        g, = torch.autograd.grad(loss, skip)
        g = g.reshape(B, 2, length).cpu().numpy()
        out["g_loc"], out["g_log_scale"] = g[:, 0], g[:, 1]
    return out


def device_case(shape, kind):
    """One (shape, range): the CPU reference (computed once, shared, left unchanged) and the device's results."""
    key = (shape, kind)
    if key not in _cases:
        B, C, H, W, ns, fo, level = SHAPES[shape]
        c = tl.case(kind, B, C * H * W, ns, SEED, first_object=fo, draw=DRAW, level=level)
        c["dev"] = run_latent(c["loc"], c["log_scale"], ns, fo, level, (C, H, W), c["g_z"], c["g_KL"])
        _cases[key] = c
    return _cases[key]


def assert_within_bars(tag, dev, c, quantities=tl.QUANTITIES):
    for k in quantities:
        worst = float(np.max(tl.excess(dev[k], c["want"][k], c["bar"][k])))
        print(f"{tag} {k}: worst |got - ref| / bar = {worst:.3f}, R = {c['R'][k]:.3f}")
        assert np.isfinite(dev[k]).all(), k                               # (also: no element left at its NaN poison)
        assert worst <= tl.MARGIN * c["R"][k], (k, worst, c["R"][k])


@pytest.mark.parametrize("kind", list(tl.RANGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_sample_within_its_bar_of_float64(shape, kind):
    """eps (the device's own draws, through eps_out), z, kl_elem and both halves of g_skip against the float64 composition fed the
    host's v."""
    B, C, H, W, ns, fo, level = SHAPES[shape]
    c = device_case(shape, kind)
    host = latent_draws(B, C * H * W, ns=ns, seed=SEED, draw=DRAW, level=level, first_object=fo)
    assert np.array_equal(host.view(np.uint32), c["v"].view(np.uint32))
    assert np.isfinite(c["dev"]["KL"]).all()
    assert_within_bars(f"{shape} {kind}", c["dev"], c)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_object_sum_follows_the_stated_order(shape):
    """KL[b] is the float32 sum of the device's own kl_elem in csrc/latent.hip's order, bit for bit, and the KL of that object called
    alone (another B, another alignment in memory, first_object + b)."""
    B, C, H, W, ns, fo, level = SHAPES[shape]
    c = device_case(shape, "wide")
    KL, kl = c["dev"]["KL"], c["dev"]["kl"]
    want = np.array([tl.ordered_sum(kl[b]) for b in range(B)], np.float32)
    assert np.array_equal(KL.view(np.uint32), want.view(np.uint32)), (KL, want)
    for b in range(B):
        alone = run_latent(c["loc"][b:b + 1], c["log_scale"][b:b + 1], ns, fo + b, level, (C, H, W))
        assert np.array_equal(alone["KL"].view(np.uint32), KL[b:b + 1].view(np.uint32))
        assert np.array_equal(alone["z"].view(np.uint32), c["dev"]["z"][:, b:b + 1].view(np.uint32))


def test_a_batch_cut_with_first_object_draws_what_the_whole_batch_draws():
    """B = 5, ns = 3 whole against b in [0, 2) and [2, 5) with first_object + 0 / + 2: z, KL and g_skip (for the sliced cotangents)
    are equal bit for bit -- the sample index is a counter word, not part of the object index.  len = 99: the parts sit at another
    alignment in memory than the whole batch's rows."""
    B, C, H, W, ns, fo, level = SHAPES["5x3x11x3+3"]
    c = device_case("5x3x11x3+3", "wide")
    whole = c["dev"]
    for lo, hi in ((0, 2), (2, 5)):
        part = run_latent(np.ascontiguousarray(c["loc"][lo:hi]), np.ascontiguousarray(c["log_scale"][lo:hi]), ns, fo + lo, level,
                          (C, H, W), np.ascontiguousarray(c["g_z"][:, lo:hi]), np.ascontiguousarray(c["g_KL"][lo:hi]))
        assert np.array_equal(part["z"].view(np.uint32), whole["z"][:, lo:hi].view(np.uint32))
        assert np.array_equal(part["KL"].view(np.uint32), whole["KL"][lo:hi].view(np.uint32))
        for k in ("g_loc", "g_log_scale", "eps", "kl"):
            assert np.array_equal(part[k].view(np.uint32), np.ascontiguousarray(whole[k][..., lo:hi, :]).view(np.uint32)), k
    again = run_latent(c["loc"], c["log_scale"], ns, fo, level, (C, H, W))
    assert np.array_equal(again["z"].view(np.uint32), whole["z"].view(np.uint32))
    other = run_latent(c["loc"], c["log_scale"], ns, fo, level, (C, H, W), draw=DRAW + 1)
    assert not np.array_equal(other["z"], whole["z"])


def test_injected_eps_and_extreme_operands():
    """Every combination of eps in {0, +-5.5}, log_scale in {-1e10, -30, 1, 1 + 2^-23, 50} and loc in {0, +-1e3} (45 elements, two
    samples, two objects): values and gradients within the bars and finite."""
    ls_v = np.array([-1e10, -30.0, 1.0, 1 + 2.0 ** -23, 50.0], np.float32)
    loc_v = np.array([0.0, 1e3, -1e3], np.float32)
    eps_v = np.array([0.0, 5.5, -5.5], np.float32)
    ls_g, loc_g, eps_g = (a.ravel() for a in np.meshgrid(ls_v, loc_v, eps_v, indexing="ij"))
    B, ns, length = 2, 2, 45
    loc, ls = np.tile(loc_g, (B, 1)), np.tile(ls_g, (B, 1))
    eps = np.stack([np.tile(eps_g, (B, 1)), np.tile(np.roll(eps_g, 1), (B, 1))]).astype(np.float32)
    c = tl.case(None, B, length, ns, 9, eps=eps, operands_=(loc, ls))
    for k, R in c["R"].items():
        assert R <= tl.R_MAX, (k, R)
    dev = run_latent(loc, ls, ns, 0, 0, (1, 5, 9), c["g_z"], c["g_KL"], eps=eps)
    assert np.array_equal(dev["eps"], eps)
    assert np.isfinite(dev["KL"]).all()
    assert_within_bars("extremes", dev, c)


def test_a_nan_operand_stays_in_its_own_element_and_its_objects_sum():
    B, ns, C, H, W = 3, 2, 1, 5, 7
    loc, ls = tl.operands("trainer", B, C * H * W, 3)
    loc[0, 3] = np.nan
    ls[1, 7] = np.nan
    g_z, g_KL = tl.cotangents(B, C * H * W, ns, 4)
    dev = run_latent(loc, ls, ns, 0, 1, (C, H, W), g_z, g_KL)
    hit = np.zeros((B, C * H * W), bool)
    hit[0, 3] = hit[1, 7] = True
    assert np.array_equal(np.isnan(dev["kl"]), hit)
    assert np.array_equal(np.isnan(dev["z"]), np.broadcast_to(hit, (ns,) + hit.shape))
    assert np.isnan(dev["KL"]).tolist() == [True, True, False]
    only_loc, only_ls = np.zeros_like(hit), np.zeros_like(hit)
    only_loc[0, 3] = only_ls[1, 7] = True
    assert np.array_equal(np.isnan(dev["g_loc"]), only_loc) and np.array_equal(np.isnan(dev["g_log_scale"]), only_ls)
    assert np.isfinite(dev["eps"]).all()


def test_cotangent_handling(monkeypatch):
    """Only g_z (KL unused: the kernel gets a null g_KL), only g_KL, a non-contiguous g_z, and neither -- where no backward is
    launched."""
    B, C, H, W, ns, fo, level = SHAPES["3x1x5x7"]
    c = device_case("3x1x5x7", "trainer")
    length = C * H * W
    dev = _dev()

    def fresh():
        skip = torch.from_numpy(np.stack([c["loc"], c["log_scale"]], axis=1)).to(dev).reshape(B, 2 * C, H, W).requires_grad_(True)
        return (skip,) + normal_latents(skip, ns=ns, seed=SEED, draw=DRAW, level=level, first_object=fo)

    def halves(g):
        g = g.reshape(B, 2, length).cpu().numpy()
        return dict(g_loc=g[:, 0], g_log_scale=g[:, 1])
    gz = torch.from_numpy(c["g_z"]).to(dev).reshape(ns * B, C, H, W)
    gk = torch.from_numpy(c["g_KL"]).to(dev)
    zero_z, zero_k = np.zeros_like(c["g_z"]), np.zeros_like(c["g_KL"])
    skip, z, KL = fresh()
    g_only_z, = torch.autograd.grad((z * gz).sum(), skip)
    ref = tl.case("trainer", B, length, ns, SEED, first_object=fo, draw=DRAW, level=level, cotangents_=(c["g_z"], zero_k))
    assert_within_bars("only g_z", halves(g_only_z), ref, ("g_loc", "g_log_scale"))
    skip, z, KL = fresh()
    g_only_k, = torch.autograd.grad((KL * gk).sum(), skip)
    ref = tl.case("trainer", B, length, ns, SEED, first_object=fo, draw=DRAW, level=level, cotangents_=(zero_z, c["g_KL"]))
    assert_within_bars("only g_KL", halves(g_only_k), ref, ("g_loc", "g_log_scale"))
    # a non-contiguous cotangent: every second column of a tensor twice as wide
    wide = torch.zeros(ns * B, C, H, 2 * W, device=dev)
    wide[..., ::2] = gz
    strided = wide[..., ::2]
    assert not strided.is_contiguous()
    skip, z, KL = fresh()
    torch.autograd.backward((z,), (strided,))
    assert torch.equal(skip.grad, g_only_z)
    # neither cotangent: nothing is launched, nothing flows
    calls = []
    real = _lib.load()

    class Counting:
        def __getattr__(self, name):
            if name == "ctpvae_latent_bwd_f32":
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(latents._lib, "load", lambda: Counting())
    ctx = types.SimpleNamespace(saved_tensors=(skip.detach(),), eps=None, key=(ns, tl.EPS32, fo, SEED, DRAW, level))
    assert latents._NormalLatents.backward(ctx, None, None) == (None,) * 8 and not calls
    skip, z, KL = fresh()
    g, = torch.autograd.grad(skip.sum() + 0 * z.detach().sum(), skip)                  # the outputs are not part of the loss
    assert torch.equal(g, torch.ones_like(g)) and not calls
    g, = torch.autograd.grad((KL * gk).sum(), skip)
    assert calls == ["ctpvae_latent_bwd_f32"] and torch.equal(g, g_only_k)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 --normal -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def test_find_loss_feeds_the_decoder_the_fused_latents_of_every_level(monkeypatch):
    """find_loss_vae_unsup(fused_latents=(seed, draw, first_object)): the decoder's inputs are, level by level, within the bars of the
    float64 composition on the encoder's own outputs with the host's draws for (seed, draw, level, first_object), sample-major; the
    KL it returns is the levels' device sums added in ascending level without the input level's."""
    t = _small_trainer()
    ns, B = 2, 3
    seed, draw, fo = 99, 4, 6
    ps, m, ie = t._batch()
    angles_i = torch.from_numpy(np.ascontiguousarray(t.angles.next().astype(np.int32)))
    kept = {}
    real_decode = t.dec.forward

    def decode(lat):
        kept["latents"] = [z.detach() for z in lat]
        return real_decode(lat)
    monkeypatch.setattr(t.dec, "forward", decode)
    with torch.no_grad():
        skips = t.enc(ie / 300)
        _, kl, _, _ = tr.find_loss_vae_unsup(ps, m, ie, t.enc, t.dec, t.pnm, t.sqrt_reg, 1.0, 1.0, num_samples=ns, theta=t.theta_host,
                                             angles_i=angles_i, pad=t.pad, fused_latents=(seed, draw, fo))
    assert len(kept["latents"]) == len(skips) == t.args.num_blocks + 1 and kl.shape == (B,)
    total = None
    for level, (sk, z) in enumerate(zip(skips, kept["latents"])):
        C, H, W = sk.shape[1] // 2, sk.shape[2], sk.shape[3]
        assert z.shape == (ns * B, C, H, W)
        flat = sk.contiguous().reshape(B, 2, C * H * W).cpu().numpy()
        c = tl.case(None, B, C * H * W, ns, seed, first_object=fo, draw=draw, level=level, operands_=(flat[:, 0], flat[:, 1]),
                    sqrt_reg=t.sqrt_reg)
        assert c["R"]["z"] <= tl.R_MAX
        worst = float(np.max(tl.excess(z.reshape(ns, B, -1).cpu().numpy(), c["want"]["z"], c["bar"]["z"])))
        print(f"level {level}: len {C * H * W}, worst |z - ref| / bar = {worst:.3f}, R = {c['R']['z']:.3f}")
        assert worst <= tl.MARGIN * c["R"]["z"]
        if level >= 1:
            _, KL = normal_latents(sk.contiguous(), ns=ns, seed=seed, draw=draw, level=level, first_object=fo, sqrt_reg=t.sqrt_reg)
            total = KL if total is None else total + KL
    assert torch.equal(kl, total)


def test_fused_latents_training_runs_are_finite():
    for extra in ("--fused_latents", "--fused_latents --fused_head"):
        losses, _ = _small_trainer(extra).train()
        assert len(losses) == 3 and all(math.isfinite(v) for v in losses), (extra, losses)


def test_fused_latents_and_head_training_run_is_reproducible():
    """With --fused_head --fused_latents nothing in the step draws from torch's global generator: two equal-seed runs under
    --reproducible (deterministic convolution algorithms) are bit-equal, losses and parameters."""
    runs = []
    was = torch.backends.cudnn.deterministic            # (--reproducible switches it on for the process: put back for the tests that follow)
    try:
        for k in range(2):
            t = _small_trainer("--reproducible --fused_head --fused_latents")
            torch.manual_seed(1000 + k)                 # the global generator is not part of the step: another state, the same run
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
            runs.append((losses, [p.detach().clone() for p in t.params]))
    finally:
        torch.backends.cudnn.deterministic = was
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
