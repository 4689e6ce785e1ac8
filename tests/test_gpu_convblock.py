"""The fused ConvBlock glue on the device (ct_pvae_amd/convblock.py, csrc/convblock.hip) against tests/np_twin_convblock.py -- by bits
forward, in value backward (the sign of a zero sum is not held: the torch chain starts from +0) -- and against the trainer's
_PeriodicPad and _Maxout on the device; cotangent handling, streams, a ConvBlock and the trainer with --fused_blocks."""
import math
import types

import numpy as np
import pytest
import torch

from ct_pvae_amd import convblock, maxout, periodic_pad
from ct_pvae_amd import trainer as tr
from tests import np_twin_convblock as tw

pytestmark = pytest.mark.gpu

_pad_cases, _maxout_cases = {}, {}


def _dev():
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pad_case(case):
    """One (shape, pads): the input (standard normal with a NaN and an infinity planted), a finite cotangent and the twin's results,
    computed once, shared and left unchanged."""
    if case not in _pad_cases:
        shape, pads = case
        rng = np.random.default_rng(11 * sum(shape) + sum(pads))
        x = rng.standard_normal(shape).astype(np.float32)
        flat = x.reshape(-1)
        flat[0] = np.nan if flat.size == 1 else np.inf
        flat[-1] = np.nan
        out = tw.pad_fwd(x, pads)
        g = rng.standard_normal(out.shape).astype(np.float32)
        _pad_cases[case] = dict(x=x, out=out, g=g, gx=tw.pad_bwd(g, shape[2:], pads))
    return _pad_cases[case]


def maxout_case(shape):
    if shape not in _maxout_cases:
        rng = np.random.default_rng(13 * sum(shape))
        y = rng.standard_normal(shape).astype(np.float32)
        out, first = tw.maxout_fwd(y)
        g = rng.standard_normal(out.shape).astype(np.float32)
        _maxout_cases[shape] = dict(y=y, out=out, first=first, g=g, gy=tw.maxout_bwd(g, first))
    return _maxout_cases[shape]


def run_pad(x, pads, g):
    xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
    out = periodic_pad(xt, pads)
    gx, = torch.autograd.grad(out, xt, torch.from_numpy(g).to(_dev()))
    return out.detach(), gx


def run_maxout(y, g):
    yt = torch.from_numpy(y).to(_dev()).requires_grad_(True)
    out = maxout(yt)
    gy, = torch.autograd.grad(out, yt, torch.from_numpy(g).to(_dev()))
    return out.detach(), gy


# ---- periodic pad --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tw.PAD_CASES, ids=tw.pad_id)
def test_pad_forward_is_the_twin_bit_for_bit(case):
    c = pad_case(case)
    assert np.isnan(c["x"]).any() and (case[0] == (1, 1, 1, 1) or np.isinf(c["x"]).any())
    out, _ = run_pad(c["x"], case[1], c["g"])
    assert out.dtype == torch.float32 and tuple(out.shape) == c["out"].shape and out.is_contiguous()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(c["out"]))


@pytest.mark.parametrize("case", tw.PAD_CASES, ids=tw.pad_id)
def test_pad_backward_is_the_twin_and_the_same_from_run_to_run(case):
    """np.array_equal with the twin's two ascending folds on every shape (values: a zero's sign is not held); where every source
    element has at most two copies per axis -- the pads of an axis together do not exceed its extent, so no sum has more than two
    terms per axis and the order of the device's index_add_ cannot matter -- also torch.equal with trainer._PeriodicPad's gradient
    on the device."""
    shape, pads = case
    c = pad_case(case)
    _, gx = run_pad(c["x"], pads, c["g"])
    assert tuple(gx.shape) == shape and gx.dtype == torch.float32
    assert np.array_equal(gx.cpu().numpy(), c["gx"])
    _, again = run_pad(c["x"], pads, c["g"])
    assert torch.equal(gx, again)
    if tw.at_most_two_copies(shape, pads):
        xt = torch.from_numpy(c["x"]).to(_dev()).requires_grad_(True)
        ref, = torch.autograd.grad(tr._PeriodicPad.apply(xt, pads), xt, torch.from_numpy(c["g"]).to(_dev()))
        assert torch.equal(gx, ref)


def test_pad_chain_comparison_covers_the_shapes_it_can():
    assert [tw.at_most_two_copies(*c) for c in tw.PAD_CASES] == [False, False, False, True, True, True, True]


# ---- maxout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tw.MAXOUT_SHAPES, ids=tw.shape_id)
def test_maxout_forward_and_backward_are_the_twin_and_the_trainers(shape):
    """Forward by bits; with finite cotangents the backward is torch.equal to the twin and to trainer._Maxout's gradient."""
    c = maxout_case(shape)
    out, gy = run_maxout(c["y"], c["g"])
    assert out.dtype == torch.float32 and tuple(out.shape) == c["out"].shape
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(c["out"]))
    assert tuple(gy.shape) == shape and torch.equal(gy.cpu(), torch.from_numpy(c["gy"]))
    yt = torch.from_numpy(c["y"]).to(_dev()).requires_grad_(True)
    ref, = torch.autograd.grad(tr._Maxout.apply(yt), yt, torch.from_numpy(c["g"]).to(_dev()))
    assert torch.equal(gy, ref)


def test_maxout_planted_pairs_and_an_infinite_cotangent():
    """A tie, a NaN in the first half only, a NaN in the second half only, (-0, +0), (+0, -0), (inf, inf), (-inf, 1): the twin's bits.
    With an infinite cotangent the half that was taken gets inf and the other 0 -- the kernel selects.  trainer._Maxout multiplies
    (g * first, then g - that) and gives NaN there through inf * 0 and inf - inf, so it is not compared on this input."""
    y, first = tw.planted_maxout()
    want, got_first = tw.maxout_fwd(y)
    assert np.array_equal(got_first, first)
    g = np.full(want.shape, np.inf, np.float32)
    g[..., 1] = -np.inf
    out, gy = run_maxout(y, g)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    gy = gy.cpu().numpy()
    assert np.array_equal(_bits(gy), _bits(tw.maxout_bwd(g, first))) and not np.isnan(gy).any()
    assert np.array_equal(gy[:, :1], np.where(first, g, 0.0)) and np.array_equal(gy[:, 1:], np.where(first, 0.0, g))


def test_maxout_saves_one_byte_per_output_element():
    c = maxout_case((3, 4, 16, 16))
    yt = torch.from_numpy(c["y"]).to(_dev()).requires_grad_(True)
    out = maxout(yt)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 1
    for t in saved:
        assert t.numel() * t.element_size() <= out.numel()
    assert torch.equal(saved[0].bool().cpu(), torch.from_numpy(c["first"]))


# ---- cotangents and streams ------------------------------------------------------------------------------------------------------
def _ops():
    """(name, op, input, finite cotangent as numpy) of one pad and one maxout case."""
    pc = ((2, 3, 5, 7), (2, 1, 1, 1))
    c, m = pad_case(pc), maxout_case((2, 6, 3, 5))
    x = np.nan_to_num(c["x"], nan=0.5, posinf=2.0)
    return [("pad", lambda t: periodic_pad(t, pc[1]), x, c["g"]), ("maxout", maxout, m["y"], m["g"])]


def test_a_missing_cotangent_gives_no_gradient():
    ctx = types.SimpleNamespace(geom=(2, 3, 5, 7, 2, 1, 1, 1), saved_tensors=(torch.zeros(1, 1, 1, 1, dtype=torch.uint8),))
    assert convblock._FusedPeriodicPad.backward(ctx, None) == (None, None)
    assert convblock._FusedMaxout.backward(ctx, None) is None
    for name, op, x, _ in _ops():
        xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
        out = op(xt)
        g, = torch.autograd.grad(xt.sum() + 0 * out.detach().sum(), xt)             # the output is not part of the loss
        assert torch.equal(g, torch.ones_like(g)), name


def test_strided_and_float64_cotangents_give_the_gradient_of_their_float32_copy():
    for name, op, x, g in _ops():
        gd = torch.from_numpy(g).to(_dev())
        xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
        want, = torch.autograd.grad(op(xt), xt, gd)
        strided = gd.transpose(2, 3).contiguous().transpose(2, 3)                   # the same values, the last two strides swapped
        assert not strided.is_contiguous() and strided.shape == gd.shape
        got, = torch.autograd.grad(op(xt), xt, strided)
        assert torch.equal(got, want), name
        got, = torch.autograd.grad(op(xt), xt, gd.double())
        assert got.dtype == torch.float32 and torch.equal(got, want), name
        # the nodes themselves convert: called directly, past autograd's own cast of a cotangent's dtype
        out = op(xt)
        direct = out.grad_fn.apply(gd.double().transpose(2, 3).contiguous().transpose(2, 3))
        direct = direct[0] if isinstance(direct, tuple) else direct
        assert direct.dtype == torch.float32 and torch.equal(direct, want), name


def test_both_ops_launch_on_the_current_stream():
    side = torch.cuda.Stream(device=_dev())
    for name, op, x, g in _ops():
        gd = torch.from_numpy(g).to(_dev())
        xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
        out = op(xt)
        gx, = torch.autograd.grad(out, xt, gd)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out_s = op(xt)
            gx_s, = torch.autograd.grad(out_s, xt, gd)
        side.synchronize()
        assert torch.equal(out_s, out) and torch.equal(gx_s, gx), name


# ---- ConvBlock -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transposed"])
def test_convblock_with_fused_blocks_is_the_unfused_block(transpose):
    """k = 4, stride 2 on [2][3][16][16]: the same tensor enters the convolution, the output is torch.equal, and so is the gradient
    arriving at the convolution's output (the maxout's backward)."""
    dev = _dev()
    torch.manual_seed(5)
    plain = tr.ConvBlock(3, 4, 4, 2, transpose).to(dev)
    fused = tr.ConvBlock(3, 4, 4, 2, transpose, fused_blocks=True).to(dev)
    fused.load_state_dict(plain.state_dict())
    x = torch.randn(2, 3, 16, 16, device=dev)
    seen = {}
    for tag, blk in (("plain", plain), ("fused", fused)):
        kept = seen.setdefault(tag, {})

        def pre(mod, args, kept=kept):
            kept["conv_in"] = args[0].detach().clone()

        def post(mod, args, result, kept=kept):
            result.register_hook(lambda g: kept.__setitem__("g_conv_out", g.detach().clone()))
        h1, h2 = blk.ab.register_forward_pre_hook(pre), blk.ab.register_forward_hook(post)
        out = blk(x)
        if "cot" not in seen:
            seen["cot"] = torch.randn_like(out)
        out.backward(seen["cot"])
        kept["out"] = out.detach()
        h1.remove(), h2.remove()
    p, f = seen["plain"], seen["fused"]
    assert p["conv_in"].shape == ((2, 3, 16, 16) if transpose else (2, 3, 18, 18))
    assert torch.equal(f["conv_in"], p["conv_in"])
    assert torch.equal(f["out"], p["out"]) and f["out"].shape == ((2, 4, 32, 32) if transpose else (2, 4, 8, 8))
    assert torch.equal(f["g_conv_out"], p["g_conv_out"])


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 --normal -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def test_fused_blocks_training_run_is_finite():
    t = _small_trainer("--fused_blocks")
    assert all(m.fused_blocks for net in (t.enc, t.dec) for m in net.modules() if isinstance(m, tr.ConvBlock))
    losses, _ = t.train()
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), losses


def test_fused_blocks_training_run_is_the_unfused_run_bit_for_bit():
    """Under --reproducible --fused_head --fused_latents runs are bit-equal from run to run (tests/test_gpu_latent.py); there a run
    with --fused_blocks and a run without it give equal losses and torch.equal parameters: the forwards are copies and selections,
    every pad of this recipe is at most 3 on extents of at least 16 (at most two terms per backward sum and axis), a zero of either
    sign changes no later value, and the convolution algorithms are fixed."""
    runs = []
    was = torch.backends.cudnn.deterministic            # (--reproducible switches it on for the process: put back for the tests that follow)
    try:
        for extra in ("", " --fused_blocks"):
            t = _small_trainer("--reproducible --fused_head --fused_latents" + extra)
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
            runs.append((losses, [p.detach().clone() for p in t.params]))
    finally:
        torch.backends.cudnn.deterministic = was
    print("losses", runs[0][0], runs[1][0])
    differing = [i for i, (a, b) in enumerate(zip(runs[0][1], runs[1][1])) if not torch.equal(a, b)]
    print("parameters that differ:", differing)
    assert runs[0][0] == runs[1][0]
    assert not differing
