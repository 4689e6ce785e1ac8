"""The ConvBlock's dropout on the device (ct_pvae_amd/convblock.py dropout / dropout_pad, csrc/convblock.hip) against
tests/np_twin_dropout.py and tests/np_twin_convblock.py, by bits unless a test says otherwise; cotangent handling, streams, what the
nodes save, a ConvBlock with dropout and the trainer with --dp."""
import math
import types

import numpy as np
import pytest
import torch

from ct_pvae_amd import convblock, dropout, dropout_pad, periodic_pad
from ct_pvae_amd import trainer as tr
from tests import np_twin_convblock as tw
from tests import np_twin_dropout as td

pytestmark = pytest.mark.gpu

SEED, DRAW, LAYER = 1234, 7, 5
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 2, 16, 16), (2, 1, 130, 67)]


def _dev():
    return torch.device("cuda", 0)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _data(shape, salt=0):
    rng = np.random.default_rng(17 * sum(shape) + salt)
    return rng.standard_normal(shape).astype(np.float32)


def _to_dev(a, unaligned=False):
    """The array on the device; unaligned: as a view one float into a larger buffer, so the pointer is 4 bytes past a 16-byte line."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not unaligned:
        return t.to(_dev())
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=_dev())
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _key(first=0):
    return dict(seed=SEED, draw=DRAW, layer=LAYER, first_object=first)


def run(op, x, g, unaligned=False):
    xt = _to_dev(x, unaligned).detach().requires_grad_(True)
    out = op(xt)
    gx, = torch.autograd.grad(out, xt, _to_dev(g, unaligned))
    return out.detach(), gx


# ---- the standalone pair -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=tw.shape_id)
def test_dropout_forward_and_backward_are_the_twin_bit_for_bit(shape):
    """Both rates; first_object 0, 1 (len odd: the Philox blocks straddle the quads) and 2^34 // len (the second counter word); an
    aligned pointer and one 4 bytes past a 16-byte line."""
    x, g = _data(shape), _data(shape, 1)
    length = x[0].size
    for rate in td.RATES:
        for first in (0, 1, 2 ** 34 // length):
            k = td.keep_like(x, rate, SEED, DRAW, LAYER, first)
            want, want_g = td.drop_fwd(x, k, rate), td.drop_bwd(g, k, rate)
            for unaligned in (False, True):
                out, gx = run(lambda t: dropout(t, rate, **_key(first)), x, g, unaligned)
                assert out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()
                assert np.array_equal(_bits(out), _bits(want)), (rate, first, unaligned)
                assert tuple(gx.shape) == shape and np.array_equal(_bits(gx), _bits(want_g)), (rate, first, unaligned)


@pytest.mark.parametrize("rate", td.RATES)
def test_dropout_selects(rate):
    """A NaN and an infinity at dropped places give +0, a kept -0.0 stays -0.0, an infinite cotangent at a dropped place gives +0."""
    shape = (2, 3, 5, 7)
    x, g = _data(shape), _data(shape, 1)
    k = td.keep_like(x, rate, SEED, DRAW, LAYER, 1)
    dropped, kept = np.flatnonzero(~k.reshape(-1)), np.flatnonzero(k.reshape(-1))
    assert len(dropped) >= 3 and len(kept) >= 1
    x.reshape(-1)[dropped[0]], x.reshape(-1)[dropped[1]], x.reshape(-1)[kept[0]] = np.nan, np.inf, -0.0
    g.reshape(-1)[dropped[2]], g.reshape(-1)[dropped[0]] = np.inf, -np.inf
    for unaligned in (False, True):
        out, gx = run(lambda t: dropout(t, rate, **_key(1)), x, g, unaligned)
        out, gx = out.cpu().numpy(), gx.cpu().numpy()
        assert np.array_equal(_bits(out), _bits(td.drop_fwd(x, k, rate))) and np.array_equal(_bits(gx), _bits(td.drop_bwd(g, k, rate)))
        assert not np.isnan(out).any() and np.isfinite(out).all() and np.isfinite(gx).all()
        assert (_bits(out).reshape(-1)[dropped] == 0).all() and (_bits(gx).reshape(-1)[dropped] == 0).all()       # +0, not -0
        assert _bits(out).reshape(-1)[kept[0]] == 0x80000000


# ---- fused into the pad --------------------------------------------------------------------------------------------------------
def _pad_input(case):
    """tests/test_gpu_convblock.py's input: standard normal with an infinity (a NaN at one element) and a NaN planted."""
    shape, pads = case
    x = _data(shape, sum(pads))
    flat = x.reshape(-1)
    flat[0] = np.nan if flat.size == 1 else np.inf
    flat[-1] = np.nan
    return x


@pytest.mark.parametrize("case", tw.PAD_CASES, ids=tw.pad_id)
def test_dropout_pad_forward_is_pad_of_dropout_three_ways(case):
    shape, pads = case
    x = _pad_input(case)
    xt = torch.from_numpy(x).to(_dev())
    plain = tw.pad_fwd(x, pads)
    for rate in td.RATES:
        for first in (0, 1):
            k = td.keep_like(x, rate, SEED, DRAW, LAYER, first)
            out = dropout_pad(xt, pads, rate, **_key(first))
            assert out.dtype == torch.float32 and tuple(out.shape) == plain.shape and out.is_contiguous()
            assert np.array_equal(_bits(out), _bits(tw.pad_fwd(td.drop_fwd(x, k, rate), pads))), (rate, first)
            assert np.array_equal(_bits(out), _bits(periodic_pad(dropout(xt, rate, **_key(first)), pads))), (rate, first)
            with np.errstate(invalid="ignore", over="ignore"):
                at_source = np.where(tw.pad_fwd(k, pads), plain * td.scale(rate), np.float32(0.0)).astype(np.float32)
            assert np.array_equal(_bits(out), _bits(at_source)), (rate, first)


@pytest.mark.parametrize("case", tw.PAD_CASES, ids=tw.pad_id)
def test_dropout_pad_backward_is_the_pads_backward_masked_and_scaled(case):
    """By bits: the device's own periodic_pad backward (the same two folds), masked and scaled by the twin.  In value: the twin's
    folds, masked and scaled (the sign of a zero sum is not held there, as in tests/test_gpu_convblock.py).  The same from call to call."""
    shape, pads = case
    x = np.nan_to_num(_pad_input(case), nan=0.5, posinf=2.0)
    g = _data(tw.pad_fwd(x, pads).shape, 3)
    _, acc = run(lambda t: periodic_pad(t, pads), x, g)
    folds = tw.pad_bwd(g, shape[2:], pads)
    for rate in td.RATES:
        for first in (0, 1):
            k = td.keep_like(x, rate, SEED, DRAW, LAYER, first)
            _, gx = run(lambda t: dropout_pad(t, pads, rate, **_key(first)), x, g)
            assert tuple(gx.shape) == shape and gx.dtype == torch.float32
            assert np.array_equal(_bits(gx), _bits(td.drop_bwd(acc.cpu().numpy(), k, rate))), (rate, first)
            assert np.array_equal(gx.cpu().numpy(), td.drop_bwd(folds, k, rate)), (rate, first)
            _, again = run(lambda t: dropout_pad(t, pads, rate, **_key(first)), x, g)
            assert torch.equal(gx, again)


# ---- batches, saved tensors, cotangents, streams -------------------------------------------------------------------------------
PADS = (2, 1, 1, 1)


def _ops(first=0, rate=0.25):
    return [("dropout", lambda t, f=first: dropout(t, rate, **_key(f))),
            ("dropout_pad", lambda t, f=first: dropout_pad(t, PADS, rate, **_key(f)))]


def test_a_batch_cut_in_two_calls_is_the_whole_batch():
    shape = (4, 3, 5, 7)                                               # len 105: the second call's first element is no multiple of 4
    x = _data(shape)
    for first in (0, 3):
        for (name, whole_op), (_, lo_op), (_, hi_op) in zip(_ops(first), _ops(first), _ops(first + 2)):
            g = _data(tuple(whole_op(torch.from_numpy(x).to(_dev())).shape), 1)
            out, gx = run(whole_op, x, g)
            out_lo, gx_lo = run(lo_op, x[:2], g[:2])
            out_hi, gx_hi = run(hi_op, x[2:], g[2:])
            assert torch.equal(torch.cat([out_lo, out_hi]), out) and torch.equal(torch.cat([gx_lo, gx_hi]), gx), (name, first)


def test_nothing_is_saved_for_the_backward():
    x = torch.from_numpy(_data((2, 3, 5, 7))).to(_dev()).requires_grad_(True)
    for name, op in _ops():
        out = op(x)
        assert out.grad_fn is not None and tuple(out.grad_fn.saved_tensors) == (), name


def test_a_missing_cotangent_gives_no_gradient():
    ctx = types.SimpleNamespace(geom=(2, 3, 5, 7, 2, 1, 1, 1), key=(0, SEED, DRAW, LAYER, td.threshold(0.25), float(td.scale(0.25))))
    assert convblock._Dropout.backward(ctx, None) == (None, None)
    assert convblock._FusedDropoutPad.backward(ctx, None) == (None, None, None)
    for name, op in _ops():
        xt = torch.from_numpy(_data((2, 3, 5, 7))).to(_dev()).requires_grad_(True)
        out = op(xt)
        g, = torch.autograd.grad(xt.sum() + 0 * out.detach().sum(), xt)             # the output is not part of the loss
        assert torch.equal(g, torch.ones_like(g)), name


def test_strided_and_float64_cotangents_give_the_gradient_of_their_float32_copy():
    x = _data((2, 3, 5, 7))
    for name, op in _ops():
        xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
        gd = torch.from_numpy(_data(tuple(op(xt).shape), 1)).to(_dev())
        want, = torch.autograd.grad(op(xt), xt, gd)
        strided = gd.transpose(2, 3).contiguous().transpose(2, 3)                   # the same values, the last two strides swapped
        assert not strided.is_contiguous() and strided.shape == gd.shape
        got, = torch.autograd.grad(op(xt), xt, strided)
        assert torch.equal(got, want), name
        got, = torch.autograd.grad(op(xt), xt, gd.double())
        assert got.dtype == torch.float32 and torch.equal(got, want), name
        # the nodes themselves convert: called directly, past autograd's own cast of a cotangent's dtype
        direct = op(xt).grad_fn.apply(gd.double().transpose(2, 3).contiguous().transpose(2, 3))
        direct = direct[0] if isinstance(direct, tuple) else direct
        assert direct.dtype == torch.float32 and torch.equal(direct, want), name


def test_both_ops_launch_on_the_current_stream():
    side = torch.cuda.Stream(device=_dev())
    x = _data((2, 3, 5, 7))
    for name, op in _ops():
        xt = torch.from_numpy(x).to(_dev()).requires_grad_(True)
        out = op(xt)
        gd = torch.from_numpy(_data(tuple(out.shape), 1)).to(_dev())
        gx, = torch.autograd.grad(out, xt, gd)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out_s = op(xt)
            gx_s, = torch.autograd.grad(out_s, xt, gd)
        side.synchronize()
        assert torch.equal(out_s, out) and torch.equal(gx_s, gx), name


def test_argument_errors_come_before_any_launch():
    x = torch.from_numpy(_data((2, 3, 5, 7))).to(_dev())
    for rate in (0.0, 1.0, -0.1, float("nan"), 1 - 1e-9):
        with pytest.raises(ValueError):
            dropout(x, rate, **_key())
        with pytest.raises(ValueError):
            dropout_pad(x, PADS, rate, **_key())
    with pytest.raises(ValueError):
        dropout(x, 0.5, seed=0, draw=0, layer=2 ** 24)
    with pytest.raises(ValueError):
        dropout_pad(x, (1, 1, -1, 1), 0.5, **_key())
    with pytest.raises(ValueError):
        dropout(x, 0.5, seed=0, draw=0, layer=0, first_object=2 ** 63 // 105)
    with pytest.raises(TypeError):
        dropout(x.double(), 0.5, **_key())
    with pytest.raises(ValueError):
        dropout(x.transpose(2, 3), 0.5, **_key())
    with pytest.raises(convblock._lib.RadonLibraryError):
        dropout(x.cpu(), 0.5, **_key())
    with pytest.raises(convblock._lib.RadonLibraryError):
        dropout_pad(x.cpu(), PADS, 0.5, **_key())
    torch.cuda.synchronize()


# ---- ConvBlock -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transposed"])
def test_convblock_with_dropout(transpose):
    """k = 4, stride 2 on [2][3][16][16], rate 0.25, layer 5, draw 2, first_object 3.  eval(), and train() while the key holds no draw:
    the block without dropout, bit for bit.  train() with a draw: dropout -> the undropped block's forward on that tensor, bit for
    bit, with fused_blocks and without, so the two agree; the gradient of the input is +0 at every dropped element."""
    dev = _dev()
    torch.manual_seed(5)
    rate = 0.25
    x = torch.randn(2, 3, 16, 16, device=dev)
    k = torch.from_numpy(td.keep_like(x.cpu().numpy(), rate, SEED, 2, 5, 3)).to(dev)
    outs = []
    for fused in (False, True):
        plain = tr.ConvBlock(3, 4, 4, 2, transpose, fused_blocks=fused).to(dev)
        if outs:
            plain.load_state_dict(outs[0][1])
        key = tr.DropoutKey(rate, SEED)
        blk = tr.ConvBlock(3, 4, 4, 2, transpose, fused_blocks=fused, dropout=key, layer=5).to(dev)
        blk.load_state_dict(plain.state_dict())
        want_plain = plain(x)
        assert blk.training and torch.equal(blk(x), want_plain)                    # no draw set: nothing is dropped
        key.set(2, 3)
        assert torch.equal(blk.eval()(x), want_plain)
        blk.train()
        xt = x.clone().requires_grad_(True)
        out = blk(xt)
        dropped_x = dropout(x, rate, seed=SEED, draw=2, layer=5, first_object=3)
        assert torch.equal(dropped_x != 0, k & (x != 0)) and not torch.equal(dropped_x, x)
        assert torch.equal(out, plain(dropped_x)) and not torch.equal(out, want_plain)
        out.backward(torch.ones_like(out))
        assert (_bits(xt.grad)[~k.cpu().numpy()] == 0).all() and (xt.grad[k] != 0).any()
        key.clear()
        assert torch.equal(blk(x), want_plain)
        outs.append((out.detach(), plain.state_dict()))
    assert torch.equal(outs[0][0], outs[1][0])


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
_runs = {}


def _run(extra):
    """One training run of tests/test_gpu_convblock.py's small recipe under --fused_head --fused_latents --reproducible, kept."""
    if extra not in _runs:
        was = torch.backends.cudnn.deterministic        # (--reproducible switches it on for the process: put back for the tests that follow)
        try:
            args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 --normal -i 3 --train --fused_head --fused_latents "
                                "--reproducible " + extra).split())
            t = tr.PVAETrainer(args, _dev())
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses), losses
            torch.manual_seed(99)                        # the evaluation's latents and head come from torch's global generator
            final = t.final_evaluation()
        finally:
            torch.backends.cudnn.deterministic = was
        _runs[extra] = dict(trainer=t, losses=losses, params=[p.detach().clone() for p in t.params], final=final)
    return _runs[extra]


def test_two_dropout_runs_are_bit_equal_and_differ_from_a_run_without():
    a = _run("--dp 0.2")
    t = a["trainer"]
    blocks = [m for net in (t.enc, t.dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
    assert [m.layer for m in blocks] == list(range(len(blocks))) and t.enc_drop.draw is None and t.dec_drop.draw is None
    _runs["again"] = _runs.pop("--dp 0.2")
    b = _run("--dp 0.2")
    print("losses", a["losses"], b["losses"])
    assert a["losses"] == b["losses"] and all(torch.equal(p, q) for p, q in zip(a["params"], b["params"]))
    none = _run("--dp 0")
    print("losses without dropout", none["losses"])
    assert none["trainer"].enc_drop is None and none["losses"] != a["losses"]
    assert not all(torch.equal(p, q) for p, q in zip(a["params"], none["params"]))


def test_dropout_run_with_fused_blocks_is_the_unfused_run_bit_for_bit():
    a, f = _run("--dp 0.2"), _run("--dp 0.2 --fused_blocks")
    print("losses", a["losses"], f["losses"])
    differing = [i for i, (p, q) in enumerate(zip(a["params"], f["params"])) if not torch.equal(p, q)]
    print("parameters that differ:", differing)
    assert a["losses"] == f["losses"] and not differing


def test_final_evaluation_runs_without_dropout():
    """The --dp 0.2 trainer's final evaluation is the one of a --dp 0 trainer that holds the same weights: same losses, same samples."""
    a, none = _run("--dp 0.2"), _run("--dp 0")
    t = none["trainer"]
    t.enc.load_state_dict(a["trainer"].enc.state_dict())
    t.dec.load_state_dict(a["trainer"].dec.state_dict())
    was = torch.backends.cudnn.deterministic
    try:
        torch.backends.cudnn.deterministic = True
        torch.manual_seed(99)
        loss_final, recon_final = t.final_evaluation()
    finally:
        torch.backends.cudnn.deterministic = was
    assert np.array_equal(loss_final, a["final"][0]) and np.array_equal(recon_final, a["final"][1])
    assert not np.array_equal(loss_final, none["final"][0])                        # (the weights did change)
