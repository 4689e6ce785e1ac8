"""The fused ConvBlock convolution on the device (ct_pvae_amd/conv.py, csrc/conv.hip) against tests/np_twin_conv.py BY BITS -- out,
first, gx, gw and gb --, the matrix instruction's lane maps with exact integers, planted ties, a NaN, an infinite cotangent, the tail
rule, object independence, run-to-run equality, the skipped input gradient, torch's float64 ConvBlock on the device within the
twin's bars, and the trainer with --fused_conv."""
import math

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, conv, periodic_conv_maxout
from ct_pvae_amd import trainer as tr
from tests import np_twin_conv as tw
from tests import np_twin_convblock as cb

pytestmark = pytest.mark.gpu

_cases = {}


def _dev():
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def operands(case, integers=False):
    N, Cin, H, W, C, k, s = case
    rng = np.random.default_rng(sum(case) + 17 * k)
    pads = tw.block_pads(H, W, k, s)
    gshape = (N, C) + tw.out_hw(H, W, k, s, pads)
    if integers:          # small, asymmetric, exact: every sum is an integer below 2^24 whatever its order
        x = rng.integers(-3, 4, (N, Cin, H, W)).astype(np.float32)
        w = rng.integers(-2, 3, (2 * C, Cin, k, k)).astype(np.float32)
        b = rng.integers(-5, 6, 2 * C).astype(np.float32)
        g = rng.integers(-2, 3, gshape).astype(np.float32)
    else:
        x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
        w = (rng.standard_normal((2 * C, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
        b = (0.1 * rng.standard_normal(2 * C)).astype(np.float32)
        g = rng.standard_normal(gshape).astype(np.float32)
    return dict(x=x, w=w, b=b, g=g, s=s, k=k, pads=pads)


def twin(c):
    """The twin's five results of one set of operands, added to the dict."""
    out, first = tw.forward(c["x"], c["w"], c["b"], c["s"], c["pads"])
    gw, gb = tw.weight_grad(c["x"], c["g"], first, c["k"], c["s"], c["pads"])
    gx = tw.input_grad(c["g"], first, c["w"], c["x"].shape[2:], c["s"], c["pads"])
    c.update(out=out, first=first, gw=gw, gb=gb, gx=gx)
    return c


def conv_case(case):
    """Operands and the twin's results of one case: computed once, shared and left unchanged."""
    if case not in _cases:
        _cases[case] = twin(operands(case))
    return _cases[case]


def run(c, x_grad=True):
    """The device's (out, first, gx, gw, gb) as numpy; gx is None without x_grad."""
    dev = _dev()
    x = torch.from_numpy(c["x"]).to(dev).requires_grad_(x_grad)
    w = torch.from_numpy(c["w"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(c["b"]).to(dev).requires_grad_(True)
    _, first = conv._conv_maxout_with_first(x, w, b, c["s"], c["pads"])
    out = periodic_conv_maxout(x, w, b, c["s"], c["pads"])
    assert out.dtype == torch.float32 and out.is_contiguous() and first.dtype == torch.uint8 and first.shape == out.shape
    grads = torch.autograd.grad(out, (x, w, b) if x_grad else (w, b), torch.from_numpy(c["g"]).to(dev))
    gx = grads[0].cpu().numpy() if x_grad else None
    return out.detach().cpu().numpy(), first.cpu().numpy(), gx, grads[-2].cpu().numpy(), grads[-1].cpu().numpy()


def assert_is_the_twin(c, got):
    out, first, gx, gw, gb = got
    assert out.shape == c["out"].shape and gw.shape == c["w"].shape and gb.shape == c["b"].shape
    assert set(np.unique(first).tolist()) <= {0, 1}
    assert np.array_equal(first.astype(bool), c["first"])
    for name, a, want in (("out", out, c["out"]), ("gw", gw, c["gw"]), ("gb", gb, c["gb"])) + ((("gx", gx, c["gx"]),) if gx is not None else ()):
        differ = _bits(a) != _bits(want)
        assert not differ.any(), (name, int(differ.sum()), a[differ][:4], want[differ][:4])


@pytest.mark.parametrize("case", tw.CASES + tw.CHUNK_CASES, ids=tw.case_id)
def test_forward_and_gradients_are_the_twin_bit_for_bit(case):
    c = conv_case(case)
    assert c["gx"].shape == c["x"].shape
    assert_is_the_twin(c, run(c))


def test_lane_maps_with_exact_integers():
    """Small asymmetric integer operands: every sum is exact in any order, so a row / column swap, a transposed accumulator tile or a
    k-pair fed to the wrong half shows against an integer evaluation (float64 conv2d on the CPU is exact here), apart from any
    question of rounding.  2C = 40 straddles a 32-row tile, 9 x 10 under stride 2 leaves ragged pixel tiles."""
    case = (3, 4, 9, 10, 20, 4, 2)
    N, Cin, H, W, C, k, s = case
    c = operands(case, integers=True)
    wl, wr, hl, hr = c["pads"]
    x64 = torch.from_numpy(c["x"]).double().requires_grad_(True)
    w64 = torch.from_numpy(c["w"]).double().requires_grad_(True)
    b64 = torch.from_numpy(c["b"]).double().requires_grad_(True)
    xp = x64[:, :, torch.from_numpy(cb.pad_index(H, hl, hr))][:, :, :, torch.from_numpy(cb.pad_index(W, wl, wr))]
    y = torch.nn.functional.conv2d(xp, w64, b64, stride=s)
    first = y[:, :C] >= y[:, C:]
    want = torch.where(first, y[:, :C], y[:, C:])
    assert want.abs().max() < 2 ** 24 and not np.array_equal(c["w"], c["w"].transpose(0, 1, 3, 2))
    gx, gw, gb = torch.autograd.grad(y, (x64, w64, b64), torch.from_numpy(cb.maxout_bwd(c["g"], first.numpy())).double())
    out, got_first, got_gx, got_gw, got_gb = run(c)
    assert np.array_equal(got_first.astype(bool), first.numpy())
    assert np.array_equal(out, want.detach().numpy()) and np.array_equal(got_gw, gw.numpy()) and np.array_equal(got_gb, gb.numpy())
    assert np.array_equal(got_gx, gx.numpy())


def test_equal_halves_tie_everywhere():
    """The second half's weights and bias equal the first's: first is all ones, out is the first half, and the second half's gw and gb
    are +0 by bits (the selection feeds +0, and a chain from +0 of +-0 products stays +0)."""
    c = operands((2, 3, 5, 7, 2, 3, 1))
    c["w"][2:], c["b"][2:] = c["w"][:2], c["b"][:2]
    twin(c)
    got = run(c)
    assert got[1].all() and c["first"].all()
    assert not _bits(got[3][2:]).any() and not _bits(got[4][2:]).any() and got[3][:2].any()
    assert_is_the_twin(c, got)


def test_a_nan_in_x_and_an_infinite_cotangent():
    """A NaN input makes every y that reads it NaN in both halves: the comparison is false and the second half is taken.  An infinite
    cotangent goes to the half that was taken as inf and to the other as +0, by selection: no NaN in any gradient."""
    c = operands((2, 3, 5, 7, 2, 3, 1))
    c["x"][1, 2, 3, 4] = np.nan
    twin(c)
    assert np.isnan(c["out"]).any() and not c["first"][np.isnan(c["out"])].any()
    assert_is_the_twin(c, run(c))
    c = operands((2, 3, 5, 7, 2, 3, 1))
    c["g"][0, 1, 2, 3] = np.inf
    c["g"][1, 0, 4, 6] = -np.inf
    twin(c)
    got = run(c)
    assert_is_the_twin(c, got)
    assert not any(np.isnan(a).any() for a in got[2:]) and np.isinf(got[3]).any() and np.isinf(got[2]).any()


def test_tail_rule_turns_a_negative_zero_into_a_positive_one():
    """K = 1 is odd: a -0 bias with a zero input and positive weights gives -0 products and, through the closing fma(+0, +0, acc), +0;
    K = 2 with no tail keeps -0.  Both are the twin's bits."""
    for cin, sign in ((1, False), (2, True)):
        c = dict(x=np.zeros((1, cin, 3, 3), np.float32), w=-np.ones((2, cin, 1, 1), np.float32), b=np.array([-0.0, -0.0], np.float32),
                 g=np.ones((1, 1, 3, 3), np.float32), s=1, k=1, pads=(0, 0, 0, 0))
        c["x"][:] = 0.0
        twin(c)
        got = run(c)
        assert np.signbit(got[0]).all() == sign and np.signbit(c["out"]).all() == sign
        assert_is_the_twin(c, got)


def test_an_objects_result_does_not_depend_on_the_other_objects():
    c = conv_case((3, 4, 9, 10, 20, 4, 2))
    whole = run(c)
    for n in range(3):
        one = dict(c, x=c["x"][n:n + 1].copy(), g=c["g"][n:n + 1].copy())
        out, first, gx, _, _ = run(one)
        assert np.array_equal(_bits(out), _bits(whole[0][n:n + 1])) and np.array_equal(first, whole[1][n:n + 1])
        assert np.array_equal(_bits(gx), _bits(whole[2][n:n + 1]))


def test_three_calls_give_equal_bits():
    c = conv_case((1, 4, 128, 128, 4, 4, 1))           # 16 chunks
    runs = [run(c) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_x_without_a_gradient_runs_no_input_gradient_launch(monkeypatch):
    c = conv_case((2, 3, 5, 7, 1, 3, 1))
    lib, calls = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(lib, name)

            def wrapped(*args):
                calls.append(name)
                return fn(*args)
            return wrapped
    monkeypatch.setattr(_lib, "_lib", Recorder())
    out, first, gx, gw, gb = run(c, x_grad=False)
    assert gx is None and calls.count("ctpvae_conv_bwd_weight_f32") == 1
    assert "ctpvae_conv_bwd_input_f32" not in calls and "ctpvae_periodic_pad_bwd_f32" not in calls
    assert_is_the_twin(c, (out, first, None, gw, gb))
    del calls[:]
    run(c)
    assert calls.count("ctpvae_conv_bwd_input_f32") == 1 and calls.count("ctpvae_periodic_pad_bwd_f32") == 1
    # weight and bias without a gradient: no weight launch, no workspace
    del calls[:]
    x = torch.from_numpy(c["x"]).to(_dev()).requires_grad_(True)
    out = periodic_conv_maxout(x, torch.from_numpy(c["w"]).to(_dev()), torch.from_numpy(c["b"]).to(_dev()), c["s"], c["pads"])
    gx, = torch.autograd.grad(out, x, torch.from_numpy(c["g"]).to(_dev()))
    assert "ctpvae_conv_bwd_weight_f32" not in calls and np.array_equal(_bits(gx.cpu().numpy()), _bits(c["gx"]))


def test_saves_x_weight_and_one_byte_per_output_element():
    c = conv_case((2, 6, 12, 12, 1, 4, 1))
    x = torch.from_numpy(c["x"]).to(_dev()).requires_grad_(True)
    w = torch.from_numpy(c["w"]).to(_dev()).requires_grad_(True)
    out = periodic_conv_maxout(x, w, torch.from_numpy(c["b"]).to(_dev()), c["s"], c["pads"])
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].data_ptr() == x.data_ptr() and saved[1].data_ptr() == w.data_ptr()
    assert saved[2].dtype == torch.uint8 and saved[2].shape == out.shape


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_id)
def test_within_the_bars_of_the_default_block_in_float64_on_the_device(case):
    """The default ConvBlock (trainer._PeriodicPad, torch's convolution, trainer._Maxout) in float64 on the same parameters: out within
    the larger of the two halves' bars; the three gradients within their bars of autograd.grad(y64, (x, w, b), gy64) with gy64 built
    from the DEVICE's own first, so no element is left out near a tie."""
    N, Cin, H, W, C, k, s = case
    c = conv_case(case)
    out, first, gx, gw, gb = run(c)
    dev = _dev()
    blk = tr.ConvBlock(Cin, C, k, s, False).to(dev).double()
    with torch.no_grad():
        blk.ab.weight.copy_(torch.from_numpy(c["w"]).double())
        blk.ab.bias.copy_(torch.from_numpy(c["b"]).double())
    x64 = torch.from_numpy(c["x"]).to(dev).double().requires_grad_(True)
    out64 = blk(x64)
    ybar = tw.forward_bar(c["x"], c["w"], c["b"], s, c["pads"])
    assert (np.abs(out - out64.detach().cpu().numpy()) <= np.maximum(ybar[:, :C], ybar[:, C:])).all()
    y64 = blk.ab(tr._PeriodicPad.apply(x64, c["pads"]))
    gy64 = torch.from_numpy(cb.maxout_bwd(c["g"], first.astype(bool))).to(dev).double()
    gx64, gw64, gb64 = torch.autograd.grad(y64, (x64, blk.ab.weight, blk.ab.bias), gy64)
    gw_bar, gb_bar = tw.weight_grad_bar(c["x"], c["g"], first.astype(bool), k, s, c["pads"])
    assert (np.abs(gw - gw64.cpu().numpy()) <= gw_bar).all() and (np.abs(gb - gb64.cpu().numpy()) <= gb_bar).all()
    assert (np.abs(gx - gx64.cpu().numpy()) <= tw.input_grad_bar(c["g"], first.astype(bool), c["w"], (H, W), s, c["pads"])).all()


def test_convblock_with_fused_conv_and_dropout_is_dropout_pad_then_the_convolution():
    """A block with fused_conv under --dp: the bits of dropout_pad followed by the fused convolution on the padded tensor with no
    pads, in out and in the input's gradient."""
    from ct_pvae_amd import dropout_pad
    dev = _dev()
    torch.manual_seed(7)
    key = tr.DropoutKey(0.25, 12345)
    key.draw, key.first_object = 3, 0
    blk = tr.ConvBlock(3, 4, 4, 2, False, fused_conv=True, dropout=key, layer=5).to(dev).train()
    x = torch.randn(2, 3, 9, 10, device=dev, requires_grad=True)
    out = blk(x)
    cot = torch.randn_like(out)
    gx, = torch.autograd.grad(out, x, cot)
    pads = tw.block_pads(9, 10, 4, 2)
    x2 = x.detach().clone().requires_grad_(True)
    padded = dropout_pad(x2, pads, 0.25, seed=12345, draw=3, layer=5, first_object=0)
    ref = periodic_conv_maxout(padded, blk.ab.weight, blk.ab.bias, 2, (0, 0, 0, 0))
    gx2, = torch.autograd.grad(ref, x2, cot)
    assert torch.equal(out, ref) and (padded == 0).any()
    assert np.array_equal(_bits(gx.cpu().numpy()), _bits(gx2.cpu().numpy()))


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 --normal -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def test_fused_conv_training_runs_are_bit_equal_and_checkpoints_cross_the_flag(tmp_path):
    runs = []
    was = torch.backends.cudnn.deterministic            # (--reproducible switches it on for the process: put back for the tests that follow)
    try:
        for _ in range(2):
            t = _small_trainer("--reproducible --fused_head --fused_latents --fused_conv")
            blocks = [m for net in (t.enc, t.dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
            assert blocks and all(m.fused_conv for m in blocks) and any(m.transpose for m in blocks)
            losses, _ = t.train()
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses), losses
            runs.append((losses, [p.detach().clone() for p in t.params], t))
        print("losses", runs[0][0], runs[1][0])
        assert runs[0][0] == runs[1][0]
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
        path = str(tmp_path / "ckpt" / "ckpt-3.pt")
        runs[0][2].save(path, runs[0][0])
        plain = _small_trainer("--reproducible --fused_head --fused_latents")
        assert not any(m.fused_conv for net in (plain.enc, plain.dec) for m in net.modules() if isinstance(m, tr.ConvBlock))
        plain.restore(path)
        assert all(torch.equal(p, q) for p, q in zip(plain.params, runs[0][1]))
        assert math.isfinite(plain.train_step())
    finally:
        torch.backends.cudnn.deterministic = was
