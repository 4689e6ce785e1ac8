"""The fused transposed ConvBlock on the device (ct_pvae_amd/conv_transpose.py, csrc/conv_transpose.hip) against
tests/np_twin_conv_transpose.py BY BITS -- out, first, gx, gw and gb --, the matrix instruction's lane maps with exact integers,
planted ties, a NaN, an infinite cotangent, the tail rule, object independence, run-to-run equality, the skipped launches, torch's
float64 transposed block on the device within the twin's bars, and the trainer with --fused_conv --fused_convt and no --reproducible."""
import math

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, conv_transpose, conv_transpose_maxout
from ct_pvae_amd import trainer as tr
from tests import np_twin_conv_transpose as tw
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
    pad, opad = tw.block_pad(k, s)
    gshape = (N, C) + tw.out_hw(H, W, k, s, pad, opad)
    if integers:          # small, asymmetric, exact: every sum is an integer below 2^24 whatever its order
        x = rng.integers(-3, 4, (N, Cin, H, W)).astype(np.float32)
        w = rng.integers(-2, 3, (Cin, 2 * C, k, k)).astype(np.float32)
        b = rng.integers(-5, 6, 2 * C).astype(np.float32)
        g = rng.integers(-2, 3, gshape).astype(np.float32)
    else:
        x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
        w = (rng.standard_normal((Cin, 2 * C, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
        b = (0.1 * rng.standard_normal(2 * C)).astype(np.float32)
        g = rng.standard_normal(gshape).astype(np.float32)
    return dict(x=x, w=w, b=b, g=g, s=s, k=k, pad=pad, opad=opad)


def twin(c):
    """The twin's five results of one set of operands, added to the dict."""
    out, first = tw.forward(c["x"], c["w"], c["b"], c["s"], c["pad"], c["opad"])
    gw = tw.weight_grad(c["x"], c["g"], first, c["k"], c["s"], c["pad"])
    gb = tw.bias_grad(c["g"], first)
    gx = tw.input_grad(c["g"], first, c["w"], c["x"].shape[2:], c["s"], c["pad"])
    c.update(out=out, first=first, gw=gw, gb=gb, gx=gx)
    return c


def convt_case(case):
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
    _, first = conv_transpose._conv_transpose_maxout_with_first(x, w, b, c["s"], c["pad"], c["opad"])
    out = conv_transpose_maxout(x, w, b, c["s"], c["pad"], c["opad"])
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
    c = convt_case(case)
    assert c["gx"].shape == c["x"].shape
    assert_is_the_twin(c, run(c))


@pytest.mark.parametrize("case", [(3, 4, 9, 10, 20, 4, 2), (1, 3, 3, 4, 3, 3, 2), (1, 66, 3, 5, 3, 4, 2)], ids=tw.case_id)
def test_lane_maps_with_exact_integers(case):
    """Small asymmetric integer operands: every sum is exact in any order, so a row / column swap, a transposed accumulator tile, a
    k-pair fed to the wrong half or a tap of the wrong phase shows against an integer evaluation (float64 conv_transpose2d on the
    CPU is exact here), apart from any question of rounding.  2C = 40 straddles a 32-row tile; k = 3, s = 2 with opad = 1 has phases
    of unequal length; 66 input channels are three column tiles of the weight gradient and three row tiles of the input gradient."""
    N, Cin, H, W, C, k, s = case
    c = operands(case, integers=True)
    x64 = torch.from_numpy(c["x"]).double().requires_grad_(True)
    w64 = torch.from_numpy(c["w"]).double().requires_grad_(True)
    b64 = torch.from_numpy(c["b"]).double().requires_grad_(True)
    y = torch.nn.functional.conv_transpose2d(x64, w64, b64, stride=s, padding=c["pad"], output_padding=c["opad"])
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
    c = operands((2, 3, 5, 7, 2, 4, 2))
    c["w"][:, 2:], c["b"][2:] = c["w"][:, :2], c["b"][:2]
    twin(c)
    got = run(c)
    assert got[1].all() and c["first"].all()
    assert not _bits(got[3][:, 2:]).any() and not _bits(got[4][2:]).any() and got[3][:, :2].any() and got[4][:2].any()
    assert_is_the_twin(c, got)


def test_a_nan_in_x_reaches_exactly_the_outputs_whose_valid_taps_read_it():
    """x[1, 2, 3, 4] = NaN with k = 4, s = 2, pad = 1: the outputs (oy, ox) of object 1 with 0 <= oy + 1 - 2 * 3 < 4 and
    0 <= ox + 1 - 2 * 4 < 4, in every channel and both halves -- the comparison is false there and the second half is taken; no other
    output, and no output of object 0."""
    c = operands((2, 3, 5, 7, 2, 4, 2))
    c["x"][1, 2, 3, 4] = np.nan
    twin(c)
    want = np.zeros(c["out"].shape, bool)
    want[1, :, 5:9, 7:11] = True
    assert want[1, 0].sum() == 16
    got = run(c)
    assert np.array_equal(np.isnan(got[0]), want) and np.array_equal(np.isnan(c["out"]), want) and not got[1][want].any()
    assert_is_the_twin(c, got)


def test_an_infinite_cotangent_goes_to_one_half_by_selection():
    """An infinite cotangent goes to the half that was taken as inf and to the other as +0, by selection: no NaN in any gradient."""
    c = operands((2, 3, 5, 7, 2, 4, 2))
    c["g"][0, 1, 2, 3] = np.inf
    c["g"][1, 0, 9, 13] = -np.inf
    twin(c)
    got = run(c)
    assert_is_the_twin(c, got)
    assert not any(np.isnan(a).any() for a in got[2:])
    assert np.isinf(got[2]).any() and np.isinf(got[3]).any() and np.isinf(got[4]).sum() == 2


def test_tail_rule_turns_a_negative_zero_into_a_positive_one():
    """A -0 bias, a zero input and negative weights give -0 products.  k = 3, s = 2, Cin = 1: the pixels whose phase has an odd
    number of taps (1) end on +0 through the closing fma(+0, +0, acc), those with 2 or 4 taps keep -0 -- in ONE call.  With Cin = 2
    every chain is even and every pixel keeps -0.  Both are the twin's bits."""
    oy, ox = np.arange(6)[:, None], np.arange(6)[None, :]
    taps = np.where((oy + 1) % 2 == 0, 2, 1) * np.where((ox + 1) % 2 == 0, 2, 1)
    for cin in (1, 2):
        c = dict(x=np.zeros((1, cin, 3, 3), np.float32), w=-np.ones((cin, 2, 3, 3), np.float32), b=np.array([-0.0, -0.0], np.float32),
                 g=np.ones((1, 1, 6, 6), np.float32), s=2, k=3, pad=1, opad=1)
        twin(c)
        got = run(c)
        assert np.array_equal(np.signbit(got[0][0, 0]), (cin * taps) % 2 == 0)
        assert_is_the_twin(c, got)


def test_an_objects_result_does_not_depend_on_the_other_objects():
    c = convt_case((3, 4, 9, 10, 20, 4, 2))
    whole = run(c)
    for n in range(3):
        one = dict(c, x=c["x"][n:n + 1].copy(), g=c["g"][n:n + 1].copy())
        out, first, gx, _, _ = run(one)
        assert np.array_equal(_bits(out), _bits(whole[0][n:n + 1])) and np.array_equal(first, whole[1][n:n + 1])
        assert np.array_equal(_bits(gx), _bits(whole[2][n:n + 1]))


def test_three_calls_give_equal_bits():
    c = convt_case((1, 2, 64, 64, 2, 4, 2))            # 4 chunks of m, 16 of mo
    runs = [run(c) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_gradients_that_are_not_needed_run_no_launch(monkeypatch):
    c = convt_case((2, 3, 5, 7, 1, 4, 2))
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
    assert gx is None and calls.count("ctpvae_convt_bwd_weight_f32") == 1 and "ctpvae_convt_bwd_input_f32" not in calls
    assert_is_the_twin(c, (out, first, None, gw, gb))
    del calls[:]
    run(c)
    assert calls.count("ctpvae_convt_bwd_input_f32") == 1 and calls.count("ctpvae_convt_bwd_weight_f32") == 1
    assert not any("periodic_pad" in name or "_conv_" in name for name in calls)           # there is no pad to fold
    # weight and bias without a gradient: neither weight launch, no workspace
    del calls[:]
    x = torch.from_numpy(c["x"]).to(_dev()).requires_grad_(True)
    out = conv_transpose_maxout(x, torch.from_numpy(c["w"]).to(_dev()), torch.from_numpy(c["b"]).to(_dev()), c["s"], c["pad"], c["opad"])
    gx, = torch.autograd.grad(out, x, torch.from_numpy(c["g"]).to(_dev()))
    assert "ctpvae_convt_bwd_weight_f32" not in calls and "ctpvae_convt_wgrad_workspace_bytes" not in calls
    assert calls.count("ctpvae_convt_bwd_input_f32") == 1 and np.array_equal(_bits(gx.cpu().numpy()), _bits(c["gx"]))


def test_saves_x_weight_and_one_byte_per_output_element():
    c = convt_case((2, 3, 5, 7, 1, 4, 2))
    x = torch.from_numpy(c["x"]).to(_dev()).requires_grad_(True)
    w = torch.from_numpy(c["w"]).to(_dev()).requires_grad_(True)
    out = conv_transpose_maxout(x, w, torch.from_numpy(c["b"]).to(_dev()), c["s"], c["pad"], c["opad"])
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[0].data_ptr() == x.data_ptr() and saved[1].data_ptr() == w.data_ptr()
    assert saved[2].dtype == torch.uint8 and saved[2].shape == out.shape


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_id)
def test_within_the_bars_of_the_default_block_in_float64_on_the_device(case):
    """The default transposed ConvBlock (torch's ConvTranspose2d, trainer._Maxout) in float64 on the same parameters: out within the
    larger of the two halves' bars; the three gradients within their bars of autograd.grad(y64, (x, w, b), gy64) with gy64 built from
    the DEVICE's own first, so no element is left out near a tie.  The cases include the toy recipe's --ks 2 --se 1 block."""
    N, Cin, H, W, C, k, s = case
    c = convt_case(case)
    out, first, gx, gw, gb = run(c)
    dev = _dev()
    blk = tr.ConvBlock(Cin, C, k, s, True).to(dev).double()
    assert (blk.ab.padding[0], blk.ab.output_padding[0]) == (c["pad"], c["opad"])
    with torch.no_grad():
        blk.ab.weight.copy_(torch.from_numpy(c["w"]).double())
        blk.ab.bias.copy_(torch.from_numpy(c["b"]).double())
    x64 = torch.from_numpy(c["x"]).to(dev).double().requires_grad_(True)
    out64 = blk(x64)
    ybar = tw.forward_bar(c["x"], c["w"], c["b"], s, c["pad"], c["opad"])
    assert out64.shape == out.shape
    assert (np.abs(out - out64.detach().cpu().numpy()) <= np.maximum(ybar[:, :C], ybar[:, C:])).all()
    y64 = blk.ab(x64)
    gy64 = torch.from_numpy(cb.maxout_bwd(c["g"], first.astype(bool))).to(dev).double()
    gx64, gw64, gb64 = torch.autograd.grad(y64, (x64, blk.ab.weight, blk.ab.bias), gy64)
    assert (np.abs(gw - gw64.cpu().numpy()) <= tw.weight_grad_bar(c["x"], c["g"], first.astype(bool), k, s, c["pad"])).all()
    assert (np.abs(gb - gb64.cpu().numpy()) <= tw.bias_grad_bar(c["g"], first.astype(bool))).all()
    assert (np.abs(gx - gx64.cpu().numpy()) <= tw.input_grad_bar(c["g"], first.astype(bool), c["w"], (H, W), s, c["pad"])).all()


def test_the_ks2_se1_decoder_crops_the_fused_block_as_the_default_one():
    """The toy recipe's --ks 2 --se 1: the transposed block's output is one pixel larger than the skip and DecodeNet crops it.  What
    reaches the head of a decoder with fused_convt is the operator's output cropped as DecodeNet.forward crops it, by bits, next to the
    skip; and it lies within the twin's forward bars of what reaches the head of the default decoder in float64."""
    dev = _dev()
    torch.manual_seed(11)
    dec = tr.DecodeNet([4, 6], 2, 1, 2, 1, 0, 2, fused_convt=True).to(dev)
    plain = tr.DecodeNet([4, 6], 2, 1, 2, 1, 0, 2).to(dev)
    plain.load_state_dict(dec.state_dict(), strict=True)
    plain.double()
    lat = [torch.randn(2, 2, 4, 6, device=dev), torch.randn(2, 3, 4, 6, device=dev)]
    up = dec.ups[0][0]
    assert up.transpose and up.fused_convt and (up.ab.stride[0], up.ab.padding[0], up.ab.output_padding[0]) == (1, 0, 0)
    full = conv_transpose_maxout(lat[-1], up.ab.weight, up.ab.bias, 1, 0, 0)
    assert tuple(full.shape) == (2, 4, 5, 7)
    seen = []
    handles = [net.head.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].detach())) for net in (dec, plain)]
    alpha, beta = dec(lat)
    alpha64, beta64 = plain([t.double() for t in lat])
    for h in handles:
        h.remove()
    assert tuple(alpha.shape) == tuple(beta.shape) == tuple(alpha64.shape) == (2, 1, 4, 6)
    assert torch.equal(seen[0][:, :4], full[..., 1:5, 1:7]) and torch.equal(seen[0][:, 4:], lat[0])
    ybar = tw.forward_bar(lat[-1].cpu().numpy(), up.ab.weight.detach().cpu().numpy(), up.ab.bias.detach().cpu().numpy(), 1, 0, 0)
    bar = np.maximum(ybar[:, :4], ybar[:, 4:])[..., 1:5, 1:7]
    assert (np.abs(seen[0][:, :4].cpu().numpy() - seen[1][:, :4].cpu().numpy()) <= bar).all()


def test_convblock_with_fused_convt_and_dropout_is_dropout_then_the_operator():
    """A transposed block with fused_convt under --dp: the bits of convblock.dropout followed by the operator, in out and in the
    input's gradient."""
    from ct_pvae_amd import dropout
    dev = _dev()
    torch.manual_seed(7)
    key = tr.DropoutKey(0.25, 12345)
    key.draw, key.first_object = 3, 0
    blk = tr.ConvBlock(3, 4, 4, 2, True, fused_convt=True, dropout=key, layer=5).to(dev).train()
    x = torch.randn(2, 3, 9, 10, device=dev, requires_grad=True)
    out = blk(x)
    assert tuple(out.shape) == (2, 4, 18, 20)
    cot = torch.randn_like(out)
    gx, = torch.autograd.grad(out, x, cot)
    x2 = x.detach().clone().requires_grad_(True)
    dropped = dropout(x2, 0.25, seed=12345, draw=3, layer=5, first_object=0)
    ref = conv_transpose_maxout(dropped, blk.ab.weight, blk.ab.bias, 2, 1, 0)
    gx2, = torch.autograd.grad(ref, x2, cot)
    assert torch.equal(out, ref) and (dropped == 0).any()
    assert np.array_equal(_bits(gx.cpu().numpy()), _bits(gx2.cpu().numpy()))


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _small_trainer(extra=""):
    args = tr.get_args(("--nsa 20 --td 6 -b 3 --ns 2 --api 10 --pnm 1e4 --normal -i 3 --train " + extra).split())
    return tr.PVAETrainer(args, _dev())


def _refuse_torch_convolution(module, inputs):
    raise AssertionError("a torch convolution ran in a network built with --fused_conv --fused_convt")


def test_training_is_bit_equal_without_the_deterministic_switch_and_checkpoints_cross_the_flag(tmp_path):
    """--fused_conv --fused_convt without --reproducible: torch.backends.cudnn.deterministic stays False, no ConvBlock.ab runs (a
    forward pre-hook on each raises), two runs of 3 steps give equal losses and equal parameters bit for bit, and a checkpoint
    written with the flag restores into a trainer without it, which steps."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = False
    try:
        runs = []
        for _ in range(2):
            t = _small_trainer("--fused_head --fused_latents --fused_conv --fused_convt")
            blocks = [m for net in (t.enc, t.dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
            assert blocks and all(m.fused_conv and m.fused_convt for m in blocks) and any(m.transpose for m in blocks)
            for m in blocks:
                m.ab.register_forward_pre_hook(_refuse_torch_convolution)
            losses, _ = t.train()
            assert torch.backends.cudnn.deterministic is False
            assert len(losses) == 3 and all(math.isfinite(v) for v in losses), losses
            runs.append((losses, [p.detach().clone() for p in t.params], t))
        print("losses", runs[0][0], runs[1][0])
        assert runs[0][0] == runs[1][0]
        assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
        path = str(tmp_path / "ckpt" / "ckpt-3.pt")
        runs[0][2].save(path, runs[0][0])
        plain = _small_trainer("--fused_head --fused_latents --fused_conv")
        blocks = [m for net in (plain.enc, plain.dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
        assert not any(m.fused_convt for m in blocks) and any(m.transpose for m in blocks)
        plain.restore(path)
        assert all(torch.equal(p, q) for p, q in zip(plain.params, runs[0][1]))
        assert math.isfinite(plain.train_step())
        assert torch.backends.cudnn.deterministic is False
    finally:
        torch.backends.cudnn.deterministic = was
