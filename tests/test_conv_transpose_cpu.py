"""Host side of the fused transposed ConvBlock (ct_pvae_amd/conv_transpose.py, csrc/conv_transpose.hip):
tests/np_twin_conv_transpose.py against torch's float64 conv_transpose2d and its autograd on the CPU within the twin's own error
bars, the twin's tail rule and selection, the entry points' and the wrapper's argument checks, the workspace rule, the ABI table, the
trainer's flag, the block's unchanged state_dict and the kernels' register budget.  The kernels themselves:
tests/test_gpu_conv_transpose.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_conv_transpose as tw
from tests import np_twin_convblock as cb
from tests.conftest import ROOT

NEW_SYMBOLS = ("ctpvae_convt_wgrad_workspace_bytes", "ctpvae_convt_fwd_f32", "ctpvae_convt_bwd_weight_f32", "ctpvae_convt_bwd_input_f32")


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def _operands(case):
    N, Cin, H, W, C, k, s = case
    rng = np.random.default_rng(sum(case) + 17 * k)
    pad, opad = tw.block_pad(k, s)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cin, 2 * C, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(2 * C)).astype(np.float32)
    g = rng.standard_normal((N, C) + tw.out_hw(H, W, k, s, pad, opad)).astype(np.float32)
    return x, w, b, pad, opad, g


def test_block_pad_is_the_convblocks_rule_and_the_chunk_cases_sit_on_the_edges():
    from ct_pvae_amd import trainer as tr
    for k, s in ((4, 2), (2, 1), (3, 2), (4, 1), (5, 3), (8, 2), (1, 1), (3, 3), (2, 2), (8, 8), (7, 2), (3, 1)):
        ab = tr.ConvBlock(1, 1, k, s, True).ab
        assert tw.block_pad(k, s) == (ab.padding[0], ab.output_padding[0]), (k, s)
        assert 0 <= ab.padding[0] < k and 0 <= ab.output_padding[0] < s
    assert tw.block_pad(3, 2) == (1, 1) and tw.block_pad(2, 1) == (0, 0) and tw.block_pad(8, 2) == (3, 0)
    sizes = []
    for N, Cin, H, W, C, k, s in tw.CHUNK_CASES:
        OH, OW = tw.out_hw(H, W, k, s, *tw.block_pad(k, s))
        sizes.append((N * H * W, N * OH * OW))
    assert sizes == [(1023, 1023), (1024, 1024), (1025, 1025), (256, 1024), (960, 1025)]
    assert tw.out_hw(4, 6, 2, 1, 0, 0) == (5, 7)                       # --ks 2 --se 1: one pixel larger than the input
    N, Cin, H, W, C, k, s = tw.CASES[-1]
    assert tw.chunks_of(N * H * W) == 4 and tw.chunks_of(N * 128 * 128) == 16


@pytest.mark.parametrize("case", tw.CASES + tw.CHUNK_CASES, ids=tw.case_id)
def test_twin_lies_within_its_bars_of_float64(case):
    """conv_transpose2d in float64, the maxout by the TWIN's own selection (so no element has to be left out near a tie),
    autograd.grad for the three gradients."""
    N, Cin, H, W, C, k, s = case
    x, w, b, pad, opad, g = _operands(case)
    y = tw.conv_y(x, w, b, s, pad, opad)
    out, first = tw.forward(x, w, b, s, pad, opad)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    b64 = torch.from_numpy(b).double().requires_grad_(True)
    y64 = torch.nn.functional.conv_transpose2d(x64, w64, b64, stride=s, padding=pad, output_padding=opad)
    assert tuple(y64.shape) == y.shape == (N, 2 * C) + tw.out_hw(H, W, k, s, pad, opad)
    assert (np.abs(y - y64.detach().numpy()) <= tw.forward_bar(x, w, b, s, pad, opad)).all()
    assert np.array_equal(out, np.where(first, y[:, :C], y[:, C:]))
    gx64, gw64, gb64 = torch.autograd.grad(y64, (x64, w64, b64), torch.from_numpy(cb.maxout_bwd(g, first)).double())
    gw, gb = tw.weight_grad(x, g, first, k, s, pad), tw.bias_grad(g, first)
    assert gw.shape == w.shape and gb.shape == b.shape and gw.dtype == gb.dtype == np.float32
    assert (np.abs(gw - gw64.numpy()) <= tw.weight_grad_bar(x, g, first, k, s, pad)).all()
    assert (np.abs(gb - gb64.numpy()) <= tw.bias_grad_bar(g, first)).all()
    gx = tw.input_grad(g, first, w, (H, W), s, pad)
    assert gx.shape == x.shape and gx.dtype == np.float32
    assert (np.abs(gx - gx64.numpy()) <= tw.input_grad_bar(g, first, w, (H, W), s, pad)).all()


def test_twin_tail_rule_and_selection():
    """A chain of odd length with a -0 bias and -0 products: the closing fma(+0, +0, acc) turns -0 into +0; an even chain keeps it.
    k = 3, s = 2, Cin = 1 has phases of 1, 2 and 4 taps: both in ONE call, by the pixel's phase.  Equal halves tie everywhere:
    first is all ones and the second half's gradients are +0."""
    mz = np.array([-0.0, -0.0], np.float32)
    y1 = tw.conv_y(np.zeros((1, 1, 2, 2), np.float32), np.ones((1, 2, 1, 1), np.float32), mz, 1, 0, 0)
    assert not np.signbit(y1).any()
    y2 = tw.conv_y(np.zeros((1, 2, 2, 2), np.float32), np.ones((2, 2, 1, 1), np.float32), mz, 1, 0, 0)
    assert y2.shape == (1, 2, 2, 2) and not np.signbit(y2).any()       # (+0) * 1 = +0 products: -0 + +0 = +0 either way
    y2 = tw.conv_y(np.zeros((1, 2, 2, 2), np.float32), -np.ones((2, 2, 1, 1), np.float32), mz, 1, 0, 0)
    assert np.signbit(y2).all()                                        # an even chain of -0 products keeps -0
    y3 = tw.conv_y(np.zeros((1, 1, 3, 3), np.float32), -np.ones((1, 2, 3, 3), np.float32), mz, 2, 1, 1)
    assert y3.shape == (1, 2, 6, 6)
    oy, ox = np.arange(6)[:, None], np.arange(6)[None, :]
    taps = np.where((oy + 1) % 2 == 0, 2, 1) * np.where((ox + 1) % 2 == 0, 2, 1)      # phase 0 has taps 0 and 2, phase 1 has tap 1
    assert np.array_equal(np.signbit(y3[0, 0]), taps % 2 == 0) and np.array_equal(np.signbit(y3[0, 1]), taps % 2 == 0)
    case = (2, 3, 5, 7, 2, 4, 2)
    x, w, b, pad, opad, g = _operands(case)
    w[:, 2:], b[2:] = w[:, :2], b[:2]
    _, first = tw.forward(x, w, b, 2, pad, opad)
    assert first.all()
    gw, gb = tw.weight_grad(x, g, first, 4, 2, pad), tw.bias_grad(g, first)
    assert not gw[:, 2:].view(np.uint32).any() and not gb[2:].view(np.uint32).any() and gw[:, :2].any() and gb[:2].any()


def test_bad_arguments_are_einval_before_any_hip_call(lib):
    L = lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # (host pointers: every call below is refused before a pointer is used or a HIP call is made)
    #       N  Cin H  W  C  k  s  pad opad
    geom = [2, 3, 5, 7, 2, 4, 2, 1, 0]
    calls = ((L.ctpvae_convt_fwd_f32, [p, p, p], [p, p, None], (0, 1, 2, 12, 13)),
             (L.ctpvae_convt_bwd_weight_f32, [p, p, p], [p, p, p, None], (0, 1, 2, 12, 13, 14)),
             (L.ctpvae_convt_bwd_input_f32, [p, p, p], [p, None], (0, 1, 2, 12)))
    for fn, head, tail, pointers in calls:
        for i in pointers:
            bad = head + geom + tail
            bad[i] = None
            assert fn(*bad) == lib.EINVAL and "null" in lib.last_error(), (fn.__name__, i)

    def refused(g, word):
        for fn, head, tail, _ in calls:
            assert fn(*(head + list(g) + tail)) == lib.EINVAL and word in lib.last_error(), (fn.__name__, g, lib.last_error())
        assert L.ctpvae_convt_wgrad_workspace_bytes(*g) == lib.EINVAL and word in lib.last_error(), (g, lib.last_error())
    for i in range(5):
        for v in (0, -1):
            refused(geom[:i] + [v] + geom[i + 1:], "at least 1")
    for k in (0, 9):
        refused(geom[:5] + [k, 1, 0, 0], "kernel size")
    for s in (0, 5):
        refused(geom[:6] + [s, 1, 0], "stride")
    for pad in (-1, 4):
        refused(geom[:7] + [pad, 0], "padding")
    for opad in (-1, 2):
        refused(geom[:8] + [opad], "output padding")
    refused([1, 1, 1, 1, 1, 2, 1, 1, 0], "at least one pixel")           # OH = 0 * 1 - 2 + 2 = 0
    refused([1, 1, 1, 5, 1, 3, 1, 2, 0], "at least one pixel")           # OH = -1 while OW = 3
    for g in ([2 ** 15, 2 ** 8, 2 ** 8, 1, 1, 1, 1, 0, 0],               # N * Cin * H * W = 2^31
              [1, 1, 2 ** 15, 2 ** 15, 1, 1, 1, 0, 0],                   # only the 2C-channel output
              [1, 1, 2 ** 14, 2 ** 14, 1, 2, 2, 0, 0],                   # only the output, which the stride makes larger
              [1, 2 ** 20, 8, 8, 2 ** 10, 1, 1, 0, 0],                   # only the weights
              [2 ** 31 - 1] * 5 + [8, 8, 0, 0]):
        refused(g, "31 bits")
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL, "convt")


def test_workspace_rule_at_its_edges(lib):
    """4 * (ceil(N * H * W / chunk) * Cin * 2C * k * k + ceil(N * OH * OW / chunk) * 2C) bytes: a function of the shapes alone."""
    L = lib.load()
    assert L.ctpvae_conv_wgrad_chunk_len() == tw.CHUNK == 1024
    for case, (wc, bc) in zip(tw.CHUNK_CASES, ((1, 1), (1, 1), (2, 2), (1, 1), (1, 2))):
        N, Cin, H, W, C, k, s = case
        assert L.ctpvae_convt_wgrad_workspace_bytes(*case, *tw.block_pad(k, s)) == 4 * (wc * 2 * k * k + bc * 2), case
    assert L.ctpvae_convt_wgrad_workspace_bytes(1, 1, 1, 1, 1, 1, 1, 0, 0) == 16
    # c3's largest transposed layer: 60 -> 2 * 4 at 64 x 64, ten objects, k = 4: 40 chunks of m, 160 chunks of mo
    assert L.ctpvae_convt_wgrad_workspace_bytes(10, 60, 64, 64, 4, 4, 2, 1, 0) == 4 * (40 * 60 * 8 * 16 + 160 * 8)
    for case in tw.CASES:
        N, Cin, H, W, C, k, s = case
        pad, opad = tw.block_pad(k, s)
        OH, OW = tw.out_hw(H, W, k, s, pad, opad)
        want = 4 * (tw.chunks_of(N * H * W) * Cin * 2 * C * k * k + tw.chunks_of(N * OH * OW) * 2 * C)
        assert L.ctpvae_convt_wgrad_workspace_bytes(*case, pad, opad) == want, case
    # a workspace past 2^31 - 1 floats is refused although every tensor fits: 1024 chunks x 32 x 1024 x 64 floats
    assert L.ctpvae_convt_wgrad_workspace_bytes(1, 32, 1024, 1024, 512, 8, 1, 4, 0) == lib.EINVAL
    assert "must fit 31 bits" in lib.last_error() and "chunks" in lib.last_error()
    assert L.ctpvae_convt_wgrad_workspace_bytes(1, 32, 1024, 1024, 8, 8, 1, 4, 0) == 4 * (1024 * 32 * 16 * 64 + 1023 * 16)


def test_header_library_and_binding_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctpvae_radon.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ctpvae_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in lib.SIGNATURES, name
    assert {n for n in declared if "_convt_" in n} == {n for n in exported if "_convt_" in n} == set(NEW_SYMBOLS)
    assert lib.load().ctpvae_abi_version() == lib.ABI_VERSION == 3400
    make = open(os.path.join(ROOT, "ct_pvae_amd", "csrc", "Makefile")).read()
    assert "conv_transpose.hip" in make and "conv_tile.h" in make


def test_python_wrapper_refuses_what_it_cannot_run(lib):
    import ct_pvae_amd
    from ct_pvae_amd import conv_transpose
    fn = ct_pvae_amd.conv_transpose_maxout
    assert fn is conv_transpose.conv_transpose_maxout
    x, w, b = torch.zeros(2, 3, 5, 7), torch.zeros(3, 4, 4, 4), torch.zeros(4)
    for bad in ((x.numpy(), w, b), (x, w.numpy(), b), (x, w, b.numpy()), (x.double(), w, b), (x, w.double(), b), (x, w, b.double())):
        with pytest.raises(TypeError):
            fn(*bad, 2, 1, 0)
    for bad in ((2.0, 1, 0), (2, 1.0, 0), (2, 1, 0.0), (True, 1, 0), (2, (1, 1), 0)):
        with pytest.raises(TypeError):
            fn(x, w, b, *bad)
    for bad in ((x[0], w, b), (x, w[0], b), (x, w, b[None]),                           # axes
                (torch.zeros(2, 0, 5, 7), torch.zeros(0, 4, 4, 4), b),                 # empty
                (torch.zeros(2, 6, 5, 7)[:, :3], w, b),                                # not contiguous
                (x, torch.zeros(3, 4, 4, 8)[..., :4], b), (x, w, torch.zeros(8)[::2]),
                (x, torch.zeros(2, 4, 4, 4), b),                                       # Cin
                (x, torch.zeros(3, 3, 4, 4), torch.zeros(3)),                          # an odd channel count
                (x, torch.zeros(3, 4, 4, 3), b),                                       # not square
                (x, w, torch.zeros(6)),                                                # bias
                (x, torch.zeros(3, 4, 9, 9), b)):                                      # k > 8
        with pytest.raises(ValueError):
            fn(*bad, 2, 1, 0)
    for bad in ((0, 1, 0), (5, 1, 0), (2, -1, 0), (2, 4, 0), (2, 1, -1), (2, 1, 2)):
        with pytest.raises(ValueError):
            fn(x, w, b, *bad)
    with pytest.raises(ValueError, match="at least one pixel"):
        fn(torch.zeros(1, 3, 1, 1), torch.zeros(3, 4, 2, 2), b, 1, 1, 0)
    with pytest.raises(lib.RadonLibraryError, match="no CPU path"):
        fn(x, w, b, 2, 1, 0)
    with pytest.raises(lib.RadonLibraryError, match="no CPU path"):
        conv_transpose._conv_transpose_maxout_with_first(x, w, b, 2, 1, 0)


def test_fused_convt_flag():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).fused_convt is False and tr.get_args(["--normal"]).fused_convt is False              # off by default
    for flags in ("--fused_convt", "--det --fused_convt", "--normal --fused_convt --dp 0.1", "--reproducible --fused_convt",
                  "--normal --fused_head --fused_latents --fused_blocks --fused_update --fused_conv --fused_convt"):
        assert tr.get_args(flags.split()).fused_convt is True
    a = tr.get_args("--normal --fused_conv".split())
    assert a.fused_convt is False and a.fused_conv is True                # --fused_conv alone leaves the transposed blocks on torch
    a = tr.get_args("--normal --fused_convt".split())
    assert a.fused_convt is True and a.fused_conv is False                # and the other way round


def test_fused_convt_blocks_keep_their_parameters_and_names():
    from ct_pvae_amd import trainer as tr
    torch.manual_seed(3)
    plain = tr.ConvBlock(3, 4, 4, 2, True)
    torch.manual_seed(3)
    fused = tr.ConvBlock(3, 4, 4, 2, True, fused_convt=True)
    assert plain.fused_convt is False and fused.fused_convt is True and fused.fused_conv is False
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf) == ["ab.weight", "ab.bias"]
    assert [tuple(v.shape) for v in sp.values()] == [tuple(v.shape) for v in sf.values()] == [(3, 8, 4, 4), (8,)]
    assert all(torch.equal(a, b) for a, b in zip(sp.values(), sf.values()))                                  # the same initialisation
    assert (fused.ab.stride, fused.ab.padding, fused.ab.output_padding) == ((2, 2), (1, 1), (0, 0))
    nets = {}
    for flag in (False, True):
        torch.manual_seed(4)
        enc = tr.EncodeNet(2, [4, 6], 2, 4, 2, 1, 4, fused_convt=flag)
        dec = tr.DecodeNet(enc.channels, 2, 1, 4, 2, 1, 4, fused_convt=flag)
        nets[flag] = (enc, dec)
        blocks = [m for net in (enc, dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
        assert len(blocks) == 9 and all(blk.fused_convt is flag and blk.fused_conv is False for blk in blocks)
        assert sum(blk.transpose for blk in blocks) == 2
    for a, b in zip(nets[False], nets[True]):
        assert list(a.state_dict()) == list(b.state_dict())
        assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
    with pytest.raises(Exception, match="no CPU path"):
        fused(torch.zeros(1, 3, 8, 8))                      # the flag is taken: no quiet torch convolution behind it
    padded = tr.ConvBlock(3, 4, 4, 2, False, fused_convt=True)            # a non-transposed block ignores the flag
    assert tuple(padded(torch.zeros(1, 3, 8, 8)).shape) == (1, 4, 4, 4)


def test_no_conv_transpose_kernel_has_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "conv_transpose.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen, bad = None, [], []
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            seen.append(name)
            if int(m.group(1)) > 0:
                bad.append((name, int(m.group(1))))
    assert len(seen) == 4 and all("convt_" in n for n in seen), seen
    assert not bad, f"kernels with scratch (register spills): {bad}"
