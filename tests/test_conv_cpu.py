"""Host side of the fused ConvBlock convolution (ct_pvae_amd/conv.py, csrc/conv.hip): tests/np_twin_conv.py against a float64
evaluation by torch on the CPU within its own error bars, the twin's fold against np_twin_convblock's, the entry points' and the
wrapper's argument checks, the workspace rule, the ABI table, the trainer's flag, the block's unchanged state_dict and the kernels'
register budget.  The kernels themselves: tests/test_gpu_conv.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_conv as tw
from tests import np_twin_convblock as cb
from tests.conftest import ROOT

NEW_SYMBOLS = ("ctpvae_conv_wgrad_chunk_len", "ctpvae_conv_wgrad_workspace_bytes", "ctpvae_conv_fwd_f32", "ctpvae_conv_bwd_weight_f32",
               "ctpvae_conv_bwd_input_f32")


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def _operands(case):
    N, Cin, H, W, C, k, s = case
    rng = np.random.default_rng(sum(case) + 17 * k)
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((2 * C, Cin, k, k)) / np.sqrt(Cin * k * k)).astype(np.float32)
    b = (0.1 * rng.standard_normal(2 * C)).astype(np.float32)
    pads = tw.block_pads(H, W, k, s)
    g = rng.standard_normal((N, C) + tw.out_hw(H, W, k, s, pads)).astype(np.float32)
    return x, w, b, pads, g


def test_fma32_is_the_correctly_rounded_fma():
    """Against exact rational arithmetic on planted and random operands: double rounding, cancellation, a tie broken by the product's
    low bits, subnormal results, signed zeros."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (-a * b + rng.standard_normal(2000).astype(np.float32) * np.float32(1e-7)).astype(np.float32)      # heavy cancellation
    planted = [(1 + 2.0 ** -12, 1 + 2.0 ** -12, 2.0 ** 24), (1 + 2.0 ** -23, 1 - 2.0 ** -23, -1.0), (2.0 ** -80, 2.0 ** -69, 2.0 ** -149),
               (3.0, 2.0 ** -150, 2.0 ** -149), (1 + 2.0 ** -23, 1 + 2.0 ** -23, 2.0 ** 25)]
    a = np.concatenate([a, np.array([p[0] for p in planted], np.float32)])
    b = np.concatenate([b, np.array([p[1] for p in planted], np.float32)])
    c = np.concatenate([c, np.array([p[2] for p in planted], np.float32)])
    got = tw.fma32(a, b, c)
    assert got.dtype == np.float32
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):           # a tie: the even one
            assert (int(got[i:i + 1].view(np.uint32)[0]) & 1) == 0, i
    z = tw.fma32(np.float32(0), np.float32(0), np.array([-0.0, 0.0], np.float32))
    assert np.signbit(z).tolist() == [False, False]                    # the tail rule: -0 becomes +0
    assert np.signbit(tw.fma32(np.float32(-1), np.float32(0), np.float32(-0.0)))


@pytest.mark.parametrize("case", tw.CASES, ids=tw.case_id)
def test_twin_lies_within_its_bars_of_float64(case):
    """conv2d in float64 on the explicitly wrapped input, the maxout by the TWIN's own selection (so no element has to be left out
    near a tie), autograd.grad for the three gradients."""
    N, Cin, H, W, C, k, s = case
    x, w, b, pads, g = _operands(case)
    y = tw.conv_y(x, w, b, s, pads)
    out, first = tw.forward(x, w, b, s, pads)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    b64 = torch.from_numpy(b).double().requires_grad_(True)
    wl, wr, hl, hr = pads
    xp = x64[:, :, torch.from_numpy(cb.pad_index(H, hl, hr))][:, :, :, torch.from_numpy(cb.pad_index(W, wl, wr))]
    y64 = torch.nn.functional.conv2d(xp, w64, b64, stride=s)
    assert tuple(y64.shape) == y.shape == (N, 2 * C) + tw.out_hw(H, W, k, s, pads)
    bar = tw.forward_bar(x, w, b, s, pads)
    assert (np.abs(y - y64.detach().numpy()) <= bar).all()
    assert np.array_equal(out, np.where(first, y[:, :C], y[:, C:]))
    gx64, gw64, gb64 = torch.autograd.grad(y64, (x64, w64, b64), torch.from_numpy(cb.maxout_bwd(g, first)).double())
    gw, gb = tw.weight_grad(x, g, first, k, s, pads)
    gw_bar, gb_bar = tw.weight_grad_bar(x, g, first, k, s, pads)
    assert gw.shape == w.shape and gb.shape == b.shape
    assert (np.abs(gw - gw64.numpy()) <= gw_bar).all() and (np.abs(gb - gb64.numpy()) <= gb_bar).all()
    gx = tw.input_grad(g, first, w, (H, W), s, pads)
    assert gx.shape == x.shape
    assert (np.abs(gx - gx64.numpy()) <= tw.input_grad_bar(g, first, w, (H, W), s, pads)).all()


def test_twin_fold_is_the_periodic_pads_backward():
    """input_grad is padded_grad under np_twin_convblock.pad_bwd by bits, also where an axis wraps more than once; and the chunk
    cases' M are one below, at and one above the chunk length."""
    case = (1, 2, 2, 3, 3, 4, 1)
    N, Cin, H, W, C, k, s = case
    x, w, b, pads, g = _operands(case)
    assert pads == (2, 1, 2, 1) and not cb.at_most_two_copies((N, Cin, H, W), pads)
    _, first = tw.forward(x, w, b, s, pads)
    gp = tw.padded_grad(g, first, w, (H, W), s, pads)
    assert gp.shape == (N, Cin, H + 3, W + 3)
    assert np.array_equal(tw.input_grad(g, first, w, (H, W), s, pads).view(np.uint32), cb.pad_bwd(gp, (H, W), pads).view(np.uint32))
    assert [c[0] * c[2] * c[3] for c in tw.CHUNK_CASES] == [tw.CHUNK - 1, tw.CHUNK, tw.CHUNK + 1]
    assert all(tw.block_pads(c[2], c[3], 1, 1) == (0, 0, 0, 0) for c in tw.CHUNK_CASES)


def test_twin_tail_rule_and_selection():
    """K = 1 (odd) with a -0 bias and a zero input: the chain's -0 becomes +0 through the closing fma(+0, +0, acc); K = 2 keeps it.
    Equal halves tie everywhere: first is all ones and the second half's gradients are +0."""
    x = np.zeros((1, 1, 2, 2), np.float32)
    mz = np.array([-0.0, -0.0], np.float32)
    y1 = tw.conv_y(x, np.ones((2, 1, 1, 1), np.float32), mz, 1, (0, 0, 0, 0))
    assert not np.signbit(y1).any()
    y2 = tw.conv_y(np.zeros((1, 2, 2, 2), np.float32), -np.ones((2, 2, 1, 1), np.float32), mz, 1, (0, 0, 0, 0))
    assert np.signbit(y2).all()
    case = (2, 3, 5, 7, 2, 3, 1)
    x, w, b, pads, g = _operands(case)
    w[2:], b[2:] = w[:2], b[:2]
    _, first = tw.forward(x, w, b, 1, pads)
    assert first.all()
    gw, gb = tw.weight_grad(x, g, first, 3, 1, pads)
    assert not gw[2:].view(np.uint32).any() and not gb[2:].view(np.uint32).any() and gw[:2].any()


def test_bad_arguments_are_einval_before_any_hip_call(lib):
    L = lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # (host pointers: every call below is refused before a pointer is used or a HIP call is made)
    #       N  Cin H  W  C  k  s  wl wr hl hr
    geom = [2, 3, 5, 7, 2, 3, 1, 1, 1, 1, 1]
    calls = ((L.ctpvae_conv_fwd_f32, [p, p, p], [p, p, None], (0, 1, 2, 14, 15)),
             (L.ctpvae_conv_bwd_weight_f32, [p, p, p], [p, p, p, None], (0, 1, 2, 14, 15, 16)),
             (L.ctpvae_conv_bwd_input_f32, [p, p, p], [p, None], (0, 1, 2, 14)))
    for fn, head, tail, pointers in calls:
        for i in pointers:
            bad = head + geom + tail
            bad[i] = None
            assert fn(*bad) == lib.EINVAL and "null" in lib.last_error(), (fn.__name__, i)
    def refused(g, word):
        for fn, head, tail, _ in calls:
            assert fn(*(head + list(g) + tail)) == lib.EINVAL and word in lib.last_error(), (fn.__name__, g, lib.last_error())
        assert L.ctpvae_conv_wgrad_workspace_bytes(*g) == lib.EINVAL and word in lib.last_error(), (g, lib.last_error())
    for i in range(5):
        for v in (0, -1):
            refused(geom[:i] + [v] + geom[i + 1:], "at least 1")
    for k in (0, 9):
        refused(geom[:5] + [k, 1] + geom[7:], "kernel size")
    for s in (0, 4):
        refused(geom[:6] + [s] + geom[7:], "stride")
    for i in (7, 8, 9, 10):
        refused(geom[:i] + [-1] + geom[i + 1:], "negative")
    refused([1, 1, 2, 2, 1, 4, 1, 0, 0, 0, 0], "one window")
    for g in ([2 ** 15, 2 ** 8, 2 ** 8, 1, 1, 1, 1, 0, 0, 0, 0],             # N * Cin * H * W = 2^31
              [1, 1, 2 ** 15, 2 ** 15, 2, 1, 1, 0, 0, 0, 0],                 # only the 2C-channel output
              [1, 1, 2 ** 15, 2 ** 15 - 1, 1, 2, 1, 2 ** 15 + 1, 0, 0, 0],       # only the padded input
              [1, 2 ** 20, 8, 8, 2 ** 10, 1, 1, 0, 0, 0, 0],                 # only the weights
              [2 ** 31 - 1] * 5 + [8, 8, 0, 0, 0, 0]):
        refused(g, "31 bits")
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL, "conv")


def test_workspace_rule_at_its_edges(lib):
    """4 * ceil(N * OH * OW / chunk) * 2C * (Cin * k * k + 1) bytes: a function of the shapes alone."""
    L = lib.load()
    assert L.ctpvae_conv_wgrad_chunk_len() == tw.CHUNK == 1024
    for case, want_chunks in zip(tw.CHUNK_CASES, (1, 1, 2)):
        N, Cin, H, W, C, k, s = case
        assert tw.chunks_of(N * H * W) == want_chunks
        assert L.ctpvae_conv_wgrad_workspace_bytes(N, Cin, H, W, C, k, s, 0, 0, 0, 0) == 4 * want_chunks * 2 * 2
    assert L.ctpvae_conv_wgrad_workspace_bytes(1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0) == 16
    # c3's largest layer: 40 -> 80 at 64 x 64, ten objects, k = 4 with pads (2, 1, 2, 1): 40 chunks x 80 rows x 641 taps
    assert L.ctpvae_conv_wgrad_workspace_bytes(10, 40, 64, 64, 40, 4, 1, 2, 1, 2, 1) == 4 * 40 * 80 * 641
    for case in tw.CASES:
        N, Cin, H, W, C, k, s = case
        pads = tw.block_pads(H, W, k, s)
        OH, OW = tw.out_hw(H, W, k, s, pads)
        assert L.ctpvae_conv_wgrad_workspace_bytes(*case, *pads) == 4 * tw.chunks_of(N * OH * OW) * 2 * C * (Cin * k * k + 1), case
    # a workspace past 2^31 - 1 floats is refused although every tensor fits: 1024 chunks x 1024 rows x 2049 taps
    assert L.ctpvae_conv_wgrad_workspace_bytes(1, 32, 1024, 1024, 512, 8, 1, 4, 3, 4, 3) == lib.EINVAL
    assert "chunks * 2C * (K + 1) must fit 31 bits" in lib.last_error()
    assert L.ctpvae_conv_wgrad_workspace_bytes(1, 32, 1024, 1024, 256, 8, 1, 4, 3, 4, 3) == 4 * 1024 * 512 * 2049


def test_header_library_and_binding_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctpvae_radon.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ctpvae_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in lib.SIGNATURES, name
    assert {n for n in declared if "_conv_" in n} == {n for n in exported if "_conv_" in n} == set(NEW_SYMBOLS)
    assert lib.load().ctpvae_abi_version() == lib.ABI_VERSION == 3400
    assert "conv.hip" in open(os.path.join(ROOT, "ct_pvae_amd", "csrc", "Makefile")).read()


def test_python_wrapper_refuses_what_it_cannot_run(lib):
    import ct_pvae_amd
    from ct_pvae_amd import conv
    fn = ct_pvae_amd.periodic_conv_maxout
    assert fn is conv.periodic_conv_maxout
    x, w, b = torch.zeros(2, 3, 5, 7), torch.zeros(4, 3, 3, 3), torch.zeros(4)
    pads = (1, 1, 1, 1)
    for bad in ((x.numpy(), w, b), (x, w.numpy(), b), (x, w, b.numpy()), (x.double(), w, b), (x, w.double(), b), (x, w, b.double())):
        with pytest.raises(TypeError):
            fn(*bad, 1, pads)
    with pytest.raises(TypeError):
        fn(x, w, b, 1.0, pads)
    for bad in ((x[0], w, b), (x, w[0], b), (x, w, b[None]),                           # axes
                (torch.zeros(2, 0, 5, 7), torch.zeros(4, 0, 3, 3), b),                 # empty
                (torch.zeros(2, 6, 5, 7)[:, :3], w, b),                                # not contiguous
                (x, torch.zeros(4, 3, 3, 6)[..., :3], b), (x, w, torch.zeros(8)[::2]),
                (x, torch.zeros(4, 2, 3, 3), b),                                       # Cin
                (x, torch.zeros(3, 3, 3, 3), torch.zeros(3)),                          # an odd channel count
                (x, torch.zeros(4, 3, 3, 2), b),                                       # not square
                (x, w, torch.zeros(6)),                                                # bias
                (x, torch.zeros(4, 3, 9, 9), b)):                                      # k > 8
        with pytest.raises(ValueError):
            fn(*bad, 1, pads)
    for stride in (0, 4):
        with pytest.raises(ValueError):
            fn(x, w, b, stride, pads)
    for bad in ((1, 1, 1), (1, 1, -1, 1)):
        with pytest.raises(ValueError):
            fn(x, w, b, 1, bad)
    with pytest.raises(ValueError):
        fn(torch.zeros(1, 3, 1, 1), w, b, 1, (0, 0, 0, 0))                           # no window fits
    with pytest.raises(lib.RadonLibraryError, match="no CPU path"):
        fn(x, w, b, 1, pads)
    with pytest.raises(lib.RadonLibraryError, match="no CPU path"):
        conv._conv_maxout_with_first(x, w, b, 1, pads)


def test_fused_conv_flag():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).fused_conv is False and tr.get_args(["--normal"]).fused_conv is False              # off by default
    for flags in ("--fused_conv", "--det --fused_conv", "--normal --fused_conv --dp 0.1", "--reproducible --fused_conv",
                  "--normal --fused_head --fused_latents --fused_blocks --fused_update --fused_conv"):
        assert tr.get_args(flags.split()).fused_conv is True
    a = tr.get_args("--normal --fused_blocks".split())
    assert a.fused_conv is False and a.fused_blocks is True


def test_fused_conv_blocks_keep_their_parameters_and_names():
    from ct_pvae_amd import trainer as tr
    torch.manual_seed(3)
    plain, fused = tr.ConvBlock(3, 4, 4, 2, False), tr.ConvBlock(3, 4, 4, 2, False, fused_conv=True)
    assert plain.fused_conv is False and fused.fused_conv is True
    sp, sf = plain.state_dict(), fused.state_dict()
    assert list(sp) == list(sf) == ["ab.weight", "ab.bias"]
    assert [tuple(v.shape) for v in sp.values()] == [tuple(v.shape) for v in sf.values()] == [(8, 3, 4, 4), (8,)]
    fused.load_state_dict(sp, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(sp.values(), fused.state_dict().values()))
    nets = {}
    for flag in (False, True):
        torch.manual_seed(4)
        enc = tr.EncodeNet(2, [4, 6], 2, 4, 2, 1, 4, fused_conv=flag)
        dec = tr.DecodeNet(enc.channels, 2, 1, 4, 2, 1, 4, fused_conv=flag)
        nets[flag] = (enc, dec)
        blocks = [m for net in (enc, dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
        assert len(blocks) == 9 and all(blk.fused_conv is flag for blk in blocks)
    for a, b in zip(nets[False], nets[True]):
        assert list(a.state_dict()) == list(b.state_dict())
        assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))      # the same initialisation
    with pytest.raises(Exception, match="no CPU path"):
        fused(torch.zeros(1, 3, 8, 8))                      # the flag is taken: no quiet torch convolution behind it


def test_no_conv_kernel_has_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "conv.hip", "-o", os.devnull],
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
    assert len(seen) == 4 and all("conv_" in n for n in seen), seen
    assert not bad, f"kernels with scratch (register spills): {bad}"
