"""Host side of the fused ConvBlock glue (ct_pvae_amd/convblock.py, csrc/convblock.hip): tests/np_twin_convblock.py against the
trainer's _PeriodicPad and _Maxout on the CPU, the entry points' argument checks, the wrappers' input checks, the trainer's flag and
the nets' unchanged state_dict.  The kernels themselves: tests/test_gpu_convblock.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import np_twin_convblock as tw
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", tw.PAD_CASES, ids=tw.pad_id)
def test_pad_twin_is_the_trainers_periodic_pad_on_the_cpu(case):
    """Forward by bits, gradient by np.array_equal -- also where an axis wraps more than once: torch's CPU index_add_ adds in
    ascending order, the order the twin (and csrc/convblock.hip) states."""
    from ct_pvae_amd import trainer as tr
    shape, pads = case
    rng = np.random.default_rng(sum(shape) + 7 * sum(pads))
    x = rng.standard_normal(shape).astype(np.float32)
    want = tw.pad_fwd(x, pads)
    wl, wr, hl, hr = pads
    assert want.shape == shape[:2] + (shape[2] + hl + hr, shape[3] + wl + wr)
    xt = torch.from_numpy(x).requires_grad_(True)
    out = tr._PeriodicPad.apply(xt, pads)
    assert np.array_equal(_bits(out.detach().numpy()), _bits(want))
    g = rng.standard_normal(want.shape).astype(np.float32)
    out.backward(torch.from_numpy(g))
    assert np.array_equal(xt.grad.numpy(), tw.pad_bwd(g, shape[2:], pads))


def test_pad_twin_wraps_as_stated():
    """H = 1 with a 4-tap kernel: every padded row is row 0; a column of W = 3 under (2, 1) is read at 1, 2, 0, 1, 2, 0."""
    assert tw.pad_index(3, 2, 1).tolist() == [1, 2, 0, 1, 2, 0] and tw.pad_index(1, 2, 1).tolist() == [0, 0, 0, 0]
    g = np.arange(16, dtype=np.float32).reshape(1, 1, 4, 4)
    assert tw.pad_bwd(g, (1, 1), (2, 1, 2, 1)).tolist() == [[[[120.0]]]]
    assert not tw.at_most_two_copies((2, 2, 2, 3), (2, 1, 2, 1)) and tw.at_most_two_copies((2, 3, 5, 7), (2, 1, 1, 1))
    # the order matters once there are three terms: (1e8 + 1) - 1e8 = 0 in float32, 1e8 + (1 - 1e8) != that in general
    g = np.array([1e8, 1.0, -1e8], np.float32).reshape(1, 1, 1, 3)
    assert tw.pad_bwd(g, (1, 1), (1, 1, 0, 0)).item() == 0.0


@pytest.mark.parametrize("shape", tw.MAXOUT_SHAPES, ids=tw.shape_id)
def test_maxout_twin_is_the_trainers_maxout_on_the_cpu(shape):
    from ct_pvae_amd import trainer as tr
    rng = np.random.default_rng(sum(shape))
    y = rng.standard_normal(shape).astype(np.float32)
    want, first = tw.maxout_fwd(y)
    yt = torch.from_numpy(y).requires_grad_(True)
    out = tr._Maxout.apply(yt)
    assert np.array_equal(_bits(out.detach().numpy()), _bits(want))
    g = rng.standard_normal(want.shape).astype(np.float32)
    out.backward(torch.from_numpy(g))
    assert np.array_equal(yt.grad.numpy(), tw.maxout_bwd(g, first))


def test_maxout_twin_on_the_planted_pairs():
    """A tie and both signed-zero pairings take the first half, a NaN in either half takes the second; the trainer's _Maxout agrees
    by bits."""
    from ct_pvae_amd import trainer as tr
    y, first = tw.planted_maxout()
    out, got_first = tw.maxout_fwd(y)
    assert np.array_equal(got_first, first)
    assert np.array_equal(_bits(out), _bits(np.where(first, y[:, :1], y[:, 1:])))
    assert np.array_equal(_bits(tr._Maxout.apply(torch.from_numpy(y)).numpy()), _bits(out))
    g = np.full(out.shape, np.inf, np.float32)
    gy = tw.maxout_bwd(g, first)
    assert np.array_equal(gy[:, :1], np.where(first, np.inf, 0.0)) and np.array_equal(gy[:, 1:], np.where(first, 0.0, np.inf))


def test_bad_arguments_are_einval_before_any_hip_call(lib):
    L = lib.load()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # (host pointers: every call below is refused before the pointer is used or a HIP call is made)
    #       src planes H  W  wl wr hl hr dst stream
    good = [p, 2, 3, 4, 2, 1, 2, 1, p, None]
    for fn in (L.ctpvae_periodic_pad_fwd_f32, L.ctpvae_periodic_pad_bwd_f32):
        for i in (0, 8):
            bad = list(good)
            bad[i] = None
            assert fn(*bad) == lib.EINVAL and "null" in lib.last_error()
        for i in (1, 2, 3):
            for v in (0, -1):
                bad = list(good)
                bad[i] = v
                assert fn(*bad) == lib.EINVAL and "at least 1" in lib.last_error(), (i, v)
        for i in (4, 5, 6, 7):
            bad = list(good)
            bad[i] = -1
            assert fn(*bad) == lib.EINVAL and "negative" in lib.last_error(), i
        for planes, H, W, pads in ((2 ** 15, 2 ** 8, 2 ** 8, (0, 0, 0, 0)),             # 2^31 elements exactly
                                   (1, 2 ** 15, 2 ** 15, (2 ** 15, 0, 0, 0)),           # ... only once padded
                                   (1, 1, 1, (2 ** 31 - 1, 2 ** 31 - 1, 0, 0)),         # the padded width alone
                                   (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, (0, 0, 0, 0))):
            assert fn(p, planes, H, W, *pads, p, None) == lib.EINVAL and "31 bits" in lib.last_error(), (planes, H, W, pads)
    #         y  n  len out first stream
    good_f = [p, 2, 8, p, p, None]
    for i in (0, 3, 4):
        bad = list(good_f)
        bad[i] = None
        assert L.ctpvae_maxout_fwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    #         g first n  len gy stream
    good_b = [p, p, 2, 8, p, None]
    for i in (0, 1, 4):
        bad = list(good_b)
        bad[i] = None
        assert L.ctpvae_maxout_bwd_f32(*bad) == lib.EINVAL and "null" in lib.last_error()
    for n, length, word in ((0, 8, "at least 1"), (2, 0, "at least 1"), (-1, 8, "at least 1"), (2 ** 15, 2 ** 15, "31 bits"),
                            (2 ** 31 - 1, 2 ** 31 - 1, "31 bits")):
        assert L.ctpvae_maxout_fwd_f32(p, n, length, p, p, None) == lib.EINVAL and word in lib.last_error(), (n, length)
        assert L.ctpvae_maxout_bwd_f32(p, p, n, length, p, None) == lib.EINVAL and word in lib.last_error(), (n, length)
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL, "convblock")


def test_python_wrappers_refuse_what_they_cannot_run(lib):
    from ct_pvae_amd import maxout, periodic_pad
    x = torch.zeros(2, 4, 5, 7)
    pads = (2, 1, 2, 1)
    for fn in (lambda t: periodic_pad(t, pads), maxout):
        with pytest.raises(TypeError):
            fn(x.numpy())
        with pytest.raises(TypeError):
            fn(x.double())
        with pytest.raises(ValueError):
            fn(x[0])                                                 # not 4-D
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 0, 5, 7))                              # empty
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 8, 5, 7)[:, :4])                       # a channel half: not contiguous
        with pytest.raises(lib.RadonLibraryError, match="no CPU path"):
            fn(x)
    with pytest.raises(ValueError):
        maxout(torch.zeros(2, 3, 5, 7))                              # odd channel count
    for bad in ((2, 1, 2), (2, 1, -1, 1)):
        with pytest.raises(ValueError):
            periodic_pad(x, bad)


def test_fused_blocks_flag():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).fused_blocks is False and tr.get_args(["--normal"]).fused_blocks is False          # off by default
    for flags in ("--fused_blocks", "--det --fused_blocks", "--normal --fused_blocks",                         # independent of --normal, --det
                  "--normal --fused_head --fused_latents --fused_blocks"):
        assert tr.get_args(flags.split()).fused_blocks is True
    a = tr.get_args("--normal --fused_head".split())
    assert a.fused_blocks is False and a.fused_head is True


def test_fused_blocks_nets_keep_their_parameters_and_names():
    """EncodeNet / DecodeNet with fused_blocks=True have the state_dict keys and shapes of the nets built without it, each loads the
    other's (strict), and every ConvBlock carries the flag it was built with."""
    from ct_pvae_amd import trainer as tr
    nets = {}
    for fused in (False, True):
        torch.manual_seed(3 + fused)
        enc = tr.EncodeNet(2, [4, 6], 2, 4, 2, 1, 4, fused_blocks=fused)
        dec = tr.DecodeNet(enc.channels, 2, 1, 4, 2, 1, 4, fused_blocks=fused)
        nets[fused] = (enc, dec)
        blocks = [m for net in (enc, dec) for m in net.modules() if isinstance(m, tr.ConvBlock)]
        assert len(blocks) == 4 + 5 and all(b.fused_blocks is fused for b in blocks)
    assert tr.ConvBlock(2, 3, 4, 2, False).fused_blocks is False                         # the default path is the torch chain
    for plain, fused in zip(nets[False], nets[True]):
        sp, sf = plain.state_dict(), fused.state_dict()
        assert list(sp) == list(sf) and [tuple(v.shape) for v in sp.values()] == [tuple(v.shape) for v in sf.values()]
        assert not all(torch.equal(a, b) for a, b in zip(sp.values(), sf.values()))
        fused.load_state_dict(sp, strict=True)
        assert all(torch.equal(a, b) for a, b in zip(sp.values(), fused.state_dict().values()))
        plain.load_state_dict({k: v + 1 for k, v in sf.items()}, strict=True)
        assert all(torch.equal(a + 1, b) for a, b in zip(sf.values(), plain.state_dict().values()))
