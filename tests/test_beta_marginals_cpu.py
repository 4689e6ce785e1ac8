"""What the Beta head's per-pixel marginals (ct_pvae_amd/marginals.py head="beta", csrc/beta_marginals.hip) promise without a device:
every refusal of the entry point before any launch, the workspace rule, the `head` keyword of PixelMarginals and its place in the
saved file, the trainer's flags, and the compiler's own report that no kernel of the file uses scratch."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import PixelMarginals, _lib
from ct_pvae_amd import trainer as tr
from tests import np_twin_marginals as tm

LO, WIDTH = 0.005, 0.01          # the reference's np.arange(0.005, 0.51, 0.01)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """The list tests/test_marginals_cpu.py holds ctpvae_tn_marginals_f32 to: null pointers and bad counts need no device."""
    lib = _lib.load()
    assert lib.ctpvae_beta_marginals_f32(None, None, 1, 4, 0, 0, 0, 1, LO, WIDTH, 50, None, None, None, None, None) == _lib.EINVAL
    assert "null" in _lib.last_error()
    one = 8       # (any non-null, 16-byte aligned address: refused before it is read)
    for kw, word in ((dict(draws=0), "draws"), (dict(draw0=2 ** 32 - 1, draws=2), "draw0"), (dict(bins=0), "bins"), (dict(bins=255), "bins"),
                     (dict(width=-1.0), "width"), (dict(width=0.0), "width"), (dict(n=0), "positive"), (dict(first_object=-1), "first_object"),
                     (dict(n=2 ** 20, pix=1, draws=2 ** 12), "32 bits"), (dict(state=None), "null")):
        a = dict(n=1, pix=4, first_object=0, draw0=0, draws=1, lo=LO, width=WIDTH, bins=50, state=one)
        a.update(kw)
        rc = lib.ctpvae_beta_marginals_f32(one, one, a["n"], a["pix"], a["first_object"], 0, a["draw0"], a["draws"], a["lo"], a["width"],
                                           a["bins"], a["state"], a["state"], a["state"], a["state"], None)
        assert rc == _lib.EINVAL and word in _lib.last_error(), (kw, _lib.last_error())
        assert "beta_marginals" in _lib.last_error()


def test_the_workspace_rule():
    """[G][2][pix] doubles, G = min(ceil(n * ceil(draws / 25) / 16), 64): the TruncatedNormal entry point's rule at its six shapes."""
    lib = _lib.load()
    for n, pix, draws in ((1, 4, 1), (8, 4, 100), (20, 16384, 100), (3, 7, 26), (20, 16384, 10 ** 6), (1, 1, 2 ** 32 - 1)):
        assert lib.ctpvae_beta_marginals_workspace_bytes(n, pix, draws) == tm.groups(n, draws) * 2 * pix * 8
        assert lib.ctpvae_beta_marginals_workspace_bytes(n, pix, draws) == lib.ctpvae_tn_marginals_workspace_bytes(n, pix, draws)
    assert lib.ctpvae_beta_marginals_workspace_bytes(0, 4, 1) == _lib.EINVAL


def test_the_head_keyword():
    assert PixelMarginals((2, 2), device="cpu").head == "truncated_normal"
    assert PixelMarginals((2, 2), device="cpu", head="truncated_normal").head == "truncated_normal"
    assert PixelMarginals((2, 2), device="cpu", head="beta").head == "beta"
    for bad in ("bogus", "Beta", None, 0):
        with pytest.raises(ValueError):
            PixelMarginals((2, 2), device="cpu", head=bad)


def test_add_with_the_beta_head_validates_before_any_launch():
    """The same checks in the same order as the default head's, then: there is no CPU path."""
    m = PixelMarginals((2, 3), device="cpu", head="beta")
    ok = torch.zeros((4, 1, 2, 3))
    with pytest.raises(TypeError):
        m.add(ok.numpy(), ok, draws=1, seed=0)
    with pytest.raises(TypeError):
        m.add(ok, ok.double(), draws=1, seed=0)
    for bad in (torch.zeros((4, 2, 3)), torch.zeros((4, 1, 3, 2)), torch.zeros((0, 1, 2, 3)), torch.zeros((4, 1, 3, 2)).transpose(2, 3)):
        with pytest.raises(ValueError):
            m.add(bad, ok, draws=1, seed=0)
        with pytest.raises(ValueError):
            m.add(ok, bad, draws=1, seed=0)
    with pytest.raises(ValueError):
        m.add(ok, torch.zeros((5, 1, 2, 3)), draws=1, seed=0)
    for kw in (dict(draws=0), dict(draws=2, draw0=2 ** 32 - 1), dict(draws=1, draw0=-1), dict(draws=1, first_object=-1), dict(draws=2 ** 30)):
        with pytest.raises(ValueError):
            m.add(ok, ok, seed=0, **kw)
    with pytest.raises(_lib.RadonLibraryError):          # every argument is fine, but there is no CPU path
        m.add(ok, ok, draws=1, seed=0)
    assert m.count == 0 and int(m.hist.sum()) == 0 and float(m.s1.abs().sum()) == 0.0 and float(m.s2.abs().sum()) == 0.0


def _filled(head):
    m = PixelMarginals((2, 2), bins=7, lo=0.25, width=0.5, device="cpu", head=head)
    m._hist.copy_(torch.arange(36).view(4, 9))
    m._s1.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5], dtype=torch.float64))
    m._s2.copy_(torch.tensor([3.0, 7.0, 13.0, 21.0], dtype=torch.float64))
    m.count = 3
    return m


@pytest.mark.parametrize("head", ["beta", "truncated_normal"])
def test_save_and_load_round_trip_the_head(tmp_path, head):
    m = _filled(head)
    path = str(tmp_path / "pixel_dist_0.npz")
    m.save(path)
    with np.load(path, allow_pickle=False) as f:            # a plain numpy string: no pickle is needed to read it
        assert {"hist", "s1", "s2", "count", "lo", "width", "shape", "head"} <= set(f.files)
        assert f["head"].dtype.kind == "U" and str(f["head"]) == head
    back = PixelMarginals.load(path, device="cpu")
    assert back.head == head and back.count == 3 and back.bins == 7 and back.lo == 0.25 and back.width == 0.5 and back.shape == (2, 2)
    assert torch.equal(back.hist, m.hist) and torch.equal(back.s1, m.s1) and torch.equal(back.s2, m.s2)


def test_a_file_without_head_loads_as_truncated_normal(tmp_path):
    m = _filled("beta")
    path = str(tmp_path / "old.npz")
    np.savez(path, hist=m.hist.numpy(), s1=m.s1.numpy(), s2=m.s2.numpy(), count=np.int64(m.count), lo=np.float64(m.lo),
             width=np.float64(m.width), shape=np.asarray(m.shape, np.int64))
    back = PixelMarginals.load(path, device="cpu")
    assert back.head == "truncated_normal" and back.count == 3 and torch.equal(back.hist, m.hist)


def test_trainer_flags():
    a = tr.get_args("--pixel_dist --fused_beta_head --en 3 --pixel_repeats 7".split())
    assert a.pixel_dist is True and a.fused_beta_head is True and a.use_normal is False and a.example_num == 3 and a.pixel_repeats == 7
    assert tr.get_args("--pixel_dist --fused_beta_head --fused_beta_latents".split()).fused_beta_latents is True
    with pytest.raises(ValueError) as err:
        tr.get_args(["--pixel_dist"])                       # torch's generator draws that head: there are no keyed samples to add
    assert "--fused_beta_head" in str(err.value) and "--normal" in str(err.value)
    with pytest.raises(ValueError):
        tr.get_args(["--pixel_dist", "--fused_beta_head", "--det"])
    with pytest.raises(ValueError):
        tr.get_args(["--pixel_dist", "--fused_beta_head", "--normal"])
    with pytest.raises(ValueError):
        tr.get_args(["--pixel_dist", "--fused_beta_latents"])


def test_beta_marginals_kernels_do_not_spill():
    """hipcc's own resource report for csrc/beta_marginals.hip with the library's flags: no kernel uses scratch."""
    import os
    import re
    import shutil
    import subprocess
    from tests.conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "beta_marginals.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert any("beta_marginals_kernel" in n for n in names) and any("beta_marginals_finish_kernel" in n for n in names)
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))
