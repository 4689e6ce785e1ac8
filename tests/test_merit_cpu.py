"""What the device metrics (ct_pvae_amd/merit.py, csrc/merit.hip) and the scoring stage (ct_pvae_amd/final_merit.py) promise without a
device: the float64 twin in the kernel's order of sums is scikit-image's and dataset_io.compare's function, the entry points refuse bad
arguments before any HIP call, the size rules equal the twin's, and final_merit's host pieces follow bin/final_merit.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, dataset_io as io
from ct_pvae_amd import final_merit as fm
from ct_pvae_amd import image_merits, merit
from ct_pvae_amd import trainer as tr
from tests import np_twin_merit as tm

RTOL = 1e-9          # the bar tests/test_dataset_io.py holds compare to against scikit-image


def test_twin_reproduces_scikit_image(golden_dir):
    z = np.load(os.path.join(golden_dir, "compare_skimage018.npz"))
    for k in "abc":
        got = tm.merits(z[k + "_r0"], z[k + "_r1"])
        np.testing.assert_allclose(got, [z[k + "_mse"], z[k + "_ssim"], z[k + "_psnr"]], rtol=RTOL)


@pytest.mark.parametrize("kind", tm.KINDS)
@pytest.mark.parametrize("shape", tm.SHAPES)
def test_twin_agrees_with_compare(shape, kind):
    """A direct-sum float64 twin lies ~1e-15 relative from compare on these inputs (max|r| = R): only a wrong formula crosses 1e-9."""
    r, t = tm.seeded_pair(shape, kind)
    assert np.abs(r).max() <= 2 * (r.max() - r.min())
    np.testing.assert_allclose(tm.merits(r, t), io.compare(r, t, verbose=False), rtol=RTOL)


def test_twin_window_rule_and_batch():
    assert [tm.win_size(m, 50) for m in (3, 4, 5, 6, 7, 8, 100)] == [3, 3, 5, 5, 7, 7, 7]
    r, t = tm.seeded_pair((8, 9), "uniform", n=3)
    b = tm.batch(r, t)
    assert b.shape == (3, 3) and all(tuple(b[k]) == tm.merits(r[k], t[k]) for k in range(3))
    with pytest.raises(ValueError):
        tm.merits(np.zeros((2, 9)), np.zeros((2, 9)))


@pytest.mark.parametrize("shape", ((3, 3), (9, 9), (40, 33)))
def test_twin_identical_images(shape):
    r, _ = tm.seeded_pair(shape, "uniform", seed=1)
    assert tm.merits(r, r) == (0.0, 1.0, np.inf)


def test_twin_order_of_sums():
    """ST(v, w): strided partials ascending, then halving -- on values whose sum depends on the order."""
    v = np.array([1.0, 2.0 ** -53, 2.0 ** -53, -1.0, 3.0])
    assert tm.st(v, 2) == ((1.0 + 2.0 ** -53) + 3.0) + (2.0 ** -53 + -1.0)
    assert tm.st(v, 4) == ((1.0 + 3.0) + 2.0 ** -53) + (2.0 ** -53 + -1.0)
    assert tm.st([], 64) == 0.0


def test_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    for fn in (lib.ctpvae_merit_f32, lib.ctpvae_merit_f64):
        assert fn(None, p, 1, 4, 4, p, p, None) == _lib.EINVAL and "null" in _lib.last_error()
        assert fn(p, None, 1, 4, 4, p, p, None) == _lib.EINVAL
        assert fn(p, p, 1, 4, 4, None, p, None) == _lib.EINVAL
        assert fn(p, p, 1, 4, 4, p, None, None) == _lib.EINVAL
        assert fn(p, p, 1, 2, 9, p, p, None) == _lib.EINVAL and "3 x 3" in _lib.last_error()
        assert fn(p, p, 1, 9, 2, p, p, None) == _lib.EINVAL
        assert fn(p, p, -1, 4, 4, p, p, None) == _lib.EINVAL and "n must be" in _lib.last_error()
        assert fn(p, p, 1, 65536, 32768, p, p, None) == _lib.EINVAL and "X * Y" in _lib.last_error()
        assert fn(p, p, 3, 32768, 32768, p, p, None) == _lib.EINVAL and "n * X * Y" in _lib.last_error()
        assert fn(None, None, 0, 4, 4, None, None, None) == 0          # n = 0: nothing to launch, nothing to point at
        assert fn(None, None, 0, 2, 4, None, None, None) == _lib.EINVAL


def test_size_queries_equal_the_twin():
    lib = _lib.load()
    assert lib.ctpvae_merit_tile() == tm.TILE == merit.merit_tile()
    for n, X, Y in ((1, 3, 3), (3, 128, 128), (17, 37, 38), (2, 39, 65), (5, 512, 96), (1000, 128, 128), (96, 512, 512), (1, 7, 100000)):
        assert lib.ctpvae_merit_workspace_bytes(n, X, Y) == tm.workspace_bytes(n, X, Y)
        win, Xo, Yo, trows, tcols, chunks = tm.shape(X, Y)
        assert chunks <= trows * tcols                      # the bound the header states: at most 4 * tiles * n doubles
    assert lib.ctpvae_merit_workspace_bytes(3, 128, 128) == 3 * (3 * 4 + 16) * 8
    assert lib.ctpvae_merit_workspace_bytes(0, 128, 128) == 0
    assert lib.ctpvae_merit_workspace_bytes(1, 2, 128) == _lib.EINVAL
    assert lib.ctpvae_merit_workspace_bytes(-1, 8, 8) == _lib.EINVAL
    assert lib.ctpvae_merit_workspace_bytes(2, 32768, 32768) == _lib.EINVAL


def test_image_merits_refusals():
    a32, a64 = np.zeros((2, 8, 8), np.float32), np.zeros((2, 8, 8), np.float64)
    with pytest.raises(ValueError, match="one shape"):
        image_merits(a32, a32[:, :7])
    with pytest.raises(ValueError, match="one dtype"):
        image_merits(a32, a64)
    with pytest.raises(ValueError, match="float32 or float64"):
        image_merits(a32.astype(np.int32), a32.astype(np.int32))
    with pytest.raises(ValueError, match=r"\[X\]\[Y\]"):
        image_merits(a32[None], a32[None])
    with pytest.raises(ValueError, match="3 x 3"):
        image_merits(a32[:, :2], a32[:, :2])
    with pytest.raises(TypeError):
        image_merits([[0.0]], [[0.0]])
    with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):
        image_merits(torch.from_numpy(a32), torch.from_numpy(a32))


def test_merit_kernels_do_not_spill():
    """hipcc's own resource report for csrc/merit.hip, compiled with the Makefile's own HIPFLAGS: every kernel is there and none uses
    scratch (tests/test_abi.py's gate names four projector sources; this is the same gate for the new one)."""
    import re
    import shutil
    import subprocess
    from tests.conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    csrc = os.path.join(ROOT, "ct_pvae_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", makefile, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert "-ffp-contract=off" in flags and "merit.hip" in re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    out = subprocess.run([hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", "merit.hip", "-o", os.devnull],
                         cwd=csrc, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    for kernel in ("merit_range_kernel", "merit_ssim_kernel", "merit_finish_kernel"):
        assert any(kernel in n for n in names), names
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))


# ---- final_merit's host pieces

def test_ground_truth_path_rule():
    """bin/final_merit.py:37,48: prefix = input_path[8:]; np.load(prefix + '_training.npy')."""
    assert fm.default_ground_truth_path("dataset_foam") == "foam_training.npy"
    assert fm.default_ground_truth_path("dataset_toy_discrete2") == "toy_discrete2_training.npy"


def test_group_by_angles():
    masks = np.zeros((6, 8), np.float32)
    masks[0, [0, 4]] = 0.5
    masks[1, [1, 5]] = 0.5
    masks[2, [0, 4]] = [0.25, 0.75]            # the same SET of angles as example 0, other values
    masks[3, [1, 5]] = 0.5
    masks[4, [0, 4, 6]] = 1 / 3
    masks[5, [0, 4]] = 0.5
    groups = fm.group_by_angles(masks)
    assert [(u.tolist(), e.tolist()) for u, e in groups] == [([0, 4], [0, 2, 5]), ([1, 5], [1, 3]), ([0, 4, 6], [4])]
    uniform = np.tile(masks[:1], (5, 1))
    (u, e), = fm.group_by_angles(uniform)
    assert u.tolist() == [0, 4] and e.tolist() == [0, 1, 2, 3, 4]
    assert sorted(k for _, e in groups for k in e.tolist()) == list(range(6))


def test_clamp():
    x = np.array([-0.5, 0.0, 0.25, 1.0, 1.5], np.float32)
    want = np.maximum(np.minimum(x, 1), 0)
    np.testing.assert_array_equal(fm.clamp01(x), want)
    np.testing.assert_array_equal(fm.clamp01(torch.from_numpy(x)).numpy(), want)
    assert fm.clamp01(x).dtype == np.float32


def test_cli_and_trainer_flags():
    with pytest.raises(SystemExit):
        fm.main(["--input_path", "dataset_x"])                         # --save_path and --pnm are required
    a = tr.get_args("--final_merit --save_path out".split())
    assert a.final_merit and a.ground_truth is None
    assert not tr.get_args([]).final_merit
    assert tr.get_args("--final_merit --save_path out --input_path dataset_x --ground_truth t.npy".split()).ground_truth == "t.npy"
    with pytest.raises(ValueError, match="--save_path"):
        tr.get_args(["--final_merit"])
    with pytest.raises(ValueError, match="--no_final_eval"):
        tr.get_args("--final_merit --save_path out --no_final_eval".split())
    # the new method sits beside pixel_dist: that one still runs without autograd (torch.no_grad wraps it), as before
    assert hasattr(tr.PVAETrainer.pixel_dist, "__wrapped__") and hasattr(tr.PVAETrainer.final_evaluation, "__wrapped__")
