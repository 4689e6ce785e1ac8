"""image_merits on the device (ct_pvae_amd/merit.py, csrc/merit.hip) against the float64 twin in the kernel's order of sums
(tests/np_twin_merit.py) and against dataset_io.compare.

Bars.  MSE and SSIM are chains of single float64 operations in one stated order, and numpy performs the same operations: the device
equals the twin bit for bit.  The PSNR ends in log10, a library function on both sides (each within 2 ulp of the true value by its
library's statement, then one multiplication): 1e-14 relative, 45 ulp, is far outside that and far inside any wrong formula.  Against
compare the bar is the issue's 1e-9 (compare itself is held to scikit-image at 1e-9; a direct-sum twin lies ~1e-15 from it on these
inputs, which keep max|r| = R).

Measured on an MI355X over every case of test_against_twin_and_compare: the worst distance from compare is 1.1e-14 relative (9 x 65
float64, n = 17; WORST_FROM_COMPARE below); MSE and SSIM equal the twin's bits in all 114 cases and the PSNR lies within 2.7e-16 of it.
tools/time_merit.py measures the same cases again and writes the figures into profiles/merit_timing.txt, beside those of the timed shapes."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, dataset_io as io
from ct_pvae_amd import image_merits, merit
from tests import np_twin_merit as tm

pytestmark = pytest.mark.gpu

# the largest |device - compare| / |compare| over every case of test_against_twin_and_compare, as measured on an MI355X (the test
# prints each case's figure before it asserts; the bar is RTOL, not this number)
WORST_FROM_COMPARE = 1.1e-14
RTOL = 1e-9
PSNR_RTOL = 1e-14
N_MAX = tm.GPU_N
T = tm.TILE
WIN = 7
SHAPES = tm.GPU_SHAPES         # the issue's shapes, and for each axis T + win - 2, T + win - 1, T + win, 2 T + 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert merit.merit_tile() == T
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def case(shape, dtype_name):
    """(ref, test [17][X][Y], the twin's [17][3], compare's [17][3]) -- computed once, shared by n = 1, 3, 17 (pair k's numbers do not
    depend on n), never modified."""
    r, t = tm.gpu_case_inputs(shape, dtype_name)
    assert r.dtype == np.dtype(dtype_name) and np.all(np.abs(r).max(axis=(1, 2)) <= 2 * (r.max(axis=(1, 2)) - r.min(axis=(1, 2))))
    twin = tm.batch(r, t)
    comp = np.array([io.compare(r[k], t[k], verbose=False) for k in range(N_MAX)])
    for a in (r, t, twin, comp):
        a.setflags(write=False)
    return r, t, twin, comp


def check_against_twin(got, twin):
    np.testing.assert_array_equal(got[:, :2], twin[:, :2])          # MSE, SSIM: the same bits
    np.testing.assert_allclose(got[:, 2], twin[:, 2], rtol=PSNR_RTOL, atol=0)


@pytest.mark.parametrize("n", (1, 3, N_MAX))
@pytest.mark.parametrize("dtype_name", ("float32", "float64"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_twin_and_compare(dev, shape, dtype_name, n):
    r, t, twin, comp = case(shape, dtype_name)
    got_t = image_merits(torch.from_numpy(r[:n]).to(dev), torch.from_numpy(t[:n]).to(dev))
    assert got_t.shape == (n, 3) and got_t.dtype is torch.float64 and got_t.device == dev
    got = got_t.cpu().numpy()
    print(f"merit {shape[0]}x{shape[1]} {dtype_name} n={n}: worst from compare {np.max(np.abs(got - comp[:n]) / np.abs(comp[:n])):.3e}, "
          f"from the twin {np.max(np.abs(got - twin[:n]) / np.abs(twin[:n])):.3e}")
    check_against_twin(got, twin[:n])
    np.testing.assert_allclose(got, comp[:n], rtol=RTOL, atol=0)


def test_golden_scikit_image_cases(dev, golden_dir):
    z = np.load(os.path.join(golden_dir, "compare_skimage018.npz"))
    for k in "abc":
        got = image_merits(z[k + "_r0"], z[k + "_r1"]).cpu().numpy()          # numpy arrays are uploaded; [X][Y] -> [1][3]
        assert got.shape == (1, 3)
        np.testing.assert_allclose(got[0], [z[k + "_mse"], z[k + "_ssim"], z[k + "_psnr"]], rtol=RTOL)
        check_against_twin(got, tm.batch(z[k + "_r0"], z[k + "_r1"]))


@pytest.mark.parametrize("dtype_name", ("float32", "float64"))
def test_identical_pairs(dev, dtype_name):
    for shape in ((3, 3), (8, 9), (T + WIN, 2 * T + 1), (128, 128)):
        r = torch.from_numpy(case_free(shape, dtype_name)).to(dev)
        got = image_merits(r, r.clone()).cpu().numpy()
        np.testing.assert_array_equal(got, np.tile([0.0, 1.0, np.inf], (r.shape[0], 1)))


def case_free(shape, dtype_name):
    return tm.seeded_pair(shape, "float32" if dtype_name == "float32" else "uniform", seed=9, n=3)[0]


def test_nan_pixel_and_constant_reference(dev):
    """Non-finite pixels propagate where numpy's formula lets them; R = 0 gives what the float64 formula gives: equal in kind (NaN where
    the twin has NaN, the same infinity where it has one) and equal in bits where finite."""
    r, t = (a.copy() for a in tm.seeded_pair((T + WIN, 50), "uniform", seed=2, n=5))
    r[1, 20, 30] = np.nan                      # in the reference: R is NaN, all three are NaN
    t[2, 38, 49] = np.nan                      # in the test image: MSE, SSIM (through its windows' mean) and PSNR are NaN
    r[3] = 0.25                                # constant reference: R = 0, c1 = c2 = 0, PSNR = 10 log10(0 / mse) = -inf
    r[4], t[4] = 0.5, 0.5                      # constant and identical: mse = 0 -> +inf by the stated rule; S is 0 / 0
    twin = tm.batch(r, t)
    got = image_merits(torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
    assert np.isnan(twin[1]).all() and np.isnan(twin[2]).all() and twin[3, 2] == -np.inf and twin[4, 2] == np.inf and twin[4, 0] == 0
    assert np.isfinite(twin[0]).all()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(twin))
    np.testing.assert_array_equal(got[:, :2], twin[:, :2])
    np.testing.assert_array_equal(np.isinf(got), np.isinf(twin))
    np.testing.assert_allclose(got[0, 2], twin[0, 2], rtol=PSNR_RTOL)
    assert got[3, 2] == -np.inf and got[4, 2] == np.inf


@pytest.mark.parametrize("shape", ((130, 67), (T + WIN, 2 * T + 1), (128, 128)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype_name", ("float32", "float64"))
def test_same_bits_every_run_and_in_any_batch(dev, shape, dtype_name):
    r, t, _, _ = case(shape, dtype_name)
    rd, td = torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)
    first = image_merits(rd, td)
    assert torch.equal(first, image_merits(rd, td))
    for k in (0, 7, N_MAX - 1):
        alone = image_merits(rd[k], td[k])                         # [X][Y]: pair k scored alone
        assert alone.shape == (1, 3) and torch.equal(alone[0], first[k]), k
    assert torch.equal(image_merits(rd[5:9].contiguous(), td[5:9].contiguous()), first[5:9])


def test_every_slot_is_written(dev):
    """The C entry on NaN-filled outputs and a NaN-filled workspace: a slot (or a partial sum) the kernels fail to write fails here."""
    lib = _lib.load()
    n, X, Y = N_MAX, T + WIN, 2 * T + 1
    r, t, twin, _ = case((X, Y), "float64")
    rd, td = torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)
    ws = torch.full((lib.ctpvae_merit_workspace_bytes(n, X, Y) // 8,), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    rc = lib.ctpvae_merit_f64(rd.data_ptr(), td.data_ptr(), n, X, Y, ws.data_ptr(), out.data_ptr(),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert not torch.isnan(ws).any() and not torch.isnan(out).any()
    check_against_twin(out.cpu().numpy(), twin)


def test_refusals_and_empty_batch(dev):
    a = torch.zeros((2, 8, 8), device=dev)
    with pytest.raises(ValueError, match="one shape"):
        image_merits(a, a[:, :7])
    with pytest.raises(ValueError, match="one dtype"):
        image_merits(a, a.double())
    with pytest.raises(ValueError, match="float32 or float64"):
        image_merits(a.half(), a.half())
    with pytest.raises(ValueError, match="3 x 3"):
        image_merits(a[:, :, :2], a[:, :, :2])
    with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):
        image_merits(a, a.cpu())
    with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):
        image_merits(a.cpu().numpy(), a.cpu())
    empty = image_merits(a[:0], a[:0])
    assert empty.shape == (0, 3) and empty.dtype is torch.float64 and empty.device == dev
    # a non-contiguous view is scored as the images it shows; a numpy operand goes to the tensor's device; no autograd
    r, t, twin, _ = case((8, 9), "float64")
    wide = torch.from_numpy(np.concatenate([r, r], axis=2)).to(dev)
    got = image_merits(wide[:, :, :9], t)
    assert got.device == dev and not got.requires_grad
    check_against_twin(got.cpu().numpy(), twin)
