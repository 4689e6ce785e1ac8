"""What the per-pixel marginals (ct_pvae_amd/marginals.py, csrc/marginals.hip) promise without a device: the library's own bin rule
(the host build of the kernel's function) against the numpy twin, bit for bit; bin_samples; every validation error that needs no
launch; the trainer's flags."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import PixelMarginals, _lib, bin_samples, marginals
from ct_pvae_amd import trainer as tr
from tests import np_twin_marginals as tm

LO, WIDTH = 0.005, 0.01          # the reference's np.arange(0.005, 0.51, 0.01)


def _ulp_neighbours(v):
    v = np.atleast_1d(np.asarray(v, np.float32))
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def edge_cases(bins):
    """The 51 nominal edges of the reference grid (as float32 of the float64 edge, and as float32 arithmetic gives them) with one ulp
    either side, 0, values just below lo, lo + bins * width, 1e10, inf, NaN, and a few negatives."""
    F = np.float32
    edges64 = LO + WIDTH * np.arange(51)
    edges32 = F(LO) + F(WIDTH) * np.arange(51, dtype=F)
    top = np.array([LO + bins * WIDTH], np.float64)
    with np.errstate(all="ignore"):
        return np.concatenate([_ulp_neighbours(edges64), _ulp_neighbours(edges32), _ulp_neighbours(top),
                               _ulp_neighbours(F(LO) + F(bins) * F(WIDTH)),
                               np.array([0.0, -0.0, LO * (1 - 1e-7), LO - 1e-9, LO - WIDTH, -1.0, 1e10, np.inf, -np.inf, np.nan], F)]).astype(F)


@pytest.mark.parametrize("bins", [1, 50, 254])
def test_host_bin_function_equals_the_twin(bins):
    x = edge_cases(bins)
    got = marginals.bin_columns(x, LO, WIDTH, bins)
    want = tm.bin_columns(x, LO, WIDTH, bins)
    assert got.dtype == np.int32 and got.shape == x.shape
    np.testing.assert_array_equal(got, want)
    assert got.min() == 0 and got.max() == bins + 1
    assert got[np.isnan(x)].tolist() == [0] and got[x == np.inf].tolist() == [bins + 1]
    assert set(got[x == 0].tolist()) == {0}
    if bins == 50:                   # every column of the reference grid is reached by its own lower edge
        assert set(got.tolist()) == set(range(52))


def test_host_bin_function_on_a_dense_sweep_and_another_grid():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-0.1, 0.7, 20000), rng.standard_normal(2000) * 5]).astype(np.float32)
    for lo, width, bins in ((LO, WIDTH, 50), (0.0, 0.125, 7), (-1.0, 0.3, 254), (0.05, 1e-3, 100)):
        np.testing.assert_array_equal(marginals.bin_columns(x, lo, width, bins), tm.bin_columns(x, lo, width, bins))


def test_bin_samples_rows_sum_to_the_number_of_samples():
    rng = np.random.default_rng(5)
    s = rng.uniform(-0.05, 0.6, (7, 11, 4)).astype(np.float32)       # e.g. [results][chains][pixels]
    s[0, 0, 0], s[1, 2, 3] = np.nan, np.inf
    h = bin_samples(s, LO, WIDTH, 50)
    assert h.shape == (4, 52) and h.dtype == np.int64
    np.testing.assert_array_equal(h.sum(axis=1), np.full(4, 77))
    np.testing.assert_array_equal(h, tm.hist(s, LO, WIDTH, 50))
    assert h[0, 0] >= 1 and h[3, 51] >= 1
    np.testing.assert_array_equal(bin_samples(s.astype(np.float64)[0, 0], LO, WIDTH, 50).sum(axis=1), np.ones(4))
    with pytest.raises(ValueError):
        bin_samples(np.float32(1.0), LO, WIDTH, 50)


@pytest.mark.parametrize("kw", [dict(bins=0), dict(bins=255), dict(width=0.0), dict(width=-1.0), dict(width=float("inf")),
                                dict(lo=float("nan")), dict(lo=float("inf")), dict(width=float("nan")), dict(width=1e-60),
                                dict(lo=1e60)])
def test_bad_grids_are_refused(kw):
    args = dict(bins=50, lo=LO, width=WIDTH)
    args.update(kw)
    with pytest.raises(ValueError):
        PixelMarginals((2, 2), device="cpu", **args)
    with pytest.raises(ValueError):
        bin_samples(np.zeros((3, 4), np.float32), args["lo"], args["width"], args["bins"])


def test_the_library_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    x, col = np.zeros(4, np.float32), np.zeros(4, np.int32)
    assert lib.ctpvae_tn_marginals_bin_host_f32(x.ctypes.data, 4, LO, WIDTH, 255, col.ctypes.data) == _lib.EINVAL
    assert "bins" in _lib.last_error()
    assert lib.ctpvae_tn_marginals_bin_host_f32(x.ctypes.data, 4, LO, 0.0, 50, col.ctypes.data) == _lib.EINVAL
    assert lib.ctpvae_tn_marginals_bin_host_f32(None, 4, LO, WIDTH, 50, col.ctypes.data) == _lib.EINVAL
    # the device entry point checks everything before it touches the GPU: null pointers and bad counts need no device
    assert lib.ctpvae_tn_marginals_f32(None, None, 1, 4, 0, 0, 0, 1, LO, WIDTH, 50, None, None, None, None, None) == _lib.EINVAL
    assert "null" in _lib.last_error()
    one = 8       # (any non-null, 16-byte aligned address: refused before it is read)
    for kw, word in ((dict(draws=0), "draws"), (dict(draw0=2 ** 32 - 1, draws=2), "draw0"), (dict(bins=0), "bins"),
                     (dict(width=-1.0), "width"), (dict(n=0), "positive"), (dict(first_object=-1), "first_object"),
                     (dict(n=2 ** 20, pix=1, draws=2 ** 12), "32 bits"), (dict(state=None), "null")):
        a = dict(n=1, pix=4, first_object=0, draw0=0, draws=1, lo=LO, width=WIDTH, bins=50, state=one)
        a.update(kw)
        rc = lib.ctpvae_tn_marginals_f32(one, one, a["n"], a["pix"], a["first_object"], 0, a["draw0"], a["draws"], a["lo"], a["width"],
                                         a["bins"], a["state"], a["state"], a["state"], a["state"], None)
        assert rc == _lib.EINVAL and word in _lib.last_error(), (kw, _lib.last_error())
    # the workspace: [G][2][pix] doubles, G = min(ceil(n * ceil(draws / 25) / 16), 64) -- bounded whatever draws is
    for n, pix, draws in ((1, 4, 1), (8, 4, 100), (20, 16384, 100), (3, 7, 26), (20, 16384, 10 ** 6), (1, 1, 2 ** 32 - 1)):
        assert lib.ctpvae_tn_marginals_workspace_bytes(n, pix, draws) == tm.groups(n, draws) * 2 * pix * 8
    assert lib.ctpvae_tn_marginals_workspace_bytes(20, 16384, 10 ** 6) == 64 * 2 * 16384 * 8
    assert lib.ctpvae_tn_marginals_workspace_bytes(0, 4, 1) == _lib.EINVAL


def test_add_validates_before_any_launch():
    m = PixelMarginals((2, 3), device="cpu")
    assert m.count == 0 and m.hist.shape == (6, 52) and m.hist.dtype == torch.int64 and m.s1.dtype == torch.float64
    assert m.edges.shape == (51,) and m.edges[0] == LO and abs(m.edges[-1] - 0.505) < 1e-12
    assert torch.isnan(m.mean()).all() and torch.isnan(m.std()).all() and m.mean().shape == (2, 3)
    ok = torch.zeros((4, 1, 2, 3))
    with pytest.raises(TypeError):
        m.add(ok.numpy(), ok, draws=1, seed=0)
    with pytest.raises(TypeError):
        m.add(ok, ok.double(), draws=1, seed=0)
    with pytest.raises(TypeError):
        m.add(ok.half(), ok, draws=1, seed=0)
    for bad in (torch.zeros((4, 2, 3)), torch.zeros((4, 2, 2, 3)), torch.zeros((4, 1, 3, 2)), torch.zeros((0, 1, 2, 3)),
                torch.zeros((4, 1, 3, 2)).transpose(2, 3)):
        with pytest.raises(ValueError):
            m.add(bad, ok, draws=1, seed=0)
        with pytest.raises(ValueError):
            m.add(ok, bad, draws=1, seed=0)
    with pytest.raises(ValueError):
        m.add(ok, torch.zeros((5, 1, 2, 3)), draws=1, seed=0)
    for kw in (dict(draws=0), dict(draws=-3), dict(draws=2, draw0=2 ** 32 - 1), dict(draws=1, draw0=2 ** 32), dict(draws=1, draw0=-1),
               dict(draws=1, first_object=-1), dict(draws=2 ** 30)):
        with pytest.raises(ValueError):
            m.add(ok, ok, seed=0, **kw)
    with pytest.raises(_lib.RadonLibraryError):          # every argument is fine, but there is no CPU path
        m.add(ok, ok, draws=1, seed=0)
    assert m.count == 0 and int(m.hist.sum()) == 0


def test_save_and_load_round_trip(tmp_path):
    m = PixelMarginals((2, 2), bins=7, lo=0.25, width=0.5, device="cpu")
    m._hist.copy_(torch.arange(36).view(4, 9))
    m._s1.copy_(torch.tensor([1.5, 2.5, 3.5, 4.5], dtype=torch.float64))
    m._s2.copy_(torch.tensor([3.0, 7.0, 13.0, 21.0], dtype=torch.float64))
    m.count = 3
    path = str(tmp_path / "pixel_dist_0.npz")
    m.save(path)
    with np.load(path) as f:
        assert {"hist", "s1", "s2", "count", "lo", "width"} <= set(f.files)
        assert f["hist"].shape == (4, 9) and int(f["count"]) == 3
    back = PixelMarginals.load(path, device="cpu")
    assert back.count == 3 and back.bins == 7 and back.lo == 0.25 and back.width == 0.5 and back.shape == (2, 2)
    assert torch.equal(back.hist, m.hist) and torch.equal(back.s1, m.s1) and torch.equal(back.s2, m.s2)
    np.testing.assert_allclose(back.mean().numpy(), np.array([[0.5, 2.5 / 3], [3.5 / 3, 1.5]]), rtol=1e-15)
    np.testing.assert_allclose(back.std().numpy().ravel(), np.sqrt((np.array([3.0, 7.0, 13.0, 21.0]) - np.array([1.5, 2.5, 3.5, 4.5]) ** 2 / 3) / 2),
                               rtol=1e-14)


def test_twin_order_is_a_sum():
    """The twin's restatement of the kernel's order adds every sample exactly once (it stays within the any-order bound of fsum)."""
    rng = np.random.default_rng(9)
    for K, n, pix in ((1, 1, 4), (26, 3, 7), (100, 20, 5), (51, 70, 3)):
        x = rng.uniform(0, 3, (K, n, pix)).astype(np.float32)
        (t1, t2), (f1, f2) = tm.ordered_sums(x), tm.fsum_sums(x)
        assert np.all(np.abs(t1 - f1) <= tm.fsum_bound(n * K) * f1) and np.all(np.abs(t2 - f2) <= tm.fsum_bound(n * K) * f2)


def test_marginals_kernels_do_not_spill():
    """hipcc's own resource report for csrc/marginals.hip with the library's flags: no kernel uses scratch."""
    import os
    import re
    import shutil
    import subprocess
    from tests.conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "marginals.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert any("tn_marginals_kernel" in n for n in names) and any("tn_marginals_finish_kernel" in n for n in names)
    assert len(scratch) == len(names) and not any(scratch), list(zip(names, scratch))


def test_trainer_flags():
    a = tr.get_args("--normal --pixel_dist --en 3 --pixel_repeats 7".split())
    assert a.pixel_dist is True and a.example_num == 3 and a.pixel_repeats == 7
    d = tr.get_args(["--normal"])
    assert d.pixel_dist is False and d.example_num == 0 and d.pixel_repeats == 10000
    with pytest.raises(ValueError):
        tr.get_args(["--pixel_dist"])                       # the Beta head is not sampled by any kernel
    with pytest.raises(ValueError):
        tr.get_args(["--pixel_dist", "--normal", "--det"])
