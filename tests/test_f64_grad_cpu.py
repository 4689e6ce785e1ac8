"""The float64 backwards of the rotate projector, on the CPU: the numpy twin (tests/np_twin64.py) states the oracle's rules, its
exact mode is the transpose of oracle.rotate_fwd_f64, and ctpvae_rotate_bwd_f64 refuses bad arguments without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import np_twin64 as twin
from tests.conftest import ROOT

GEOMS = [(1, 1, True), (1, 1, False), (2, 2, False), (17, 13, True), (17, 13, False), (33, 64, True), (33, 64, False)]


@pytest.mark.parametrize("interp", [0, 1])
def test_twin_in_fp32_is_the_oracle(oracle, interp):
    """With fp32 taps and sums the twin's two rules ARE oracle_rotate_bwd_tfcompat / _exact: the same bits."""
    rng = np.random.default_rng(7 + interp)
    for H, W, pad in GEOMS:
        geom = oracle.Geometry(H, W, pad)
        for A in (1, 7, 20):
            T, Tinv = twin.tables(twin.angle_set(A, rng), geom)
            g = rng.standard_normal((2, A, geom.PW)).astype(np.float32)
            np.testing.assert_array_equal(twin.bwd_tfcompat(g, geom, Tinv, interp, acc=np.float32),
                                          oracle.rotate_bwd_tfcompat(g, geom, Tinv, interp))
            np.testing.assert_array_equal(twin.bwd_exact(g, geom, T, interp, acc=np.float32),
                                          oracle.rotate_bwd_exact(g, geom, T, interp))


@pytest.mark.parametrize("interp", [0, 1])
def test_twin_exact_is_the_transpose_of_the_f64_forward(oracle, interp):
    """<A x, g> = <x, A^T g> with A = oracle.rotate_fwd_f64 and A^T the twin's exact mode, to double rounding: <= 1e-13 of
    the sum of |terms|."""
    rng = np.random.default_rng(11 + interp)
    for H, W, pad in GEOMS[2:] + [(64, 64, True)]:
        geom = oracle.Geometry(H, W, pad)
        A = 20
        T, _ = twin.tables(twin.angle_set(A, rng), geom)
        x = rng.random((2, H, W))
        g = rng.standard_normal((2, A, geom.PW))
        ax = oracle.rotate_fwd_f64(x, geom, T, interp)
        atg = twin.bwd_exact(g, geom, T, interp)
        assert atg.dtype == np.float64
        lhs, rhs = float((ax * g).sum()), float((x * atg).sum())
        assert abs(lhs - rhs) <= 1e-13 * float(np.abs(ax * g).sum()), (H, W, pad, lhs, rhs)


def test_twin_f64_keeps_digits_fp32_drops(oracle):
    """A float64 cotangent that fp32 cannot hold: the float64 rules differ from the fp32 ones cast back (~1e-7 relative),
    which is what a float64 caller got before ctpvae_rotate_bwd_f64."""
    rng = np.random.default_rng(3)
    geom = oracle.Geometry(17, 13, True)
    T, Tinv = twin.tables(twin.angle_set(7, rng), geom)
    g = rng.standard_normal((1, 7, geom.PW))
    for got, cast in ((twin.bwd_tfcompat(g, geom, Tinv, 1), oracle.rotate_bwd_tfcompat(g, geom, Tinv, 1)),
                      (twin.bwd_exact(g, geom, T, 1), oracle.rotate_bwd_exact(g, geom, T, 1))):
        err = np.abs(got - cast.astype(np.float64)).max() / np.abs(got).max()
        assert 1e-10 < err < 1e-5, err


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def test_bwd_f64_refuses_bad_arguments_without_a_gpu(built_lib):
    """Arguments are checked before any HIP call: a null pointer, an unknown mode or interpolation is CTPVAE_EINVAL."""
    lib = built_lib.load()
    fake = ctypes.c_void_p(256)          # never dereferenced: every call below fails its argument checks first
    geo = (2, 20, 184, 184)              # S, A, PH, PW
    tail = (128, 128, 28, 28)            # H, W, py, px
    rc = lib.ctpvae_rotate_bwd_f64(None, *geo, fake, 0, 0, *tail, fake, None)
    assert rc == built_lib.EINVAL and "null" in built_lib.last_error()
    rc = lib.ctpvae_rotate_bwd_f64(fake, *geo, fake, 0, 0, *tail, None, None)
    assert rc == built_lib.EINVAL and "null" in built_lib.last_error()
    rc = lib.ctpvae_rotate_bwd_f64(fake, *geo, fake, 0, 2, *tail, fake, None)
    assert rc == built_lib.EINVAL and "mode" in built_lib.last_error()
    rc = lib.ctpvae_rotate_bwd_f64(fake, *geo, fake, 2, 0, *tail, fake, None)
    assert rc == built_lib.EINVAL and "interpolation" in built_lib.last_error()
