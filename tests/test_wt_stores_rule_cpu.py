"""Knob WT_STORES (the store policy of the kernels that have more than one: 0 plain, 1 write-through, 2 non-temporal, unset = the
launch's rule) in the registry -- host only, no GPU needed: it is registered, takes 0, 1 and 2, is unset by a negative value and by the
reset of every knob, and the tests' own reset fixture (tests/conftest.py) clears it between tests."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def test_knob_is_registered_and_takes_every_policy(built_lib):
    lib = built_lib.load()
    built_lib.tune("*")
    assert lib.ctpvae_tune_active() == 0
    for v in (0, 1, 2):
        assert lib.ctpvae_tune_set(b"WT_STORES", v) == 0, v
        assert lib.ctpvae_tune_active() == 1
    assert lib.ctpvae_tune_set(b"WT_STORES", -1) == 0 and lib.ctpvae_tune_active() == 0
    assert lib.ctpvae_tune_set(b"WT_STORE", 1) == built_lib.EINVAL          # (an unknown name is refused: the knob above is not)
    with built_lib.tuned("WT_STORES", 1):
        assert lib.ctpvae_tune_active() == 1
    assert lib.ctpvae_tune_active() == 0
    built_lib.tune("WT_STORES", 2)
    built_lib.tune("*")
    assert lib.ctpvae_tune_active() == 0


def test_a_test_may_leave_the_knob_set(built_lib):
    built_lib.tune("WT_STORES", 1)
    assert built_lib.load().ctpvae_tune_active() == 1


def test_the_reset_fixture_has_cleared_it(built_lib):
    assert built_lib.load().ctpvae_tune_active() == 0
