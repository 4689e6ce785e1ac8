"""Which form of the planned u16 forward a launch takes (ctpvae_rotate_fwd_planned_form, host only: no GPU needed): the lean form
rotate_fwd_planned_kernel_few for dense one-part launches whose unit stages in one batch of aligned 16-byte loads, the general
kernel for everything else -- the CHOICE is asserted here, the bits in tests/test_gpu_fwd_few_form.py."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

FEW, GENERAL = 1, 0


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def form(lib, S, H, W, A, aligned=1, pad=True):
    PH, PW = (lib.ctpvae_num_proj_pix(H, W),) * 2 if pad else (H, W)
    return lib.ctpvae_rotate_fwd_planned_form(S, H, W, PH, PW, A, aligned)


def test_headline_geometry_takes_the_few_form_at_every_one_round_batch(built_lib):
    lib = built_lib.load()
    for B in (1, 2, 5, 25, 50):
        assert form(lib, B, 128, 128, 20) == FEW, B
        assert form(lib, B, 128, 128, 20, aligned=0) == GENERAL, B     # 16-byte loads need an aligned image


def test_units_the_lean_stager_cannot_serve_keep_the_general_kernel(built_lib):
    lib = built_lib.load()
    for B in (1, 5, 50):
        assert form(lib, B, 100, 100, 20) == GENERAL, B     # 100 columns: no power-of-two unit
        assert form(lib, B, 126, 128, 20) == GENERAL, B     # rows not in fours


def test_several_part_piece_lists_keep_the_general_kernel(built_lib):
    """B = 200 x 20 angles cut into two parts (single slices; knobs MIXG_G2 / MIXG_U1: the first 120 slices' pieces, then 80 slices
    x 3 task groups), and the library's own several-part cuts at B = 300 and 301 (test_two_part_piece_lists_equal_one_cut of
    tests/test_gpu_parity.py).  The library's own shape at B = 200 x 20 is ONE part -- 100 pairs x 2 classes = 200 pieces, one
    round of workgroups -- and takes the few form, as the rule says."""
    lib = built_lib.load()
    with built_lib.tuned("NS", 1), built_lib.tuned("MIXG_G2", 3), built_lib.tuned("MIXG_U1", 120):
        assert form(lib, 200, 128, 128, 20) == GENERAL
    with built_lib.tuned("NS", 1), built_lib.tuned("MIXG", 0):
        assert form(lib, 200, 128, 128, 20) == FEW
    for B in (300, 301):
        assert form(lib, B, 128, 128, 20) == GENERAL, B
        with built_lib.tuned("MIXG", 0):     # the same launch as ONE part of pieces: nothing else stands in the way
            assert form(lib, B, 128, 128, 20) == FEW, B
    assert form(lib, 200, 128, 128, 20) == FEW


def test_knob_fwd_few_0_forces_the_general_kernel(built_lib):
    lib = built_lib.load()
    with built_lib.tuned("FWD_FEW", 0):
        for B in (1, 2, 5, 25, 50, 200):
            for H, W in ((128, 128), (64, 64), (100, 100)):
                assert form(lib, B, H, W, 20) == GENERAL, (B, H, W)
    with built_lib.tuned("FWD_FEW", 1):     # 1 = wherever the conditions hold: never where they do not
        assert form(lib, 50, 128, 128, 20) == FEW
        assert form(lib, 50, 100, 100, 20) == GENERAL and form(lib, 50, 128, 128, 20, aligned=0) == GENERAL


def test_two_batches_of_loads_keep_the_general_kernel(built_lib):
    """A pair of 128 x 128 slices is 64 blocks of 4 rows x 64 columns, four per wave and batch: 8 waves would need two batches."""
    lib = built_lib.load()
    with built_lib.tuned("NS", 2), built_lib.tuned("WAVES", 8):
        assert form(lib, 50, 128, 128, 20) == GENERAL
    with built_lib.tuned("NS", 2), built_lib.tuned("WAVES", 16):
        assert form(lib, 50, 128, 128, 20) == FEW
    with built_lib.tuned("NS", 1), built_lib.tuned("WAVES", 8):     # single slices: eight blocks per wave and batch
        assert form(lib, 50, 128, 128, 20) == FEW


def test_other_launch_shapes_keep_the_general_kernel(built_lib):
    lib = built_lib.load()
    with built_lib.tuned("NO_MAGIC", 1):     # divisions: the few form has none to fall back on
        assert form(lib, 50, 128, 128, 20) == GENERAL
    with built_lib.tuned("AFFINE", 1):       # angles dealt to the XCDs
        assert form(lib, 8, 128, 128, 180) == GENERAL
    assert form(lib, 0, 128, 128, 20) == built_lib.EINVAL


def test_many_tasks_per_workgroup_keep_the_general_kernel(built_lib):
    """At most 48 tasks per workgroup (measured: the few form loses at 54, B = 50 x 180 angles, and wins at 30 and below); knob
    FWD_FEW=1 lifts the bound, nothing else."""
    lib = built_lib.load()
    assert form(lib, 50, 128, 128, 180) == GENERAL          # 540 tasks per slice pair on 10 workgroups
    with built_lib.tuned("FWD_FEW", 1):
        assert form(lib, 50, 128, 128, 180) == FEW
    with built_lib.tuned("NS", 2), built_lib.tuned("G", 1):
        assert form(lib, 50, 128, 128, 32) == FEW           # 48 per workgroup
        assert form(lib, 50, 128, 128, 33) == GENERAL       # 50
    assert form(lib, 400, 128, 128, 20) == FEW              # 30
