"""Which form of the ray-driven forward a launch takes (ctpvae_siddon_fwd_form, host only: no GPU needed) -- 0 = one slice per
workgroup read from global memory, 1 = one slice in LDS, 2 = a slice pair in LDS, 4 / 8 = the packed walk.  The CHOICE is asserted
here, at the edges of the rule derived from the code's own constants; the bits of every form in tests/test_gpu_siddon_matrix.py.

The constants (csrc/common.h, csrc/siddon.hip siddon_fwd_form_rule): 160 KiB of LDS; a slice takes ox * pitch * 4 bytes with
pitch = oz + ((1 - (oz & 31)) & 31); the packed walk serves 4 slices from 3 slices on and 8 from 6 on; where a PAIR fits LDS, up to
750 waves of pairs (ceil(oy / 2) * dt * dx <= 750 * 64 rays) keep the LDS kernels; pairs only above 500 waves (oy * dt * dx > 500 * 64
rays)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

GLOBAL, ONE, PAIR, QUAD, OCT = 0, 1, 2, 4, 8
LDS_BYTES = 160 * 1024
STORES = ("raysum", "sirt", "tv_dual", "gaussian", "poisson", "ratio")


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def form(lib, oy, ox, oz, dt, dx, store="raysum"):
    f = lib.load().ctpvae_siddon_fwd_form(oy, ox, oz, dt, dx, lib.SIDDON_STORE[store])
    if f in (QUAD, OCT):      # the size rule and the dispatch ask one function: a packed form always has its workspace
        assert lib.load().ctpvae_siddon_fwd_workspace_bytes(oy, ox, oz) == -(-oy // f) * f * ox * oz * 4, (oy, ox, oz, dt, dx, store)
    return f


def slice_bytes(ox, oz):
    return ox * (oz + ((1 - (oz & 31)) & 31)) * 4


def test_the_constants_of_this_file_are_the_headers(built_lib):
    import re
    text = open(os.path.join(ROOT, "include", "ctpvae_radon.h")).read()
    for name, value in built_lib.SIDDON_STORE.items():
        assert int(re.search(rf"#define\s+CTPVAE_SIDDON_STORE_{name.upper()}\s+(\d+)", text).group(1)) == value
    assert tuple(sorted(built_lib.SIDDON_STORE, key=built_lib.SIDDON_STORE.get)) == STORES
    common = open(os.path.join(ROOT, "ct_pvae_amd", "csrc", "common.h")).read()
    assert re.search(r"kMaxLdsBytes\s*=\s*160\s*\*\s*1024", common)


def test_lds_fit(built_lib):
    """Many slices of many rays (no wave threshold in the way), knob SIDDON_NS = 2: a pair where it fits, else one slice, else
    global memory; SIDDON_NS = 1: one slice where it fits."""
    assert slice_bytes(100, 258) == 100 * 289 * 4 <= LDS_BYTES < 2 * slice_bytes(100, 258)
    assert slice_bytes(160, 258) == 160 * 289 * 4 > LDS_BYTES
    assert 2 * slice_bytes(128, 128) == 2 * 128 * 129 * 4 <= LDS_BYTES               # the training set's images: pairs
    assert slice_bytes(184, 184) == 184 * 193 * 4 <= LDS_BYTES < 2 * slice_bytes(184, 184)     # their reconstruction grid: no pair
    for store in STORES:
        with built_lib.tuned("SIDDON_NS", 2):
            assert form(built_lib, 9, 128, 128, 17, 184, store) == PAIR
            assert form(built_lib, 9, 100, 258, 17, 200, store) == ONE               # the fallback of 2 to 1
            assert form(built_lib, 9, 184, 184, 17, 262, store) == ONE
            assert form(built_lib, 9, 160, 258, 17, 200, store) == GLOBAL
            assert form(built_lib, 9, 12, 70, 17, 200, store) == PAIR and form(built_lib, 9, 33, 47, 17, 59, store) == PAIR
        with built_lib.tuned("SIDDON_NS", 1):
            assert form(built_lib, 9, 128, 128, 17, 184, store) == ONE
            assert form(built_lib, 9, 100, 258, 17, 200, store) == ONE
            assert form(built_lib, 9, 160, 258, 17, 200, store) == GLOBAL
    # the edge itself, one row either side: 258 columns have a pitch of 289 words, 160 KiB / (289 * 4) = 141.7 rows
    with built_lib.tuned("SIDDON_NS", 1):
        assert slice_bytes(141, 258) <= LDS_BYTES < slice_bytes(142, 258)
        assert form(built_lib, 2, 141, 258, 17, 200) == ONE and form(built_lib, 2, 142, 258, 17, 200) == GLOBAL
    with built_lib.tuned("SIDDON_NS", 2):
        assert 2 * slice_bytes(70, 258) <= LDS_BYTES < 2 * slice_bytes(71, 258)
        assert form(built_lib, 2, 70, 258, 17, 200) == PAIR and form(built_lib, 2, 71, 258, 17, 200) == ONE


def test_packed_thresholds_of_the_slice_count(built_lib):
    """No knob, a grid whose pair does not fit LDS (so the wave rule does not apply): 4 slices per walk from 3 slices on, 8 from 6 on;
    the Poisson likelihood never takes the packed walk."""
    for ox, oz, dx, lds in ((184, 184, 262, ONE), (100, 258, 200, ONE), (160, 258, 200, GLOBAL)):
        for store in STORES:
            want = {1: lds, 2: lds, 3: QUAD, 5: QUAD, 6: OCT, 9: OCT, 50: OCT}
            for oy, f in want.items():
                assert form(built_lib, oy, ox, oz, 17, dx, store) == (lds if store == "poisson" else f), (ox, oz, oy, store)
    assert built_lib.load().ctpvae_siddon_fwd_workspace_bytes(2, 184, 184) == 0
    assert built_lib.load().ctpvae_siddon_fwd_workspace_bytes(3, 184, 184) == 4 * 184 * 184 * 4
    assert built_lib.load().ctpvae_siddon_fwd_workspace_bytes(6, 184, 184) == 8 * 184 * 184 * 4


def test_750_waves_of_pairs_keep_lds(built_lib):
    """Where a pair fits: ceil(oy / 2) * dt * dx <= 48000 rays keep the LDS kernels, one ray more takes the packed walk."""
    for store in STORES:
        packed = store != "poisson"
        assert form(built_lib, 3, 128, 128, 1, 24000, store) == PAIR                         # 2 * 24000 = 48000
        assert form(built_lib, 3, 128, 128, 1, 24001, store) == (QUAD if packed else PAIR)   # 48002
        assert form(built_lib, 6, 128, 128, 125, 128, store) == PAIR                         # 3 * 125 * 128 = 48000
        assert form(built_lib, 6, 128, 128, 126, 128, store) == (OCT if packed else PAIR)
        assert form(built_lib, 16, 128, 128, 20, 184, store) == PAIR                         # the measured case: 460 waves of pairs
        assert form(built_lib, 32, 128, 128, 20, 184, store) == (OCT if packed else PAIR)    # 920
    # a grid whose pair does not fit has no LDS pairs to keep: packed however few the rays
    assert form(built_lib, 3, 184, 184, 1, 8) == QUAD and form(built_lib, 3, 100, 258, 1, 8) == QUAD
    # the size rule cannot know dt and dx: it answers for the largest launch
    assert built_lib.load().ctpvae_siddon_fwd_workspace_bytes(3, 128, 128) == 4 * 128 * 128 * 4


def test_pairs_only_above_500_waves(built_lib):
    """oy * dt * dx > 32000 rays: pairs; up to there single slices (more workgroups of the same walk)."""
    for store in STORES:
        assert form(built_lib, 2, 128, 128, 1, 16000, store) == ONE          # 32000
        assert form(built_lib, 2, 128, 128, 1, 16001, store) == PAIR         # 32002
        assert form(built_lib, 5, 128, 128, 1, 6400, store) == ONE           # 32000 (3 pairs x 6400 rays: LDS either way)
        assert form(built_lib, 5, 128, 128, 1, 6401, store) == PAIR          # 32005
        assert form(built_lib, 1, 128, 128, 180, 184, store) == ONE          # nothing to pair
        assert form(built_lib, 8, 128, 128, 20, 184, store) == ONE           # the measured case: 460 waves
    assert form(built_lib, 5, 100, 258, 17, 200, "poisson") == ONE and form(built_lib, 5, 160, 258, 17, 200, "poisson") == GLOBAL


def test_every_knob_value(built_lib):
    for store in STORES:
        packed = store != "poisson"
        for oy in (1, 3, 5, 9):
            with built_lib.tuned("SIDDON_NS", 1):
                assert form(built_lib, oy, 128, 128, 180, 184, store) == ONE
            with built_lib.tuned("SIDDON_NS", 2):      # a pair wherever there are two slices, whatever the number of waves
                assert form(built_lib, oy, 128, 128, 1, 8, store) == (PAIR if oy >= 2 else ONE)
                assert form(built_lib, oy, 100, 258, 17, 200, store) == ONE
                assert form(built_lib, oy, 160, 258, 17, 200, store) == GLOBAL
            for ns in (QUAD, OCT):                    # the packed walk however few the slices or the rays
                with built_lib.tuned("SIDDON_NS", ns):
                    assert form(built_lib, oy, 128, 128, 1, 8, store) == (ns if packed else ONE)
                    assert form(built_lib, oy, 160, 258, 17, 200, store) == (ns if packed else GLOBAL)
        with built_lib.tuned("SIDDON_NS", 3):          # not a form: the slice-count rule, and single slices where that gives none
            assert form(built_lib, 9, 128, 128, 1, 8, store) == (OCT if packed else ONE)
            assert form(built_lib, 2, 128, 128, 180, 184, store) == ONE
    assert form(built_lib, 9, 128, 128, 180, 184) == OCT        # ... and unset again


def test_chunked_batches_answer_for_their_first_chunk(built_lib):
    """MAX_SLICES cuts the batches of the LDS / global-memory kernels into even chunks; the packed walk is not cut."""
    assert form(built_lib, 11, 128, 128, 17, 184) == PAIR              # 6 x 17 x 184 rays: LDS, and 11 x 17 x 184 > 32000: pairs
    with built_lib.tuned("MAX_SLICES", 4):
        assert form(built_lib, 11, 128, 128, 17, 184) == ONE           # chunks of 4: 4 x 17 x 184 = 12512 rays
        assert form(built_lib, 11, 128, 128, 64, 184) == OCT           # 6 x 64 x 184 > 48000: packed
    with built_lib.tuned("MAX_SLICES", 1):                             # (chunks are whole pairs: at least 2)
        with built_lib.tuned("SIDDON_NS", 2):
            assert form(built_lib, 11, 128, 128, 17, 184) == PAIR


def test_bad_arguments(built_lib):
    lib = built_lib.load()
    for args in ((0, 8, 8, 1, 8, 0), (1, 0, 8, 1, 8, 0), (1, 8, 0, 1, 8, 0), (1, 8, 8, 0, 8, 0), (1, 8, 8, 1, 0, 0), (1, 8, 8, 1, 8, 6),
                 (1, 8, 8, 1, 8, -1)):
        assert lib.ctpvae_siddon_fwd_form(*args) == built_lib.EINVAL, args
    assert "store" in built_lib.last_error()
