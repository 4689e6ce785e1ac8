"""The compact tail section of the tf_compat backward plan, and the SHORT kernels' index requests -- no GPU needed.

Plan size (ctpvae_rotate_plan_bytes, which = 1): the uint4 array of NA16 = ceil(A / 16) groups, H x Wpad vectors each, and behind it,
for r = A mod 16 in 1 .. 12, records of t = ceil(r / 4) dwords per (row, padded column); nothing more for r = 0 and r >= 13.

Assembly (tools/count_bwd_tail_isa.py, rotate_plan.hip cross-compiled for gfx950) of the eight SHORT forms of the planned backward:
    * ahead of the first s_barrier the index requests are PPT global_load_dwordx4 for the full first vector, PPT global_load_dwordx4 for
      the whole last vector (the path of t = 4, and of knob BWD_TAIL = 0), and PPT loads of one, two and three dwords for the records --
      one block each, nothing else;
    * no scratch, and no more VGPRs than the build before the section existed (tests/golden/r17_rotate_plan_isa.json);
    * every other kernel of the file holds that build's instructions, one for one (sha256 of the listing, branch labels normalised).
      The file was recorded with `python tools/count_bwd_tail_isa.py --fingerprint <assembly of the parent commit>`; a later change
      that means to alter one of those kernels records it again."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "count_bwd_tail_isa.py")
spec = importlib.util.spec_from_file_location("count_bwd_tail_isa", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

needs_hipcc = pytest.mark.skipif(tool.base.find_hipcc() is None, reason="hipcc is not installed")
FORMS = {"rotate_bwd_planned_kernel%s<%s, 1, true>" % (wt, t) for wt in ("", "_wt") for t in ("2, 256, 2", "2, 1024, 2", "4, 256, 1", "4, 1024, 1")}


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


@pytest.fixture(scope="module")
def assembly():
    return tool.base.assembly()


@pytest.fixture(scope="module")
def parent():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "r17_rotate_plan_isa.json")))


@pytest.mark.parametrize("H,W", ((128, 128), (40, 72), (8, 8)))
@pytest.mark.parametrize("A,r,t", ((16, 0, 0), (32, 0, 0), (1, 1, 1), (17, 1, 1), (4, 4, 1), (20, 4, 1), (5, 5, 2), (21, 5, 2), (12, 12, 3), (28, 12, 3),
                                   (13, 13, 0), (29, 13, 0)))
def test_plan_bytes_hold_the_vectors_and_the_tail_records(built_lib, H, W, A, r, t):
    assert A % 16 == r
    lib = built_lib.load()
    P = lib.ctpvae_num_proj_pix(H, W)
    wpad = -(-W // 64) * 64
    vectors = -(-A // 16) * H * wpad * 16
    assert vectors % 256 == 0                                    # the section starts where the array ends
    assert lib.ctpvae_rotate_plan_bytes(H, W, P, P, A, 1) == vectors + t * H * wpad * 4


def test_knob_is_registered(built_lib):
    lib = built_lib.load()
    built_lib.tune("*")
    for v in (0, 1):
        assert lib.ctpvae_tune_set(b"BWD_TAIL", v) == 0
    built_lib.tune("*")
    assert lib.ctpvae_tune_active() == 0


@needs_hipcc
def test_short_forms_request_exactly_their_index_data(assembly, parent):
    counts = tool.count(assembly)
    assert set(counts) == FORMS == set(parent["short_vgprs"]), sorted(counts)
    for name, r in sorted(counts.items()):
        print(name, r)
        w, ppt = r["requests"], r["ppt"]
        assert w.count(4) == 2 * ppt and w.count(1) == w.count(2) == w.count(3) == ppt and len(w) == 5 * ppt, (name, w)
        for k in range(0, len(w), ppt):                          # block by block: one width, PPT loads
            assert len(set(w[k:k + ppt])) == 1, (name, w)
        assert r["scratch"] == 0, (name, r["scratch"])
        assert r["vgprs"] <= parent["short_vgprs"][name], (name, r["vgprs"], parent["short_vgprs"][name])


@needs_hipcc
def test_every_other_kernel_of_the_file_is_the_parents(assembly, parent):
    now = tool.fingerprint(assembly)["others"]
    assert set(now) == set(parent["others"])
    changed = sorted(n for n in now if now[n] != parent["others"][n])
    assert changed == ["rotate_bwd_plan_kernel"], changed        # the plan builder writes the section: the one kernel that may differ
