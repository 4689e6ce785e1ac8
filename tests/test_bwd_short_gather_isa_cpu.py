"""The gather phase of the planned backward's SHORT forms (at most 32 angles: the headline adjoint) executes the taps its launch has
and nothing in their place -- checked in the gfx950 assembly, no GPU needed (tools/count_bwd_gather_isa.py).

A launch of A angles consumes na4 / 4 = 1 .. 8 index dwords per owned row (na4 = A rounded up to 4): a full index vector when A > 16,
then a tail of t = 1 .. 4 dwords, each as its own straight-line code.  Behind the last s_barrier of each of the four SHORT
instantiations and their write-through twins:
    * at most PPT x NS registers are zeroed (`v_mov_b32 vN, 0`: the accumulators may be) -- the form that zero-filled the dwords a
      launch does not have held 98 in the pair kernels;
    * every basic block that gathers holds, for one t in 1 .. 4, exactly 4 t PPT SDWA unpacks, 4 t PPT LDS reads and 4 t PPT adds;
      every t occurs, and t = 4 at least twice: the full vector ahead of a tail and the tail of four;
    * no scratch."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "count_bwd_gather_isa.py")
spec = importlib.util.spec_from_file_location("count_bwd_gather_isa", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

needs_hipcc = pytest.mark.skipif(tool.base.find_hipcc() is None, reason="hipcc is not installed")
FORMS = {"rotate_bwd_planned_kernel%s<%s, 1, true>" % (wt, t) for wt in ("", "_wt") for t in ("2, 256, 2", "2, 1024, 2", "4, 256, 1", "4, 1024, 1")}


@pytest.fixture(scope="module")
def counts():
    return tool.count(tool.base.assembly())


@needs_hipcc
def test_the_eight_short_forms_are_there_without_scratch(counts):
    assert set(counts) == FORMS, sorted(counts)
    for name, r in counts.items():
        assert r["scratch"] == 0, (name, r["scratch"])


@needs_hipcc
def test_no_register_is_zeroed_to_stand_in_for_a_tap(counts):
    for name, r in sorted(counts.items()):
        print(name, "zeroing moves behind the last barrier:", r["zero_movs"], "allowance", r["ppt"] * r["ns"])
        assert r["zero_movs"] <= r["ppt"] * r["ns"], (name, r["zero_movs"])


@needs_hipcc
def test_each_straight_line_case_holds_exactly_its_taps(counts):
    for name, r in sorted(counts.items()):
        print(name, r["blocks"])
        seen = []
        for unpacks, reads, adds in r["blocks"]:
            assert unpacks == reads == adds, (name, unpacks, reads, adds)
            assert unpacks % (4 * r["ppt"]) == 0 and 1 <= unpacks // (4 * r["ppt"]) <= 4, (name, unpacks)
            seen.append(unpacks // (4 * r["ppt"]))
        assert set(seen) == {1, 2, 3, 4}, (name, seen)
        assert seen.count(4) >= 2, (name, seen)      # the full group of 16 x PPT, and the tail of four dwords
