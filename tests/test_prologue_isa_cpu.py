"""The planned backward's SHORT pair instantiations (the headline adjoint: 50 x 128 x 128, 20 angles) keep a short, division-free
prologue -- checked in the gfx950 assembly, no GPU needed (tools/count_prologue_isa.py).

Static instructions ahead of the first s_barrier of rotate_bwd_planned_kernel<2, 1024, 2, 1, true>:
    before the SHORT form was written for it   426   (and that barrier stood IN FRONT of the row staging, ~900 more instructions,
                                                      with 6 v_rcp_iflag_f32 and 8 s_abs_i32 of integer divisions)
    now                                        345   (the whole prologue: decode, index requests, staging, zero cells; no division)
The bound is a regression guard, not a target: this build's count plus 10 % = 379, below the 426 it started from."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "count_prologue_isa.py")
spec = importlib.util.spec_from_file_location("count_prologue_isa", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

PARENT = 426
BOUND = 379


@pytest.mark.skipif(tool.find_hipcc() is None, reason="hipcc is not installed")
def test_short_pair_prologue_is_lean_and_division_free():
    res = tool.count(tool.assembly())
    short_pairs = {k: v for k, v in res.items() if k.replace(" ", "") in ("rotate_bwd_planned_kernel<2,1024,2,1,true>",
                                                                           "rotate_bwd_planned_kernel<2,256,2,1,true>")}
    assert len(short_pairs) == 2, sorted(res)
    for name, r in short_pairs.items():
        print(name, r)
        assert r["prologue"] < r["total"], (name, r)          # there is a barrier
        assert r["v_rcp_iflag_f32"] == 0 and r["s_abs_i32"] == 0, (name, r)
        assert r["prologue"] <= BOUND < PARENT, (name, r)
