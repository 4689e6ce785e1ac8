"""The planned forward's FEW form (rotate_fwd_planned_kernel_few<1> / <2>: the headline forward, 50 x 128 x 128, 20 angles, runs <2>)
keeps a short, division-free prologue -- checked in the gfx950 assembly, no GPU needed (tools/count_prologue_isa.py).

Static instructions ahead of the first s_barrier:
                                               pairs (NS = 2)    singles (NS = 1)
    rotate_fwd_planned_kernel<NS, false, false>    1926              1833     (the parent's kernel for these launches: every staging
                                                                               form, the three-part piece list, the affine shape, 14 / 11
                                                                               v_rcp_iflag_f32 and 14 / 11 s_abs_i32 of integer divisions)
    rotate_fwd_planned_kernel_few<NS>               550               703     (decode, first task, both mirror forms of the lean stager,
                                                                               zero cell, task counter; no division)
The bounds are regression guards, not targets: this build's counts plus 10 % = 605 and 773, below the 1926 and 1833 they started from."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "count_prologue_isa.py")
spec = importlib.util.spec_from_file_location("count_prologue_isa", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

PARENT = {2: 1926, 1: 1833}
BOUND = {2: 605, 1: 773}


@pytest.mark.skipif(tool.find_hipcc() is None, reason="hipcc is not installed")
def test_few_form_prologue_is_lean_and_division_free():
    res = tool.count(tool.assembly(), "rotate_fwd_planned_kernel")
    few = {ns: res.get("rotate_fwd_planned_kernel_few<%d>" % ns) for ns in (1, 2)}
    assert all(few.values()), sorted(res)
    for ns, r in few.items():
        print(ns, r)
        assert r["prologue"] < r["total"], (ns, r)          # there is a barrier
        assert r["v_rcp_iflag_f32"] == 0 and r["s_abs_i32"] == 0, (ns, r)
        assert r["prologue"] <= BOUND[ns] < PARENT[ns], (ns, r)
