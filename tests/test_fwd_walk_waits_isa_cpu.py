"""The walk loop of the planned u16 forward keeps its loads in flight: no s_waitcnt inside it empties a counter -- checked in the gfx950
assembly of all ten forward kernels, no GPU needed (tools/count_loop_header_waits.py).

The walk (CTPVAE_FWD_WALK_U16, rotate_plan.hip) keeps four index vectors in flight and gathers group n + 1 under the adds of group n.
The walk loop is the innermost loop holding 32 LDS gathers (four groups of eight).  In it
  - no wait asks for vmcnt below 3: a group's index vector is waited for with the three younger requests still out;
  - no wait asks for lgkmcnt below 8 in the pair kernels (NS = 2) or below 7 in the singles: the adds of a group wait for its own eight
    gathers one by one while the next group's eight stay out.  (This build: 8 in all ten.)
Until this change every trip opened with s_waitcnt vmcnt(0), with lgkmcnt(0) or lgkmcnt(7) beside it in eight of the ten kernels: the loop
left through a `break` per group, hipcc routed every break through the loop's one latch block, and the wait inserter met at the header the
state of each break -- an index vector and eight gathers just issued (profiles/r16_fwd_walk_waits_isa.txt).
No kernel keeps the old walk."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "count_loop_header_waits.py")
spec = importlib.util.spec_from_file_location("count_loop_header_waits", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

KERNELS = ["rotate_fwd_planned_kernel_few<%d>" % ns for ns in (1, 2)] + [
    "rotate_fwd_planned_kernel<%d, %s, %s>" % (ns, epi, sel) for ns in (1, 2) for epi in ("false", "true") for sel in ("false", "true")]
MIN_VMCNT = 3                # index vectors that stay in flight
MIN_LGKMCNT = {2: 8, 1: 7}   # gathers of one group


@pytest.fixture(scope="module")
def loops():
    return tool.loops(tool.assembly(), "rotate_fwd_planned_kernel")


@pytest.mark.skipif(tool.find_hipcc() is None, reason="hipcc is not installed")
@pytest.mark.parametrize("kernel", KERNELS)
def test_walk_loop_drains_no_counter(loops, kernel):
    assert kernel in loops, sorted(loops)
    walks = [lp for lp in loops[kernel] if lp["inner"] and lp["ds_reads"] == 32]
    assert len(walks) == 1, (kernel, loops[kernel])
    walk = walks[0]
    ns = int(kernel.split("<")[1][0])
    print(kernel, {k: walk[k] for k in ("header", "header_waits", "min_vmcnt", "min_lgkmcnt", "global_loads")})
    assert walk["global_loads"] == 4, (kernel, walk)             # the four index vectors of a trip
    assert walk["min_vmcnt"] is not None and walk["min_lgkmcnt"] is not None, (kernel, walk)   # it does wait for both
    assert walk["min_vmcnt"] >= MIN_VMCNT, (kernel, walk["waits"])
    assert walk["min_lgkmcnt"] >= MIN_LGKMCNT[ns], (kernel, walk["waits"])
