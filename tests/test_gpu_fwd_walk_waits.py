"""The planned u16 forward's walk (CTPVAE_FWD_WALK_U16, rotate_plan.hip: a single-exit loop of whole four-group trips, the last one to
four groups behind it) adds the same rows in the same order as before, on every path, whatever is in flight when a walk starts.

A wrong wait would show as stale taps that differ from run to run, so every case
  - equals the CPU oracle bit for bit (as tests/test_gpu_fwd_few_form.py compares),
  - is run by the general kernel (knob FWD_FEW=0) and by the few form (FWD_FEW=1), which must agree,
  - is launched three times per form, all three torch.equal.

Shapes, the smallest that reach every path:
  64 x 64 padded (92 bins, two bin blocks, up to 12 row groups of 8), 20 angles over 180 degrees, B = 1 (singles), 3 (a half-empty last
  pair) and 4.  Near 0 and 90 degrees the outer bin block's rays miss the image's rows, so its tasks have 0 or few groups; the central
  block's have up to 12: no trip at all (1..4 groups: only the tail), whole trips with every tail length.
  The same under knobs G=1, WAVES=4: one workgroup per (unit, class) with four waves takes ~20 tasks, so every wave walks several
  tasks in turn and a walk starts with the previous task's store and the next task's index loads pending -- a case the headline
  launch (one task per wave) never has.
  128 x 128 padded, B = 2, 20 angles: up to 23 groups, three bin blocks (the headline geometry).
The subset and log-likelihood-epilogue instantiations (rotate_fwd_planned_kernel<NS, EPI, SEL>) share the walk since this change; their
sinograms are compared with the same oracle rows, bit for bit, at the 64 x 64 shape."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan

pytestmark = pytest.mark.gpu

A = 20
SEVERAL_TASKS = (("G", 1), ("WAVES", 4))     # every wave takes several tasks in turn
CASES = [(64, B, knobs) for knobs in ((), SEVERAL_TASKS) for B in (1, 3, 4)] + [(128, 2, ())]
_shared = {}


def setup(oracle, N):
    """(plan, device images [4][N][N], oracle sinograms of all four) -- computed once per size and left unchanged"""
    if N not in _shared:
        d = torch.device("cuda", 0)
        theta = np.pi * np.arange(A) / A               # 0 and 90 degrees included
        plan = RotatePlan(theta, N, N, True, d, plan_format="u16")
        x_np = np.random.default_rng(16 + N).standard_normal((4, N, N)).astype(np.float32)
        T = oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW)
        want = torch.from_numpy(oracle.rotate_fwd(x_np, oracle.Geometry(N, N, True), T, 0))
        _shared[N] = (plan, torch.from_numpy(x_np).to(d), want)
    return _shared[N]


@pytest.mark.parametrize("N,B,knobs", CASES, ids=lambda v: "-".join("%s%d" % kv for kv in v) or "rule" if isinstance(v, tuple) else str(v))
def test_walk_equals_oracle_in_both_forms_and_repeats(oracle, N, B, knobs):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    plan, x_all, want_all = setup(oracle, N)
    x, want = x_all[:B], want_all[:B]
    runs = {}
    try:
        for kname, v in knobs:
            _lib.tune(kname, v)
        for few in (0, 1):
            _lib.tune("FWD_FEW", few)
            assert plan.forward_form(B, x) == few, (N, B, knobs, few)
            runs[few] = [plan.forward(x) for _ in range(3)]
    finally:
        _lib.tune("*")
    torch.cuda.synchronize()
    for few, outs in runs.items():
        assert torch.equal(outs[0].cpu(), want), (N, B, knobs, few, "oracle")
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (N, B, knobs, few, "run to run")
    assert torch.equal(runs[0][0], runs[1][0]), (N, B, knobs, "general kernel against few form")


@pytest.mark.parametrize("knobs", [(), SEVERAL_TASKS], ids=["rule", "G1-WAVES4"])
@pytest.mark.parametrize("B", [1, 3])
def test_subset_and_epilogue_kernels_add_the_same_rows(oracle, B, knobs):
    plan, x_all, want_all = setup(oracle, 64)
    d = x_all.device
    x, want = x_all[:B], want_all[:B]
    sel_np = np.random.default_rng(3).permutation(A)[:7].astype(np.int32)
    sel, rows = torch.from_numpy(sel_np).to(d), torch.from_numpy(sel_np).long()
    rng = np.random.default_rng(4)
    mask = torch.full((B, A), 0.05, device=d)
    meas = torch.from_numpy(rng.random((B, A, plan.PW)).astype(np.float32)).to(d)
    pnm = torch.tensor(1e4, device=d)
    try:
        for kname, v in knobs:
            _lib.tune(kname, v)
        got = {
            "subset": ([plan.forward(x, angles_i=sel) for _ in range(3)], want[:, rows]),
            "epilogue": ([plan.forward_loglik(x, mask, meas, pnm, 1e-7)[0] for _ in range(3)], want),
            "subset + epilogue": ([plan.forward_loglik(x, mask, meas, pnm, 1e-7, angles_i=sel, dense_inputs=True)[0] for _ in range(3)],
                                  want[:, rows]),
        }
    finally:
        _lib.tune("*")
    torch.cuda.synchronize()
    for what, (outs, w) in got.items():
        assert torch.equal(outs[0].cpu(), w), (B, knobs, what, "oracle")
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (B, knobs, what, "run to run")
