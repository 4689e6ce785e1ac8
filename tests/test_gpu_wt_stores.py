"""The store policy of the planned nearest projector pair's output stores (knob WT_STORES: 0 plain, 1 write-through, 2 non-temporal)
changes no bit: every launch below runs under 0, 1 and 2 into NaN-filled outputs, the three results are equal and hold no NaN.  That
the default rule's forms equal the oracle is tests/test_gpu_parity.py's and tests/test_gpu_fwd_few_form.py's business.

Shapes, the smallest at which a store can go wrong:
    few forward      S = 1 and 3 of 64 x 64 padded, 5 angles: an odd S ends with a lone slice of a pair, and the padded detector (94 bins) is one
                     ragged bin block of 64-lane tasks
    general forward  S = 3 of 40 x 36 padded, 7 angles (no power-of-two unit: the general kernel)
    SHORT adjoint    S = 1 and 3 of 64 x 64 x 5 angles and of 40 x 36 x 7 angles (a ragged column block, a last tile shorter than the tile
                     height), each with and without a per-slice scale
    general adjoint  S = 3 of 40 x 36 x 33 angles (more than 32: two staged groups and a partial third)"""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan

pytestmark = pytest.mark.gpu

POLICIES = (0, 1, 2)


def plan_for(H, W, A, seed):
    d = torch.device("cuda", 0)
    theta = np.random.default_rng(seed).uniform(-1.0, 4.0, A)
    return RotatePlan(theta, H, W, True, d, plan_format="u16"), d


def under_every_policy(run, shape, d):
    outs = []
    for st in POLICIES:
        out = torch.full(shape, float("nan"), device=d)
        with _lib.tuned("WT_STORES", st):
            run(out)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any(), st
        outs.append(out)
    for st, out in zip(POLICIES[1:], outs[1:]):
        assert torch.equal(out, outs[0]), st


@pytest.mark.parametrize("H,W,A,S,few", [(64, 64, 5, 1, 1), (64, 64, 5, 3, 1), (40, 36, 7, 3, 0)])
def test_forward_stores_equal_bits_under_every_policy(H, W, A, S, few):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    plan, d = plan_for(H, W, A, 10 * H + S)
    assert plan.PW % 64 != 0                                    # a ragged last bin block
    x = torch.from_numpy(np.random.default_rng(S).standard_normal((S, H, W)).astype(np.float32)).to(d)
    assert plan.forward_kernel_name(S) == "rotate_fwd_planned_kernel" and plan.forward_form(S, x) == few
    under_every_policy(lambda out: plan.forward(x, out=out), (S, A, plan.PW), d)


def adjoint_case(H, W, A, S, scaled):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    plan, d = plan_for(H, W, A, 10 * H + S + 1)
    rng = np.random.default_rng(100 + S)
    gs = torch.from_numpy(rng.standard_normal((S, A, plan.PW)).astype(np.float32)).to(d)
    scale = torch.from_numpy(rng.uniform(0.5, 2.0, S).astype(np.float32)).to(d) if scaled else None
    assert plan.backward_kernel_name(S) == "rotate_bwd_planned_kernel"
    under_every_policy(lambda out: plan.backward(gs, out=out, scale=scale), (S, H, W), d)


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("H,W,A,S", [(64, 64, 5, 1), (64, 64, 5, 3), (40, 36, 7, 1), (40, 36, 7, 3)])
def test_short_adjoint_stores_equal_bits_under_every_policy(H, W, A, S, scaled):
    adjoint_case(H, W, A, S, scaled)


def test_general_adjoint_stores_equal_bits_under_every_policy():
    adjoint_case(40, 36, 33, 3, False)
