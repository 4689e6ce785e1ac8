"""The planned backward's SHORT form (tf_compat, at most 32 angles) against the CPU oracle, bit for bit, over its two ways of staging
cotangent rows: stage_contig_rows (detector rows of whole float4s in a 16-byte aligned tensor) and the general stagers behind the
barrier (every other geometry, and an aligned geometry whose tensor starts one float off), each at the library's own tile height and
with 4 / 8 / 13 / 16 waves forced (knob BW; small workgroups need more than one batch of loads for 32 rows).

Geometries: 128 x 128 padded (184 bins), 64 x 64 and 96 x 128 unpadded (64 / 128 bins) stage lean; 64 x 64 padded (94 bins) and
50 x 50 unpadded (50 bins) have PW % 4 != 0 and fall back, as does 128 x 128 with the cotangents offset by one float."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan

pytestmark = pytest.mark.gpu

GEOMS = {   # name: (H, W, pad, float offset of the cotangent tensor, stages lean)
    "128x128": (128, 128, True, 0, True),
    "64x64": (64, 64, False, 0, True),
    "96x128": (96, 128, False, 0, True),
    "64x64_padded_pw94": (64, 64, True, 0, False),
    "50x50_pw50": (50, 50, False, 0, False),
    "128x128_offset_one_float": (128, 128, True, 1, False),
}


@pytest.mark.parametrize("name", list(GEOMS))
@pytest.mark.parametrize("A", [1, 3, 16, 17, 20, 32])
def test_short_backward_equals_oracle(oracle, name, A):
    H, W, pad, off, lean = GEOMS[name]
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * A + H + W + off)
    theta = rng.uniform(-1.0, 4.0, A)
    plan = RotatePlan(theta, H, W, pad, d)
    plan.backward_uses_plan = lambda S: True          # the planned gather whatever the dispatch rule says
    plan.backward_uses_step_plan = lambda S: False
    assert (plan.PW % 4 == 0 and off == 0) == lean, (plan.PW, off)
    geom = oracle.Geometry(H, W, pad)
    Tinv = oracle.invert_transforms(oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW))
    for S in (1, 2, 3, 50):
        g_np = rng.standard_normal((S, A, plan.PW)).astype(np.float32)
        buf = torch.zeros(S * A * plan.PW + 4, dtype=torch.float32, device=d)   # (a fresh allocation is 16-byte aligned)
        g = buf[off: off + S * A * plan.PW].view(S, A, plan.PW)
        g.copy_(torch.from_numpy(g_np))
        assert g.is_contiguous() and (g.data_ptr() % 16 == 0) == (off == 0)
        want = torch.from_numpy(oracle.rotate_bwd_tfcompat(g_np, geom, Tinv, 0))
        got = plan.backward(g)
        assert torch.equal(got.cpu(), want), (name, A, S, "default tile")
        for waves in (4, 8, 13, 16):
            with _lib.tuned("BW", waves):
                got = plan.backward(g)
            assert torch.equal(got.cpu(), want), (name, A, S, waves)
