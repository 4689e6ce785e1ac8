"""The few-angle (SHORT) planned adjoint reads the live dwords of its last index vector from the plan's compact tail section
(A mod 16 = 1 .. 12: records of 1 .. 3 dwords per row and padded column) where it read the whole uint4 before: the same taps in
the same order, so the same bits -- as knob BWD_TAIL = 0 (the uint4, the form from before the section) and as the CPU oracle's
rotate_bwd_tfcompat (NEAREST), through RotatePlan.backward as tests/test_gpu_bwd_short_tails.py.

Angle counts  1, 4, 5, 8, 12 (records alone: the launch loads no uint4), 13, 16 (one whole vector), 17, 20, 21, 24, 28 (a full
              vector, then records of 1, 2, 3 dwords), 29, 32 (two whole vectors); angles random in (-1, 4) rad, seeded.
Shapes        padded slices of 8 x 8 (W < 64, fewer rows than a tile), 40 x 40 (one ragged column block, single slices in tiles
              taller than the last) and 72 x 72 (two column blocks, the second ragged; pairs).  The planned adjoint is asked for
              whatever the Python rule would pick for so small a slice: the entry point is ctpvae_rotate_bwd_planned_scaled_f32.
Batch sizes   1, 2, 3: the single-slice form, a pair, a half-empty pair.
Cotangents    a 16-byte aligned tensor (stage_contig_rows where the bins allow it) and the same values 4 bytes further on (the
              general stager: stage_magic == 0); standard normal with a sprinkling of -0.0f.
Scale         none, and one factor per slice.
Outputs       NaN before every call.
The oracle's gradient is computed once per (shape, A) for three slices; the smaller batches are its first slices.  One more case
runs the benchmark's adjoint (50 x 128 x 128, 20 angles) against BWD_TAIL = 0 under write-through and under plain stores, and one
the two cells of 128 x 128 slices whose tiles are eleven waves tall (40 and 80 slices) against the 16-row tiles of knob BW = 8."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan, num_proj_pix

pytestmark = pytest.mark.gpu

ANGLES = (1, 4, 5, 8, 12, 13, 16, 17, 20, 21, 24, 28, 29, 32)
SIZES = (8, 40, 72)
BATCHES = (1, 2, 3)
SMAX = max(BATCHES)


def planned(theta, N, d):
    plan = RotatePlan(theta, N, N, True, d, plan_format="u16")
    assert plan._want_bwd_plan
    plan.backward_uses_plan = lambda S: True
    plan.backward_uses_step_plan = lambda S: False
    return plan


def shifted(t):
    """the values of t in memory that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    off = (1 - buf.data_ptr() // 4) % 4                          # buf[off] is 4 bytes past a 16-byte boundary
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("A", ANGLES)
@pytest.mark.parametrize("N", SIZES)
def test_compact_tail_equals_the_whole_vector_and_the_oracle(oracle, N, A):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda", 0)
    theta = np.random.default_rng(1000 * N + A).uniform(-1.0, 4.0, A)
    plan = planned(theta, N, d)
    PW = num_proj_pix(N, N)
    assert plan.PW == PW
    rng = np.random.default_rng(100 * A + N)
    g = rng.standard_normal((SMAX, A, PW)).astype(np.float32)
    g[rng.random(g.shape) < 0.05] = -0.0
    geom = oracle.Geometry(N, N, True)
    Tinv = oracle.invert_transforms(oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW))
    want = oracle.rotate_bwd_tfcompat(g, geom, Tinv, oracle.NEAREST)
    k = np.random.default_rng(A).uniform(0.5, 2.0, SMAX).astype(np.float32)
    want_scaled = k[:, None, None] * want                                   # one float32 product per pixel, as the kernel's
    gd, kd = torch.from_numpy(g).to(d), torch.from_numpy(k).to(d)
    for S in BATCHES:
        aligned = gd[:S].clone()
        assert aligned.data_ptr() % 16 == 0
        for gs, where in ((aligned, "aligned"), (shifted(aligned), "shifted")):
            for scale, ref in ((None, want), (kd[:S], want_scaled)):
                outs = {}
                for tail in (0, 1):
                    out = torch.full((S, N, N), float("nan"), device=d)
                    with _lib.tuned("BWD_TAIL", tail):
                        plan.backward(gs, out=out, scale=scale)
                    torch.cuda.synchronize()
                    outs[tail] = out
                what = f"N={N} A={A} S={S} {where} scaled={scale is not None}"
                assert torch.equal(outs[1].view(torch.int32), outs[0].view(torch.int32)), what
                assert torch.equal(outs[1].cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(ref[:S])).view(torch.int32)), what


def test_headline_adjoint_equals_the_whole_vector_under_both_stores():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda", 0)
    B, N, A = 50, 128, 20
    plan = RotatePlan(np.pi * np.arange(A) / A, N, N, True, d)
    assert plan.backward_kernel_name(B) == "rotate_bwd_planned_kernel"
    g = torch.randn((B, A, plan.PW), device=d, generator=torch.Generator(device=d).manual_seed(17))
    for st in (1, 0):
        outs = {}
        for tail in (0, 1):
            out = torch.full((B, N, N), float("nan"), device=d)
            with _lib.tuned("WT_STORES", st), _lib.tuned("BWD_TAIL", tail):
                plan.backward(g, out=out)
            torch.cuda.synchronize()
            outs[tail] = out
        assert not torch.isnan(outs[1]).any()
        assert torch.equal(outs[1].view(torch.int32), outs[0].view(torch.int32)), f"WT_STORES={st}"


@pytest.mark.parametrize("B,A", ((40, 20), (80, 32)))
def test_eleven_wave_tiles_equal_the_sixteen_row_tiles(B, A):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda", 0)
    N = 128
    plan = planned(np.pi * np.arange(A) / A, N, d)
    g = torch.randn((B, A, plan.PW), device=d, generator=torch.Generator(device=d).manual_seed(B))
    outs = []
    for bw in (-1, 8):
        out = torch.full((B, N, N), float("nan"), device=d)
        with _lib.tuned("BW", bw):
            plan.backward(g, out=out)
        torch.cuda.synchronize()
        outs.append(out)
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
