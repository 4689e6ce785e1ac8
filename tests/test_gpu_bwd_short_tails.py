"""The few-angle (SHORT) planned adjoint at every tail: a launch of A <= 32 angles runs the straight-line code of its na4 / 4 index
dwords -- a full vector of sixteen taps when A > 16, then a tail of 1 .. 4 dwords -- and every one of them equals the CPU oracle's
rotate_bwd_tfcompat (NEAREST) bit for bit, under plain and write-through stores, into NaN-filled outputs.

Angle counts  1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32: every tail of 1 .. 4 dwords, alone and behind a full group, with
              and without dead bytes in the last dword; angles random in (-1, 4) rad, seeded.
Shapes        40 x 36 (56 bins): a ragged column block, a last tile shorter than the tile height; one column of tiles taller than 32
              rows runs single slices (PPT = 4) at every batch size;
              24 x 72 (78 bins): two column blocks, the second ragged; pairs of slices (PPT = 2); 78 % 4 != 0: the general stager;
              32 x 32 (48 bins): pairs whose rows go through stage_contig_rows (48 % 4 == 0, as 56).
Batch sizes   1, 2, 3 (a single slice, a pair, a half-empty pair) and 18 (eight-wave tiles: the 1024-thread instantiations of the pair
              shapes), each with and without a per-slice scale.
Cotangents    standard normal with a sprinkling of -0.0f; one more case with a single +inf bin.  (No -inf and no NaN goes in: a NaN's
              payload may differ between host and device.)
The oracle's gradient is computed once per (shape, A) for the eighteen slices; the smaller batches are its first slices."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan, num_proj_pix

pytestmark = pytest.mark.gpu

ANGLES = (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32)
SHAPES = ((40, 36), (24, 72), (32, 32))
BATCHES = (1, 2, 3, 18)
SMAX = max(BATCHES)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def cotangents(rng, A, PW):
    g = rng.standard_normal((SMAX, A, PW)).astype(np.float32)
    g[rng.random(g.shape) < 0.05] = -0.0
    return g


def check(oracle, H, W, A, g, batches):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda", 0)
    theta = np.random.default_rng(1000 * H + A).uniform(-1.0, 4.0, A)
    plan = RotatePlan(theta, H, W, True, d, plan_format="u16")
    assert plan.PW == g.shape[2]
    geom = oracle.Geometry(H, W, True)
    Tinv = oracle.invert_transforms(oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW))
    want = oracle.rotate_bwd_tfcompat(g, geom, Tinv, oracle.NEAREST)
    k = np.random.default_rng(A).uniform(0.5, 2.0, SMAX).astype(np.float32)
    want_scaled = k[:, None, None] * want                                   # one float32 product per pixel, as the kernel's
    gd, kd = torch.from_numpy(g).to(d), torch.from_numpy(k).to(d)
    for S in batches:
        assert plan.backward_kernel_name(S) == "rotate_bwd_planned_kernel"
        for scale, ref in ((None, want), (kd[:S], want_scaled)):
            for st in (0, 1):
                out = torch.full((S, H, W), float("nan"), device=d)
                with _lib.tuned("WT_STORES", st):
                    plan.backward(gd[:S], out=out, scale=scale)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(ref[:S]), err_msg=f"S={S} scaled={scale is not None} WT_STORES={st}")


def test_the_shapes_reach_both_stagers():
    assert {num_proj_pix(H, W) % 4 == 0 for H, W in SHAPES} == {True, False}


@pytest.mark.parametrize("A", ANGLES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_short_adjoint_equals_the_oracle_bit_for_bit_at_every_tail(oracle, H, W, A):
    g = cotangents(np.random.default_rng(100 * A + H), A, num_proj_pix(H, W))
    assert (bits(g) == np.int32(-2 ** 31)).any()                           # there are -0.0f among the cotangents
    check(oracle, H, W, A, g, BATCHES)


@pytest.mark.parametrize("A", (5, 20))
def test_a_single_infinite_bin_reaches_exactly_the_pixels_that_gather_it(oracle, A):
    H, W = 24, 72
    g = cotangents(np.random.default_rng(7 + A), A, num_proj_pix(H, W))
    g[:, A - 1, num_proj_pix(H, W) // 2] = np.inf                           # the central bin of the last angle: inside every tail
    check(oracle, H, W, A, g, (3, 18))
