"""The planned u16 forward's FEW form (rotate_fwd_planned_kernel_few: dense one-part launches whose unit stages lean) against the CPU
oracle and against the general kernel (knob FWD_FEW=0), bit for bit, and the CHOICE of the form (RotatePlan.forward_form) per geometry.

Geometries: 128 x 128 padded (184 bins, 3 bin blocks), 64 x 64 padded and unpadded (one bin block), 64 x 128 and 128 x 64 unpadded
take the few form; 100 x 100 (no power-of-two unit) and 128 x 128 with the image one float off a 16-byte boundary keep the general one.
Angle sets: 1 / 2 / 3 / 20 / 32 angles over both mirror classes, and eight angles of ONE class -- there, and at one angle, the other
class's workgroups have no task: they pass the barrier and store nothing.  Batches 1 / 2 / 3 / 5 / 50 (singles, a half-empty last
pair), at the library's own launch shape and with slices per unit (NS) and task groups (G) forced: G = 1 at 32 angles is 48 tasks
on 16 waves (tasks taken from the LDS counter behind a wave's first), G = 12 at few angles is workgroups without any."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import RotatePlan

pytestmark = pytest.mark.gpu

GEOMS = {   # name: (H, W, pad, float offset of the image tensor, takes the few form)
    "128x128": (128, 128, True, 0, True),
    "64x64_padded": (64, 64, True, 0, True),
    "64x64": (64, 64, False, 0, True),
    "64x128": (64, 128, False, 0, True),
    "128x64": (128, 64, False, 0, True),
    "100x100_padded": (100, 100, True, 0, False),
    "128x128_offset_one_float": (128, 128, True, 1, False),
}
ANGLES = ["1", "2", "3", "20", "32", "one_class"]
BATCHES = (1, 2, 3, 5, 50)


def thetas(rng, which):
    if which == "one_class":
        return rng.uniform(0.1, 1.4, 8)     # cos > 0 > -sin: column and row always move opposite ways
    return rng.uniform(-1.0, 4.0, int(which))


@pytest.mark.parametrize("name", list(GEOMS))
@pytest.mark.parametrize("angles", ANGLES)
def test_few_form_equals_oracle_and_general_kernel(oracle, name, angles):
    H, W, pad, off, few = GEOMS[name]
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * ANGLES.index(angles) + H + 3 * W + off)
    theta = thetas(rng, angles)
    A = len(theta)
    plan = RotatePlan(theta, H, W, pad, d, plan_format="u16")
    T = oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW)
    same_way = (T[:, 0] >= 0) == (T[:, 3] >= 0)
    if angles == "one_class":
        assert same_way.all() or not same_way.any()
    if angles in ("20", "32"):
        assert same_way.any() and not same_way.all()
    Smax = max(BATCHES)
    x_np = rng.standard_normal((Smax, H, W)).astype(np.float32)
    buf = torch.zeros(Smax * H * W + 4, dtype=torch.float32, device=d)   # (a fresh allocation is 16-byte aligned)
    buf[off: off + Smax * H * W].copy_(torch.from_numpy(x_np).reshape(-1))
    want_all = torch.from_numpy(oracle.rotate_fwd(x_np, oracle.Geometry(H, W, pad), T, 0))   # once: a batch is its first S slices
    shapes = [()] + [(("NS", ns), ("G", G)) for ns in (1, 2) for G in (1, 5, 12)]
    for S in BATCHES:
        x = buf[off: off + S * H * W].view(S, H, W)
        assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (off == 0)
        want = want_all[:S]
        for knobs in shapes:
            for kname, v in knobs:
                _lib.tune(kname, v)
            assert plan.forward_form(S, x) == (1 if few else 0), (name, angles, S, knobs)
            got = plan.forward(x)
            with _lib.tuned("FWD_FEW", 0):
                assert plan.forward_form(S, x) == 0
                general = plan.forward(x)
            _lib.tune("*")
            assert torch.equal(got.cpu(), want), (name, angles, S, knobs, "oracle")
            assert torch.equal(got, general), (name, angles, S, knobs, "general kernel")


def test_few_form_replays_in_a_captured_graph(oracle):
    d = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    theta = rng.uniform(-1.0, 4.0, 20)
    plan = RotatePlan(theta, 128, 128, True, d, plan_format="u16")
    xs = [torch.from_numpy(rng.standard_normal((S, 128, 128)).astype(np.float32)).to(d) for S in (50, 5, 1)]
    outs = [torch.full((x.shape[0], 20, plan.PW), float("nan"), device=d) for x in xs]
    eager = []
    for x in xs:
        assert plan.forward_form(x.shape[0], x) == 1
        eager.append(plan.forward(x))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for x, out in zip(xs, outs):
            plan.forward(x, out=out)
    for _ in range(2):
        for out in outs:
            out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for out, e in zip(outs, eager):
            assert torch.equal(out, e)
    geom = oracle.Geometry(128, 128, True)
    T = oracle.rotate_transforms(np.asarray(theta, dtype=np.float32), plan.PH, plan.PW)
    assert torch.equal(outs[1].cpu(), torch.from_numpy(oracle.rotate_fwd(xs[1].cpu().numpy(), geom, T, 0)))
