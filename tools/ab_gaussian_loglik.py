"""Developer tool: the Gaussian likelihood training calls timed with ONE build of the package per process, to be run in alternation
with another checkout's build on one box (tools/ab_compare.py's method; that tool swaps the library under this tree's binding,
which cannot load a library older than the binding's symbol table -- this one imports the whole other package instead).

    python tools/ab_gaussian_loglik.py                        (this tree)
    CTPVAE_TREE=/path/to/other/checkout python tools/ab_gaussian_loglik.py     (a built checkout of another commit)

Timed, each as a HIP-graph replay of N calls between two events after three untimed replays, median of 5 (and min / max):
  rotate   the headline training call: S = 10 slices of 128 x 128, 20 of 180 angles as a host index operand, fused likelihood +
           per-object sums (RotatePlan.forward_loglik_sums), and its scaled adjoint
  siddon   calculate_log_prob_M_given_R(model="siddon", reduce="per_object") + the reconstruction gradient, B = 10 and B = 50,
           20 of 180 angles
Only default (Gaussian) arguments are passed, so both sides of a comparison run the same script.

The C++ autograd node is stubbed out at import on BOTH sides (_lib.torch_node returns None): none of the timed calls goes through it
(the rotate call is timed at the RotatePlan entry points, the siddon call never uses the node), and a checkout given through
CTPVAE_TREE need not have built it.  What is timed is the library's launches under HIP-graph replay, not the node."""
import os
import sys

import numpy as np
import torch

TREE = os.path.abspath(os.environ.get("CTPVAE_TREE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, TREE)
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import _lib, phantoms  # noqa: E402
from ct_pvae_amd.forward_functions import RotatePlan  # noqa: E402

assert os.path.abspath(cp.__file__).startswith(TREE + os.sep), (cp.__file__, TREE)
_lib.torch_node = lambda: None      # the C++ autograd node is not on these paths: neither side builds or loads it
d = torch.device("cuda", 0)


def timed(body, n):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            body()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / n)
    return f"{np.median(t):8.2f} us (min {min(t):.2f}, max {max(t):.2f})"


print("tree:", TREE, "library:", _lib.LIB_PATH, flush=True)
theta = np.ascontiguousarray(phantoms.dense_theta(180), dtype=np.float32)
sub = np.random.default_rng(0).permutation(180)[:20].astype(np.int32)
pnm = torch.tensor(1e4, device=d)

S = 10
dense = RotatePlan(theta, 128, 128, True, d)
x = torch.rand((S, 128, 128), device=d)
mask, meas = torch.full((S, 180), 0.05, device=d), torch.rand((S, 180, 184), device=d)
hsub = torch.from_numpy(sub)
w = torch.ones(S, device=d)
dlp = dense.forward_loglik_sums(x, mask, meas, pnm, 1e-7, angles_i=hsub, dense_inputs=True)[1]
gx = torch.empty_like(x)
print("rotate S=10 20/180 fwd+likelihood+sums:", timed(lambda: dense.forward_loglik_sums(x, mask, meas, pnm, 1e-7, angles_i=hsub, dense_inputs=True), 100),
      flush=True)
print("rotate S=10 20/180 scaled adjoint:     ", timed(lambda: dense.backward(dlp, out=gx, scale=w, angles_i=hsub), 100), flush=True)

for B in (10, 50):
    rng = np.random.default_rng(B)
    xs = torch.from_numpy(phantoms.foam_batch(B, 128, seed=1, supersample=2)[..., None]).to(d).requires_grad_(True)
    mk = torch.from_numpy(rng.uniform(0.02, 0.08, (B, 180)).astype(np.float32)).to(d)
    ms = torch.rand((B, 180, 184), device=d) * 3.0
    wt = torch.linspace(0.5, 2.0, B, device=d)

    def call():
        with torch.autograd.set_multithreading_enabled(False):
            s = cp.calculate_log_prob_M_given_R(xs, mk, ms, pnm, 1.2e-7, theta=theta, angles_i=sub, pad=True, model="siddon",
                                                reduce="per_object")
            return torch.autograd.grad(s, xs, wt)[0]
    print(f"siddon B={B:2d} 20/180 fwd+likelihood+sums+bwd:", timed(call, 20), flush=True)
