"""One image_merits call (csrc/merit.hip: MSE / SSIM / PSNR of a whole batch in float64, three launches) against what the same numbers
cost without it:
  (a) the host loop: the reconstructions copied back to the host, then dataset_io.compare pair by pair (numpy + five
      scipy.ndimage.uniform_filter passes each) -- what evaluate_sinogram and bin/final_merit.py do;
  (b) a torch chain on the device: the images widened to float64, five avg_pool2d passes (7 x 7, stride 1, no padding: exactly the
      window positions scikit-image keeps) and elementwise operations, the means with torch's own reductions.

    python tools/time_merit.py [--out profiles/merit_timing.txt]

Shapes: final_merit's call for the paper's foam run (3 x 1000 pairs of 128 x 128 float32) and 3 x 32 pairs of 512 x 512 float32.  Every
path gets the same two-level images plus noise, already on the device.  "ms" is the median (min .. max) of 3 windows after a warm-up
window, from a host clock around work that ends in a device synchronise; "gpu ms" is the same windows between two HIP events (for the
host loop the events bracket the host's work too, so that column repeats the wall time and no ratio is formed from it).  The paths
alternate window by window.  A ratio is reported with the span its windows allow; when two paths' windows overlap the line says so.
The next rows give the worst relative distance of the device's numbers from compare's, and of the torch chain's, over all pairs of
both shapes.  The last rows are the accuracy record of the test suite's own cases (tests/np_twin_merit.GPU_SHAPES, float32 and float64,
17 pairs each, the inputs of tests/test_gpu_merit.py): the worst distance of image_merits from compare and from the float64 twin."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from ct_pvae_amd import dataset_io  # noqa: E402
from tests import np_twin_merit as tm  # noqa: E402

SHAPES = {"foam": (1000, 128, 128), "large": (32, 512, 512)}     # examples, X, Y
CALLS = {"host loop of compare": 1, "torch float64 chain": 5, "one image_merits": 50}     # calls per window
WIN = 7


def images(n, X, Y, seed):
    """truth [n][X][Y] and three 'reconstructions' [3 n][X][Y], float32 in [0, 1]: two-level cells plus noise of three strengths."""
    rng = np.random.default_rng(seed)
    cells = (rng.random((n, X // 8 + 1, Y // 8 + 1)) < 0.4).astype(np.float32)
    truth = 0.15 + 0.6 * np.repeat(np.repeat(cells, 8, axis=1), 8, axis=2)[:, :X, :Y]
    truth[:, 0, 0] = 0.0                                              # every image's minimum: max|r| <= 2 R
    test = np.concatenate([np.clip(truth + s * rng.standard_normal(truth.shape, dtype=np.float32), 0, 1) for s in (0.05, 0.15, 0.02)])
    return truth, test.astype(np.float32)


def host_loop(ref, test):
    r, t = ref.cpu().numpy(), test.cpu().numpy()
    return np.array([dataset_io.compare(r[k], t[k], verbose=False) for k in range(len(r))])


def torch_chain(ref, test):
    r, t = ref.double()[:, None], test.double()[:, None]
    mse = ((r - t) ** 2).mean(dim=(1, 2, 3))
    R = r.amax(dim=(1, 2, 3)) - r.amin(dim=(1, 2, 3))
    NP = WIN * WIN
    cov_norm = NP / (NP - 1)
    ux, uy = F.avg_pool2d(r, WIN, 1), F.avg_pool2d(t, WIN, 1)
    uxx, uyy, uxy = F.avg_pool2d(r * r, WIN, 1), F.avg_pool2d(t * t, WIN, 1), F.avg_pool2d(r * t, WIN, 1)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = ((0.01 * R) ** 2)[:, None, None, None], ((0.03 * R) ** 2)[:, None, None, None]
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return torch.stack([mse, s.mean(dim=(1, 2, 3)), 10 * torch.log10(R * R / mse)], dim=1)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls, a.elapsed_time(b) / calls


def shape_rows(dev, name, windows=3):
    n, X, Y = SHAPES[name]
    truth, test = images(n, X, Y, seed=n)
    ref = torch.from_numpy(np.concatenate([truth] * 3)).to(dev)
    test = torch.from_numpy(test).to(dev)
    fns = {"host loop of compare": (lambda: host_loop(ref, test), CALLS["host loop of compare"]),
           "torch float64 chain": (lambda: torch_chain(ref, test), CALLS["torch float64 chain"]),
           "one image_merits": (lambda: cp.image_merits(ref, test), CALLS["one image_merits"])}
    for f, c in fns.values():
        window(f, c)
    res = {k: [] for k in fns}
    for _ in range(windows):
        for k, (f, c) in fns.items():
            res[k].append(window(f, c))
    rows = []
    for k, v in res.items():
        host, gpu = np.array(v).T
        rows.append(f"{name:5s} 3x{n} pairs {X}x{Y} f32  {k:21s} {np.median(host):11.4f} ({host.min():.4f} .. {host.max():.4f})   "
                    f"{np.median(gpu):11.4f} ({gpu.min():.4f} .. {gpu.max():.4f})")
    for base_name in ("host loop of compare", "torch float64 chain"):
        for col, clock in ((0, "host clock"), (1, "HIP events")):
            if base_name.startswith("host") and col == 1:
                continue                                             # the host loop's work is not on the device
            base, new = np.array(res[base_name])[:, col], np.array(res["one image_merits"])[:, col]
            overlap = "; the windows OVERLAP" if new.max() >= base.min() else ""
            rows.append(f"#   {name}: {base_name} / image_merits = {np.median(base) / np.median(new):.2f}x {clock} "
                        f"(span {base.min() / new.max():.2f}x .. {base.max() / new.min():.2f}x){overlap}")
    want = host_loop(ref, test)
    dist = {k: float(np.max(np.abs(f().cpu().numpy() - want) / np.abs(want))) for k, (f, _) in list(fns.items())[1:]}
    return rows, dist


def accuracy_rows(dev):
    """The cases of tests/test_gpu_merit.py::test_against_twin_and_compare, measured (no bar is applied here: the tests hold them)."""
    worst_c, where, worst_t, worst_p = 0.0, "", 0.0, 0.0
    for shape in tm.GPU_SHAPES:
        for dtype_name in ("float32", "float64"):
            r, t = tm.gpu_case_inputs(shape, dtype_name)
            got = cp.image_merits(torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
            comp = np.array([dataset_io.compare(r[k], t[k], verbose=False) for k in range(len(r))])
            twin = tm.batch(r, t)
            c = float(np.max(np.abs(got - comp) / np.abs(comp)))
            if c > worst_c:
                worst_c, where = c, f"{shape[0]} x {shape[1]} {dtype_name}"
            worst_t = max(worst_t, float(np.max(np.abs(got[:, :2] - twin[:, :2]) / np.abs(twin[:, :2]))))
            worst_p = max(worst_p, float(np.max(np.abs(got[:, 2] - twin[:, 2]) / np.abs(twin[:, 2]))))
    cases = 2 * len(tm.GPU_SHAPES)
    return [f"# the test suite's cases ({cases} cases of {tm.GPU_N} pairs each, {tm.GPU_SHAPES[0][0]} x {tm.GPU_SHAPES[0][1]} to 512 x 96, float32 and float64):",
            f"worst relative distance from dataset_io.compare, the tests' cases, one image_merits      {worst_c:.3e}   ({where})",
            f"worst relative distance from the float64 twin (tests/np_twin_merit.py): MSE, SSIM        {worst_t:.3e}   (0 = the same bits)",
            f"worst relative distance from the float64 twin: PSNR (ends in log10)                      {worst_p:.3e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "merit_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_merit.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_merit.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over 3 alternating windows",
             "# what                                                       ms per call, host clock + synchronise        gpu ms per call, HIP events"]
    worst = {}
    for name in SHAPES:
        rows, dist = shape_rows(dev, name)
        lines += rows
        for k, v in dist.items():
            worst[k] = max(worst.get(k, 0.0), v)
            lines.append(f"#   {name}: worst |{k} - compare| / |compare| over the {3 * SHAPES[name][0]} pairs: {v:.3e}")
    for k, v in worst.items():
        lines.append(f"worst relative distance from dataset_io.compare, both shapes, {k:21s} {v:.3e}")
    lines += accuracy_rows(dev)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
