"""One PixelMarginals(head="beta").add() (csrc/beta_marginals.hip: the Beta head's samples drawn, binned and summed in registers / LDS,
none stored) against what the same result costs without it: K calls of beta_head, the K outputs stacked, and torch operations that bin
the stack with the same float32 rule and sum it and its squares in float64.

    python tools/time_beta_marginals.py [--out profiles/beta_marginals_timing.txt]

Shapes: the toy (n = 8 objects of 2 x 2, K = 100 draws) and foam (n = 20 objects of 128 x 128, K = 100: 33 M samples per call).  Both
paths get the same alpha / beta (raw operands of the trainer's range, -1 .. 2: concentrations on both sides of the boost's seam at 1)
and fill a state of the same layout; the first window ASSERTS that the two histograms are equal.
"ms" is the median (min .. max) of 3 windows after a warm-up window, from a host clock around work that ends in a device synchronise;
"gpu ms" is the same windows from HIP events.  The two paths alternate window by window.  A ratio is reported with the span its windows
allow (slowest / fastest and fastest / slowest); when the two paths' windows overlap the line says so.  The last rows give the peak
device memory torch's allocator reports for one call of each path at the foam shape, above what alpha, beta and the state occupy."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ct_pvae_amd as cp  # noqa: E402
from time_marginals import GRID, SHAPES, window  # noqa: E402  (the same grid, shapes and windows as the TruncatedNormal tool's)


def stacked_baseline(alpha, beta, K, hist, s1, s2):
    """The parent's means: K head launches, one stack, the bin rule and the sums in torch."""
    n, pix, cols = alpha.shape[0], alpha.shape[2] * alpha.shape[3], GRID["bins"] + 2
    x = torch.stack([cp.beta_head(alpha, beta, seed=1, draw=k)[0].view(n, pix) for k in range(K)]).view(K * n, pix)
    lo, width = (torch.full((1,), GRID[k], dtype=torch.float32, device=x.device) for k in ("lo", "width"))
    t = (x - lo) / width                        # tensor operands: a true division, as the kernel's (a scalar divisor is multiplied by 1 / b)
    col = torch.where(t >= GRID["bins"], torch.full_like(t, GRID["bins"] + 1), 1 + torch.floor(t))
    col = torch.where(t >= 0, col, torch.zeros_like(t)).to(torch.int64)
    flat = col + torch.arange(pix, device=x.device, dtype=torch.int64)[None, :] * cols
    hist += torch.bincount(flat.view(-1), minlength=pix * cols).view(pix, cols)
    xd = x.double()
    s1 += xd.sum(dim=0)
    s2 += (xd * xd).sum(dim=0)


def shape_rows(dev, name, windows=3):
    n, X, Y, K, calls = SHAPES[name]
    g = torch.Generator(device=dev).manual_seed(n)
    alpha = torch.rand((n, 1, X, Y), device=dev, generator=g) * 3 - 1
    beta = torch.rand((n, 1, X, Y), device=dev, generator=g) * 3 - 1
    m = cp.PixelMarginals((X, Y), device=dev, head="beta", **GRID)
    hist, s1, s2 = torch.zeros_like(m.hist), torch.zeros_like(m.s1), torch.zeros_like(m.s2)
    fns = {"head x K + torch": lambda: stacked_baseline(alpha, beta, K, hist, s1, s2),
           "one add()": lambda: m.add(alpha, beta, draws=K, seed=1)}
    for f in fns.values():
        window(f, calls)
    same = bool(torch.equal(hist, m.hist))
    assert same, f"{name}: the histograms of the two paths differ after the warm-up window"
    res = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            res[k].append(window(f, calls))
    rows = []
    for k, v in res.items():
        host, gpu = np.array(v).T
        rows.append(f"{name:5s} n={n:<3d} {X}x{Y} K={K}  {k:17s} {np.median(host):9.4f} ({host.min():.4f} .. {host.max():.4f})   "
                    f"{np.median(gpu):9.4f} ({gpu.min():.4f} .. {gpu.max():.4f})")
    for col, clock in ((0, "host clock"), (1, "HIP events")):
        base, new = np.array(res["head x K + torch"])[:, col], np.array(res["one add()"])[:, col]
        overlap = "; the windows OVERLAP" if new.max() >= base.min() and base.max() >= new.min() else ""
        if new.min() > base.max():
            overlap = "; add() LOSES at this shape"
        rows.append(f"#   {name}: baseline / add() = {np.median(base) / np.median(new):.2f}x {clock} "
                    f"(span {base.min() / new.max():.2f}x .. {base.max() / new.min():.2f}x){overlap}")
    rows.append(f"#   {name}: histograms of the two paths after the warm-up window equal: {same}")
    return rows, (alpha, beta, K, m, hist, s1, s2)


def memory_rows(dev, alpha, beta, K, m, hist, s1, s2):
    rows = []
    for k, f in (("head x K + torch", lambda: stacked_baseline(alpha, beta, K, hist, s1, s2)), ("one add()", lambda: m.add(alpha, beta, draws=K, seed=1))):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        f()
        torch.cuda.synchronize()
        rows.append(f"foam peak device memory above the operands and the state, {k:17s} {(torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20:10.2f} MiB")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "beta_marginals_timing.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_beta_marginals.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# tools/time_beta_marginals.py on {torch.cuda.get_device_name(0)} ({arch}); median (min .. max) over 3 alternating windows",
             "# what                                        ms per call, host clock + synchronise     gpu ms per call, HIP events"]
    for name in SHAPES:
        rows, state = shape_rows(dev, name)
        lines += rows
    lines += memory_rows(dev, *state)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
