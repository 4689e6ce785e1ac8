"""Reconstruction metrics on the device: (MSE, SSIM, PSNR) of a whole batch of image pairs in float64, the numbers dataset_io.compare
gives one pair at a time on the host (ctvae/helper_functions.py:394-418 with scikit-image 0.18's SSIM).  csrc/merit.hip states every
operation, the tiling and the one order of every sum: three launches whatever the batch is, the same bits on every run, and a pair's
numbers do not depend on the batch around it.

    m = image_merits(truth, recon)      truth, recon [n][X][Y] (or [X][Y]) -> float64 [n][3] on their device: m[k] = (mse, ssim, psnr)
                                        of recon[k] against truth[k]; the data range of the SSIM and the PSNR is truth[k]'s max - min

With mse == 0 the PSNR is +inf (scikit-image's rule; the host compare divides by zero there).  There is no CPU path and no autograd."""
import numpy as np
import torch

from . import _lib
from . import forward_functions as _fwd
from .forward_functions import _stream_ptr

__all__ = ["image_merits", "merit_tile"]


def merit_tile():
    """Edge of the tiles of window positions the SSIM launch cuts an image into (host only)."""
    return int(_lib.load().ctpvae_merit_tile())


def _shape_dtype(name, a):
    if not isinstance(a, (torch.Tensor, np.ndarray)):
        raise TypeError(f"image_merits: {name} must be a torch tensor or a numpy array (got {type(a).__name__})")
    dtype = a.dtype if isinstance(a, torch.Tensor) else {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}.get(a.dtype)
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"image_merits: {name} must be float32 or float64 (got {a.dtype})")
    return tuple(a.shape), dtype


def image_merits(ref, test):
    """float64 [n][3] = (mse, ssim, psnr) of test[k] against ref[k].  ref, test: [X][Y] or [n][X][Y], one shape, both float32 or both
    float64, tensors on one HIP device or numpy arrays (uploaded to the other operand's device, or to the current one).  Detached: no
    autograd.  Every check is made before anything is launched."""
    (rs, rd), (ts, td) = _shape_dtype("ref", ref), _shape_dtype("test", test)
    if rs != ts:
        raise ValueError(f"image_merits: ref and test must have one shape (got {rs}, {ts})")
    if rd != td:
        raise ValueError(f"image_merits: ref and test must have one dtype, float32 or float64 (got {rd}, {td})")
    if len(rs) not in (2, 3):
        raise ValueError(f"image_merits: images must be [X][Y] or [n][X][Y] (got {rs})")
    n, X, Y = (1,) + rs if len(rs) == 2 else rs
    if min(X, Y) < 3:
        raise ValueError(f"image_merits: images must be at least 3 x 3, the smallest SSIM window (got {X} x {Y})")
    if n * X * Y >= 2 ** 31:
        raise ValueError(f"image_merits: at most 2^31 - 1 pixels in one call (got {n} x {X} x {Y})")
    devs = [a.device for a in (ref, test) if isinstance(a, torch.Tensor)]
    if any(d.type != "cuda" for d in devs) or len(set(devs)) > 1:
        raise _lib.RadonLibraryError(f"image_merits: ref and test must be on one HIP device (got {', '.join(str(d) for d in devs)}); "
                                     "there is no CPU path")
    if not devs and not torch.cuda.is_available():
        raise _lib.RadonLibraryError("image_merits: no HIP device to upload the arrays to; there is no CPU path")
    dev = devs[0] if devs else torch.device("cuda", torch.cuda.current_device())

    def on_device(a):
        t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t.reshape(n, X, Y).contiguous()

    lib = _lib.load()
    ws_bytes = _lib.check(lib.ctpvae_merit_workspace_bytes(n, X, Y), "merit_workspace_bytes")
    with torch.cuda.device(dev):
        r, t = on_device(ref), on_device(test)
        out = _fwd._new_output((n, 3), torch.float64, dev)
        if n == 0:
            return out
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
        fn = lib.ctpvae_merit_f32 if rd is torch.float32 else lib.ctpvae_merit_f64
        _lib.check(fn(r.data_ptr(), t.data_ptr(), n, X, Y, ws.data_ptr(), out.data_ptr(), _stream_ptr()), "merit")
    return out
