"""What the wrappers of the two fused ConvBlock convolutions share (conv.py: `what` "periodic_conv_maxout", symbol prefix "conv";
conv_transpose.py: "conv_transpose_maxout", "convt"): the checks of x, weight, bias and the integers, and the two launches whose
arguments differ only in the geometry's integers.  Every C symbol is fetched from _lib.load() by name when it is called."""
import torch

from . import _lib, forward_functions
from ._args import check_float32
from .forward_functions import _stream_ptr


def check_tensors(what, x, weight, bias):
    for name, t, dim in (("x", x, 4), ("weight", weight, 4), ("bias", bias, 1)):
        check_float32(what, name, t, dim, f"a non-empty tensor of {dim} axes")


def check_ints(what, **values):
    for name, v in values.items():
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{what}: {name} must be a Python int (got {type(v).__name__})")


def check_kernel_and_stride(what, k, stride):
    if not 1 <= k <= 8:
        raise ValueError(f"{what}: the kernel size must be in 1 .. 8 (got {k})")
    if not 1 <= stride <= k:
        raise ValueError(f"{what}: the stride must be in 1 .. k = {k} (got {stride})")


def require_cuda(what, x, weight, bias):
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if t.device.type != "cuda":
            raise _lib.RadonLibraryError(f"{what}: {name} must be a CUDA tensor; there is no CPU path")
        if t.device != x.device:
            raise ValueError(f"{what}: {name} is on {t.device}, x on {x.device}")


def forward(prefix, x, weight, bias, geom, hw):
    """(out, first) of ctpvae_<prefix>_fwd_f32; geom starts (N, Cin, H, W, C, ..), hw is the output's (OH, OW)."""
    N, C = geom[0], geom[4]
    out = forward_functions._new_output((N, C) + hw, torch.float32, x.device)
    first = torch.empty((N, C) + hw, dtype=torch.uint8, device=x.device)     # (saved state, every byte written by the launch)
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.load(), f"ctpvae_{prefix}_fwd_f32")(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), *geom, out.data_ptr(),
                                                                    first.data_ptr(), _stream_ptr()), f"{prefix}_fwd")
    return out, first


def weight_grad(prefix, x, g, first, weight, geom):
    """(gw, gb) of ctpvae_<prefix>_bwd_weight_f32, with the workspace ctpvae_<prefix>_wgrad_workspace_bytes asks for."""
    lib = _lib.load()
    with torch.cuda.device(g.device):
        ws = torch.empty(_lib.check(getattr(lib, f"ctpvae_{prefix}_wgrad_workspace_bytes")(*geom), f"{prefix}_wgrad_workspace_bytes") // 4,
                         dtype=torch.float32, device=g.device)
        gw = forward_functions._new_output(tuple(weight.shape), torch.float32, g.device)
        gb = forward_functions._new_output((2 * geom[4],), torch.float32, g.device)
        _lib.check(getattr(lib, f"ctpvae_{prefix}_bwd_weight_f32")(x.data_ptr(), g.data_ptr(), first.data_ptr(), *geom, ws.data_ptr(),
                                                                   gw.data_ptr(), gb.data_ptr(), _stream_ptr()), f"{prefix}_bwd_weight")
    return gw, gb
