"""The checks every fused operator makes before it looks at a device: of a float32 tensor argument, and of the counter words (seed,
draw, first_object) of the operators that draw random numbers."""
import torch


def check_float32(what, name, t, dim, layout, shape_ok=None):
    """Refuse, in this order: a non-tensor and a dtype other than float32 (TypeError); a rank other than `dim`, an empty tensor or a
    shape that `shape_ok(t.shape)` turns down, as "`what`: `name` must be `layout`"; a non-contiguous tensor (ValueError)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch tensor (got {type(t).__name__})")
    if t.dtype is not torch.float32:
        raise TypeError(f"{what}: {name} must be float32 (got {t.dtype})")
    if t.dim() != dim or t.numel() == 0 or (shape_ok is not None and not shape_ok(t.shape)):
        raise ValueError(f"{what}: {name} must be {layout} (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous (got strides {tuple(t.stride())})")


def counter_args(seed, draw, first_object):
    """(seed, draw, first_object) as the library takes them: the seed's low 64 bits, one 32-bit draw word, a non-negative offset."""
    seed, draw, first_object = int(seed), int(draw), int(first_object)
    if not 0 <= draw < 2 ** 32:
        raise ValueError(f"draw is one 32-bit counter word: 0 <= draw < 2^32 (got {draw})")
    if not 0 <= first_object < 2 ** 63:
        raise ValueError(f"first_object must be >= 0 (got {first_object})")
    return seed & (2 ** 64 - 1), draw, first_object
