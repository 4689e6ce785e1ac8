"""The update stage of a P-VAE training step -- the reference's NaN filter, per-tensor clip_by_norm and Keras Adam
(ctvae/main_ct_vae.py:353, :482-485) -- as two launches over the flat gradient buffer (csrc/update.hip states every operation, the
order of the float64 sum of squares and the two deviations from TensorFlow).

    FusedUpdate(params, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, clip_norm=100.0)
        .step(flat_grad)            one update of `params` from the FlatGradBucket.flat of exactly these tensors; flat_grad is read only
        .norms                      float32 [T] on the device: the l2 norms (NaNs counted as 0) of the last step's gradients
        .t                          steps taken
        .state_dict() / .load_state_dict()     torch.optim.Adam's layout: per parameter step / exp_avg / exp_avg_sq, plus param_groups
    adam_alpha(t, lr, beta1, beta2) the step's float32 alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t), evaluated in float64
    chunk_len(), chunk_table(lens, addresses)          the host-built chunk table (needs no GPU)

Epsilon stands OUTSIDE the bias correction, as in Keras (p -= alpha * m / (sqrt(v) + eps)); torch.optim.Adam puts it inside.  The three
stored quantities are the same under both, so a state dictionary moves between them.  Building the object and its state dictionary work
on CPU tensors; step() has no CPU path."""
import math

import numpy as np
import torch

from . import _lib
from .forward_functions import _stream_ptr

__all__ = ["FusedUpdate", "adam_alpha", "chunk_len", "chunk_table"]

CHUNK_DTYPE = np.dtype([("off", "<i8"), ("param", "<u8"), ("len", "<i4"), ("tensor", "<i4"), ("first", "<i4"), ("count", "<i4")])


def chunk_len():
    """C: no chunk of the table is longer."""
    return int(_lib.load().ctpvae_update_chunk_len())


def chunk_table(lens, addresses):
    """The chunk table of tensors of `lens` elements at the device `addresses`, as a numpy record array (CHUNK_DTYPE, one 32-byte record
    per chunk): tensor after tensor, ascending in offset, no chunk across a tensor boundary or longer than chunk_len()."""
    lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
    addresses = np.ascontiguousarray(addresses, dtype=np.uint64).reshape(-1)
    if lens.size != addresses.size:
        raise ValueError(f"chunk_table: {lens.size} lengths for {addresses.size} addresses")
    lib = _lib.load()
    nbytes = _lib.check(lib.ctpvae_update_plan_bytes(lens.ctypes.data if lens.size else None, int(lens.size)), "update_plan_bytes")
    table = np.zeros(nbytes // CHUNK_DTYPE.itemsize, dtype=CHUNK_DTYPE)
    _lib.check(lib.ctpvae_update_plan_host(lens.ctypes.data, addresses.ctypes.data, int(lens.size), table.ctypes.data), "update_plan_host")
    return table


def adam_alpha(t, lr, beta1, beta2):
    """float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t)) of step t >= 1, every operation in float64 (TensorFlow evaluates it in float32)."""
    t = int(t)
    if t < 1:
        raise ValueError(f"adam_alpha: the step count starts at 1 (got {t})")
    return float(np.float32(float(lr) * math.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t)))


def _check_params(params):
    for k, p in enumerate(params):
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"FusedUpdate: parameter {k} must be a torch tensor (got {type(p).__name__})")
        if p.dtype is not torch.float32:
            raise TypeError(f"FusedUpdate: parameter {k} must be float32 (got {p.dtype})")
        if p.numel() == 0 or not p.is_contiguous():
            raise ValueError(f"FusedUpdate: parameter {k} must be contiguous and hold at least one element (shape {tuple(p.shape)})")


class FusedUpdate:
    def __init__(self, params, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, clip_norm=100.0):
        self.params = list(params)
        if not self.params:
            raise ValueError("FusedUpdate needs at least one parameter")
        _check_params(self.params)
        self.device = self.params[0].device
        if any(p.device != self.device for p in self.params):
            raise ValueError("FusedUpdate: all parameters must be on one device")
        self._set_hyper(lr, beta1, beta2, eps)
        self.clip_norm = float(clip_norm)
        if not (math.isfinite(self.clip_norm) and self.clip_norm > 0.0):
            raise ValueError(f"FusedUpdate: clip_norm must be positive and finite (got {clip_norm})")
        self.numels = [p.numel() for p in self.params]
        self.total = sum(self.numels)
        self.m = torch.zeros(self.total, dtype=torch.float32, device=self.device)       # exp_avg, in the bucket's layout
        self.v = torch.zeros(self.total, dtype=torch.float32, device=self.device)       # exp_avg_sq
        self.norms = torch.zeros(len(self.params), dtype=torch.float32, device=self.device)
        self.t = 0
        self._ptrs = self._plan = self._plan_host = self._partials = None

    def _set_hyper(self, lr, beta1, beta2, eps):
        lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError(f"FusedUpdate: lr must be finite and >= 0 (got {lr})")
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0) or float(np.float32(beta1)) >= 1.0 or float(np.float32(beta2)) >= 1.0:
            raise ValueError(f"FusedUpdate: needs 0 <= beta1, beta2 < 1, in float32 too (got {beta1}, {beta2})")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"FusedUpdate: eps must be finite and >= 0 (got {eps})")
        self.lr, self.beta1, self.beta2, self.eps = lr, beta1, beta2, eps

    def same_params(self, params):
        """Whether `params` are exactly this object's tensors, in order."""
        params = list(params)
        return len(params) == len(self.params) and all(a is b for a, b in zip(params, self.params))

    # -- the step ----------------------------------------------------------------------------------------------
    def _build_plan(self, ptrs):
        table = chunk_table(self.numels, ptrs)
        host = torch.from_numpy(table.view(np.uint8).reshape(-1))
        if self.device.type == "cuda":
            host = host.pin_memory()            # (kept: the copy below does not wait for the host)
        self._plan_host = host
        self._plan = host.to(self.device, non_blocking=True)
        self._partials = torch.empty(table.size, dtype=torch.float64, device=self.device)
        self._ptrs = ptrs

    def step(self, flat_grad):
        """One update from flat_grad, the float32 [total] FlatGradBucket.flat of exactly these parameters, on their device.  Two launches
        on the current stream, no synchronisation; flat_grad is left as it is.  A parameter whose memory moved since the last step is
        picked up (the chunk table is rebuilt)."""
        if not isinstance(flat_grad, torch.Tensor):
            raise TypeError(f"FusedUpdate.step: flat_grad must be a torch tensor (got {type(flat_grad).__name__})")
        if flat_grad.dtype is not torch.float32:
            raise ValueError(f"FusedUpdate.step: flat_grad must be float32 (got {flat_grad.dtype})")
        if flat_grad.dim() != 1 or flat_grad.numel() != self.total or not flat_grad.is_contiguous():
            raise ValueError(f"FusedUpdate.step: flat_grad must be one contiguous row of {self.total} elements, the parameters' gradients "
                             f"back to back (got shape {tuple(flat_grad.shape)})")
        if flat_grad.device != self.device:
            raise ValueError(f"FusedUpdate.step: flat_grad is on {flat_grad.device}, the parameters on {self.device}")
        _check_params(self.params)
        for k, (p, n) in enumerate(zip(self.params, self.numels)):
            if p.numel() != n or p.device != self.device:
                raise ValueError(f"FusedUpdate.step: parameter {k} changed its size or device ({p.numel()} elements on {p.device})")
        if self.device.type != "cuda":
            raise _lib.RadonLibraryError("FusedUpdate.step: the parameters must be CUDA tensors; there is no CPU path")
        ptrs = tuple(p.data_ptr() for p in self.params)
        if ptrs != self._ptrs:
            self._build_plan(ptrs)
        t = self.t + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().ctpvae_update_f32(self._plan.data_ptr(), self._partials.numel(), len(self.params), flat_grad.data_ptr(),
                                                     self.m.data_ptr(), self.v.data_ptr(), self._partials.data_ptr(), self.norms.data_ptr(),
                                                     t, adam_alpha(t, self.lr, self.beta1, self.beta2), self.clip_norm, self.beta1,
                                                     self.beta2, self.eps, _stream_ptr()), "update")
        self.t = t
        return self

    # -- torch.optim.Adam's state dictionary -----------------------------------------------------------------------
    def state_dict(self):
        """{"state": {k: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]} as torch.optim.Adam(params, lr, (beta1, beta2), eps)
        writes it after .t steps (no state before the first)."""
        template = torch.optim.Adam([torch.zeros(1)], lr=self.lr, betas=(self.beta1, self.beta2), eps=self.eps).state_dict()
        group = dict(template["param_groups"][0], params=list(range(len(self.params))))
        state = {}
        if self.t > 0:
            for k, (p, m, v) in enumerate(zip(self.params, self.m.split(self.numels), self.v.split(self.numels))):
                state[k] = {"step": torch.tensor(float(self.t)), "exp_avg": m.clone().view(p.shape), "exp_avg_sq": v.clone().view(p.shape)}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        """Takes a state dictionary of torch.optim.Adam over the same parameter list (or one of state_dict()): lr, betas and eps of its
        group, exp_avg and exp_avg_sq of every parameter; a parameter without an entry starts from zero moments.  There is ONE step
        count: the entries' steps must be equal."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError(f"FusedUpdate.load_state_dict: needs one parameter group of {len(self.params)} parameters")
        group, state = groups[0], state_dict["state"]
        ids = {pid: k for k, pid in enumerate(group["params"])}
        if any(pid not in ids for pid in state):
            raise ValueError("FusedUpdate.load_state_dict: a state entry belongs to no parameter of the group")
        steps = {int(float(s["step"])) for s in state.values()}
        if len(steps) > 1:
            raise ValueError(f"FusedUpdate.load_state_dict: the parameters' step counts differ ({sorted(steps)}); this update keeps one")
        for pid, s in state.items():
            n = self.numels[ids[pid]]
            if s["exp_avg"].numel() != n or s["exp_avg_sq"].numel() != n:
                raise ValueError(f"FusedUpdate.load_state_dict: the state of parameter {ids[pid]} does not have its {n} elements")
        self._set_hyper(group["lr"], group["betas"][0], group["betas"][1], group["eps"])
        self.m.zero_()
        self.v.zero_()
        ms, vs = self.m.split(self.numels), self.v.split(self.numels)
        for pid, s in state.items():
            ms[ids[pid]].copy_(s["exp_avg"].reshape(-1))
            vs[ids[pid]].copy_(s["exp_avg_sq"].reshape(-1))
        self.t = steps.pop() if steps else 0
