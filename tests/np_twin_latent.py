"""Twins of the fused Normal latent block (ct_pvae_amd/csrc/latent.hip; the trainer's chunk / positive_range / + sqrt_reg / repeat /
randn-multiply-add / kl_normal_std) and the per-sample acceptance rule the tests hold the kernels to.

    draws(n, length, ns, seed, draw, level, fo)   the kernels' signed tail probabilities v [ns][n][length] from a numpy Philox
                                                  (np_twin_hmc.philox)
    eps_of(v, dtype)                              copysign(-ndtri(|v|), v): float64 (scipy) is the definition of the draw, float32
                                                  (torch.special.ndtri on the float32 t) is the twin's
    compose(loc, log_scale, eps, sqrt_reg, ns, dtype)
                                                  the trainer's composition, operation by operation, in torch on the CPU with eps
                                                  injected: float64 on the float32 operands is the definition (its autograd IS the
                                                  gradient's definition), float32 is the "float32 twin"
    gradients(c, g_z, g_KL)                       autograd of sum(z g_z) + sum_b g_KL[b] sum_i kl[b][i]
    bars(ref, g_z, g_KL, generated)               a first-order float32 error bar per sample for eps, z, kl, g_loc, g_log_scale;
                                                  U = 2^-24, every term in float64 from the float64 composition's intermediates

The bar follows the roundings of the named intermediates through the composition (U and pr's rounding: np_twin_head):
    eps      2 U |eps| + U where the generator draws it (np_twin_head's quantile term with an exact argument: t is one float32 on the
             host and on the device), 0 where it is injected
    scale    pr rel_pr + U scale,   rel_pr = U (2 + |t - 1|) below t = 1, 2 U above;   scale = pr(log_scale) + sqrt_reg
    z        |eps| dscale + scale deps + U (|scale eps| + |z|)
    kl       0.5 (2 scale dscale + U (scale^2 + loc^2) + U (scale^2 + loc^2) + U |scale^2 + loc^2 - 1|)
             + dscale / scale + U |log scale| + U |kl|
    g_loc    U sum_(s >= 1) |P_s| + U |G loc| + U |g_loc|,  P_s the partial sums of g_z over s;  G = g_KL of the object
    g_scale  sum_s (|g_z| deps + U |g_z eps|) + U sum_(s >= 1) |Q_s| + |G| dT + U |G T| + U |g_scale|,
             Q_s the partial sums of g_z eps,  T = scale - 1 / scale,  dT = dscale (1 + 1 / scale^2) + U / scale + U |T|
    g_log_scale = pr' g_scale              pr' dg_scale + |g_log_scale| (rel_pr + U)

The rule (device): for EVERY sample |got - ref| <= MARGIN * R * bar, R = max(1, the float32 twin's own worst excess on the same
operands) and MARGIN = 4, np_twin_gauss's values; R <= R_MAX is asserted on the CPU (tests/test_latent_cpu.py).  No sample is left
out: the function has no clamp whose derivative jumps (pr has slope 1 on both sides of t = 1)."""
import numpy as np
import torch
from scipy.special import ndtri

from ct_pvae_amd import trainer as tr
from tests import np_twin_gauss as tg
from tests import np_twin_head as th
from tests import np_twin_hmc

TAG = 0x4C000000
U = th.U
MARGIN, R_MAX = tg.MARGIN, tg.R_MAX
EPS32 = th.EPS32
RANGES = {"wide": ((-3.0, 3.0), (-4.0, 2.5)), "trainer": ((-1.5, 1.5), (-2.0, 1.2))}
QUANTITIES = ("eps", "z", "kl", "g_loc", "g_log_scale")
excess, twin_ratio = tg.excess, tg.twin_ratio


def words(n, length, ns, seed, draw, level, first_object=0):
    """uint32 [ns][n][length]: word e & 3 of Philox((lo32(e >> 2), hi32(e >> 2), draw, TAG | level << 16 | s), seed),
    e = (first_object + b) * length + i."""
    e = ((int(first_object) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(length) + np.arange(length, dtype=np.uint64)[None, :])
    blk = e >> np.uint64(2)
    pick = (e & np.uint64(3)).astype(np.int64)[..., None]
    out = []
    for s in range(ns):
        w = np_twin_hmc.philox(blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), np.uint64(draw), TAG | (int(level) << 16) | s, int(seed))
        out.append(np.take_along_axis(w, pick, axis=-1)[..., 0])
    return np.stack(out)


def tail(w):
    """(((w >> 7) & 0xFFFFFF) + 0.5f) * 2^-25 in float32, negative where bit 31 of w is set."""
    k = ((w >> np.uint32(7)) & np.uint32(0xFFFFFF)).astype(np.float32)
    t = (k + np.float32(0.5)) * np.float32(2.0 ** -25)
    assert t.dtype == np.float32
    return np.where((w >> np.uint32(31)) != 0, -t, t)


def draws(n, length, ns, seed, draw, level, first_object=0):
    return tail(words(n, length, ns, seed, draw, level, first_object))


def eps_of(v, dtype=np.float64):
    """copysign(-ndtri(|v|), v).  float64: the definition; float32: the twin's own quantile of the same float32 t."""
    v = np.asarray(v, np.float32)
    if dtype == np.float64:
        return np.copysign(-ndtri(np.abs(v).astype(np.float64)), v.astype(np.float64))
    q = torch.special.ndtri(torch.from_numpy(np.abs(v))).numpy()
    assert q.dtype == np.float32
    return np.copysign(-q, v)


def operands(kind, n, length, seed):
    """float32 (loc, log_scale) [n][length], uniform on the raw-input range `kind`."""
    (a0, a1), (b0, b1) = RANGES[kind]
    rng = np.random.default_rng(seed)
    return rng.uniform(a0, a1, (n, length)).astype(np.float32), rng.uniform(b0, b1, (n, length)).astype(np.float32)


def cotangents(n, length, ns, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ns, n, length)).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def compose(loc, log_scale, eps, sqrt_reg, ns, dtype):
    """The trainer's lines on skip = [loc | log_scale] ([B][2][length], a leaf that requires grad) with eps [ns][B][length] in place of
    torch.randn; returns a dict of torch tensors: skip, loc, log_scale, scale [B][1][length], eps, z [ns * B][1][length], kl [B][1][length]."""
    sk = torch.tensor(np.stack([np.asarray(loc, np.float32), np.asarray(log_scale, np.float32)], axis=1)).to(dtype).requires_grad_(True)
    B, _, length = sk.shape
    e = torch.tensor(np.asarray(eps)).to(dtype).reshape(ns * B, 1, length)
    reg = float(np.float32(sqrt_reg))
    lo, ls = sk.chunk(2, dim=1)
    scale = tr.positive_range(ls) + reg
    z = lo.repeat(ns, 1, 1) + scale.repeat(ns, 1, 1) * e
    kl = tr.kl_normal_std(lo, scale)
    return dict(skip=sk, loc=lo, log_scale=ls, scale=scale, eps=e, z=z, kl=kl, ns=ns)


def gradients(c, g_z, g_KL):
    """(g_loc, g_log_scale) [B][length] as numpy arrays of the composition's dtype."""
    dt = c["z"].dtype
    gz = torch.tensor(np.asarray(g_z, np.float32)).to(dt).reshape(c["z"].shape)
    gk = torch.tensor(np.asarray(g_KL, np.float32)).to(dt)
    loss = (c["z"] * gz).sum() + (c["kl"].sum(dim=(1, 2)) * gk).sum()
    g, = torch.autograd.grad(loss, c["skip"], retain_graph=True)
    return g[:, 0].numpy(), g[:, 1].numpy()


def values(c):
    """eps, z [ns][B][length] and kl [B][length] of a composition as numpy arrays."""
    B, length = c["kl"].shape[0], c["kl"].shape[2]
    return dict(eps=c["eps"].detach().numpy().reshape(c["ns"], B, length), z=c["z"].detach().numpy().reshape(c["ns"], B, length),
                kl=c["kl"].detach().numpy().reshape(B, length))


def bars(ref, g_z, g_KL, generated):
    """dict eps, z [ns][B][length], kl, g_loc, g_log_scale [B][length] of float64 arrays from the float64 composition `ref`.
    generated: eps came from the generator (its own rounding counts) rather than injected as float32 values (exact)."""
    v = {k: a.astype(np.float64) for k, a in values(ref).items()}
    eps, z, kl = v["eps"], v["z"], v["kl"]
    loc = ref["loc"].detach().numpy().astype(np.float64)[:, 0]
    ls = ref["log_scale"].detach().numpy().astype(np.float64)[:, 0]
    scale = ref["scale"].detach().numpy().astype(np.float64)[:, 0]
    gz = np.asarray(g_z, np.float64)
    G = np.broadcast_to(np.asarray(g_KL, np.float64)[:, None], loc.shape)
    with np.errstate(all="ignore"):
        rel_pr = U * np.where(ls < 1, 2 + np.abs(ls - 1), 2.0)
        dpr = np.where(ls < 1, np.exp(np.maximum(ls - 1, -1e10)), 1.0)
        pr = np.where(ls < 1, dpr + EPS32, ls)
        dscale = pr * rel_pr + U * scale
        deps = (2 * U * np.abs(eps) + U) if generated else np.zeros_like(eps)
        dz = np.abs(eps) * dscale + scale * deps + U * (np.abs(scale * eps) + np.abs(z))
        sq = scale * scale + loc * loc
        dkl = 0.5 * (2 * scale * dscale + 2 * U * sq + U * np.abs(sq - 1)) + dscale / scale + U * np.abs(np.log(scale)) + U * np.abs(kl)
        P = np.cumsum(gz, axis=0)
        g_loc = P[-1] + G * loc
        dg_loc = U * np.abs(P[1:]).sum(axis=0) + U * np.abs(G * loc) + U * np.abs(g_loc)
        Q = np.cumsum(gz * eps, axis=0)
        T = scale - 1 / scale
        dT = dscale * (1 + 1 / (scale * scale)) + U / scale + U * np.abs(T)
        g_scale = Q[-1] + G * T
        dg_scale = ((np.abs(gz) * deps + U * np.abs(gz * eps)).sum(axis=0) + U * np.abs(Q[1:]).sum(axis=0) + np.abs(G) * dT
                    + U * np.abs(G * T) + U * np.abs(g_scale))
        g_ls = dpr * g_scale
        return dict(eps=deps, z=dz, kl=dkl, g_loc=dg_loc, g_log_scale=dpr * dg_scale + np.abs(g_ls) * (rel_pr + U))


def case(kind, n, length, ns, seed, eps=None, first_object=0, draw=0, level=0, operands_=None, sqrt_reg=EPS32, cotangents_=None):
    """Operands (of range `kind`, or operands_ = (loc, log_scale)), cotangents, the draws (the generator's v for (seed, draw, level,
    first_object) unless eps [ns][n][length], float32, is injected), the float64 reference, its gradients and bars, and R per quantity.
    cotangents_ = (g_z, g_KL) replaces the seeded ones."""
    loc, log_scale = operands(kind, n, length, seed) if operands_ is None else operands_
    g_z, g_KL = cotangents(n, length, ns, seed + 1) if cotangents_ is None else cotangents_
    generated = eps is None
    if generated:
        v = draws(n, length, ns, seed, draw, level, first_object)
        eps64, eps32 = eps_of(v, np.float64), eps_of(v, np.float32)
    else:
        v = None
        eps32 = np.asarray(eps, np.float32)
        eps64 = eps32.astype(np.float64)
    ref = compose(loc, log_scale, eps64, sqrt_reg, ns, torch.float64)
    twin = compose(loc, log_scale, eps32, sqrt_reg, ns, torch.float32)
    bar = bars(ref, g_z, g_KL, generated)
    want = dict(zip(("g_loc", "g_log_scale"), gradients(ref, g_z, g_KL)), **values(ref))
    got = dict(zip(("g_loc", "g_log_scale"), gradients(twin, g_z, g_KL)), **values(twin))
    R = {k: twin_ratio(got[k], want[k], bar[k]) for k in QUANTITIES}
    return dict(loc=loc, log_scale=log_scale, v=v, eps32=eps32, g_z=g_z, g_KL=g_KL, ref=ref, want=want, twin=got, bar=bar, R=R, ns=ns,
                sqrt_reg=sqrt_reg)


def ordered_sum(kl_elem):
    """float32 sum of one object's kl_elem [length] in csrc/latent.hip's order: quad, the thread's quads at stride 1024, the xor
    butterfly 32 .. 1 inside each wave of 64 threads, the 16 waves ascending."""
    F = np.float32
    x = np.asarray(kl_elem, F)
    quads = -(-x.size // 4)
    q = np.zeros(quads * 4, F)
    q[:x.size] = x
    q = q.reshape(quads, 4)
    s = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
    acc = np.zeros(1024, F)
    for start in range(0, quads, 1024):
        part = s[start:start + 1024]
        acc[:part.size] = acc[:part.size] + part
    lane = np.arange(64)
    waves = acc.reshape(16, 64)
    for m in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ m]
    total = waves[0, 0]
    for k in range(1, 16):
        total = F(total + waves[k, 0])
    assert waves.dtype == F
    return F(total)


def kernel_form(loc, log_scale, eps, g_z, g_KL, sqrt_reg=EPS32):
    """csrc/latent.hip's own expressions (its header: the forward and the backward's closed form, sums over s ascending) in numpy
    float32, operation by operation, on given eps [ns][B][length].  Returns the dict z, kl, g_loc, g_log_scale.  What the CPU can say
    about the kernels' algebra; the device itself: tests/test_gpu_latent.py."""
    F = np.float32
    loc, ls, eps, gz = (np.asarray(a, F) for a in (loc, log_scale, eps, g_z))
    G = np.broadcast_to(np.asarray(g_KL, F)[:, None], loc.shape)
    with np.errstate(all="ignore"):
        e = np.exp(ls - F(1))
        scale = np.where(ls >= 1, ls, e + F(EPS32)) + F(sqrt_reg)
        dscale = np.where(ls >= 1, F(1), e)
        z = loc[None] + scale[None] * eps
        kl = F(0.5) * (scale * scale + loc * loc - F(1)) - np.log(scale)
        g_loc, g_scale = np.zeros_like(loc), np.zeros_like(loc)
        for s in range(eps.shape[0]):
            g_loc = g_loc + gz[s]
            g_scale = g_scale + gz[s] * eps[s]
        g_loc = g_loc + G * loc
        g_scale = (g_scale + G * (scale - F(1) / scale)) * dscale
    out = dict(z=z, kl=kl, g_loc=g_loc, g_log_scale=g_scale)
    assert all(a.dtype == F for a in out.values())
    return out
