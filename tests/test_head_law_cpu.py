"""The LAW of the TruncatedNormal head's sampler, on the CPU twins (tests/np_twin_head.compose fed the numpy Philox's uniforms): x is a
sample of N(loc, scale^2) truncated to [0, inf), by the closed-form CDF of tests/np_law.py -- not by the twin, which restates the
kernel's quantile construction.  The device's own x: tests/test_gpu_head_law.py, which takes its ranges, seeds and rule from here.

Per raw-operand range ("trainer", "trunc", "wide"), 2^20 pixels with random operands, the pooled PIT:
    left out        samples with x = 0 (the floor) or whose p met a bound of its clamp; their share must be <= 1e-3
    KS              ks_uniform(pit_truncnorm(loc, scale, x)) <= dkw(N) of the samples kept (Dvoretzky-Kiefer-Wolfowitz at 1e-6)
    neighbours      |corr| of the PITs of neighbouring pixels (both kept) <= corr_bound = 5.5 / sqrt(pairs)
A sampler is refused when it misses any of the three.  Leaving samples out is a rejection step: a sampler that forgets the
truncation and has its negative x floored at 0 leaves, after the floor's samples are dropped, exactly the truncated law -- what refuses
it is the cap on the share.

Measured at N = 2^20 (the figures the tests print; none of them sets a bound):
                              left out   KS / dkw   |corr| / corr_bound
    trainer                   0          0.281      0.389          (the float32 twin's figures equal the float64 twin's to 1e-3)
    trunc                     0          0.199      0.261
    wide                      9.5e-7     0.346      0.140
    z_is_1 on trunc           0          171        0.252          refused by KS
    no_truncation on trunc    0.451      0.397      0.164          refused by the cap on the share alone
    flip_lower on trunc       0          28.3       0.052          refused by KS
    flip_lower on trainer     0          180        0.292          refused by KS"""
import numpy as np
import pytest
import torch

from tests import np_law as law
from tests import np_twin_beta as tb
from tests import np_twin_head as th

F, D = np.float32, np.float64
SEED = 0x5EED0123456789
N = 2 ** 20
LEFT_OUT_CAP = 1e-3
POOLED = {kind: (200 + i, i) for i, kind in enumerate(th.RANGES)}               # range -> (operand seed, draw)
_uniforms = {}


def case(kind):
    """(alpha, beta [1][N] float32, u [1][N] float32 of the numpy Philox for (SEED, the range's draw))."""
    seed, draw = POOLED[kind]
    if kind not in _uniforms:
        _uniforms[kind] = th.uniforms(1, N, SEED, draw)
    return th.operands(kind, 1, N, seed) + (_uniforms[kind],)


def p_clamped(alpha, beta, u):
    """bool [n][pix]: the float64 composition's p met a bound of its clamp (the device keeps no p: the reference's says which)."""
    with torch.no_grad():
        p0 = th.compose(alpha, beta, u, torch.float64)["p0"].numpy()
    return (p0 < th.P_LO) | (p0 > th.P_HI)


def verdict(alpha, beta, x, clamped):
    """dict share (left out), ks, corr (ratios to dkw and corr_bound of the samples kept), refused."""
    t = np.stack([alpha, beta], axis=-1)
    c, _ = tb._pr(t, D)                                                         # positive_range of the float32 operands, float64
    x = np.asarray(x, D)
    keep = (x > 0) & ~clamped
    p = law.pit_truncnorm(c[..., 0], c[..., 1], x)
    pairs = keep[:, :-1] & keep[:, 1:]
    out = dict(share=float(1 - keep.mean()), ks=law.ks_uniform(p[keep]) / law.dkw(int(keep.sum())),
               corr=abs(law.corr(p[:, :-1][pairs], p[:, 1:][pairs])) / law.corr_bound(int(pairs.sum())))
    out["refused"] = out["share"] > LEFT_OUT_CAP or out["ks"] > 1.0 or out["corr"] > 1.0
    return out


def twin_x(kind, dtype, defect=None):
    alpha, beta, u = case(kind)
    with torch.no_grad():
        c = th.compose(alpha, beta, u, dtype, defect=defect)
    return alpha, beta, c["x"].numpy(), p_clamped(alpha, beta, u)


@pytest.mark.parametrize("kind", list(th.RANGES))
def test_pooled_range_follows_the_truncated_normal_law(kind):
    for name, dt in (("float64", torch.float64), ("float32", torch.float32)):
        v = verdict(*twin_x(kind, dt))
        print(f"{kind} {name}: left out {v['share']:.2e} (cap {LEFT_OUT_CAP:g}), KS / dkw {v['ks']:.3f}, |corr| / corr_bound {v['corr']:.3f}")
        assert v["share"] <= LEFT_OUT_CAP and v["ks"] <= 1.0 and v["corr"] <= 1.0, (kind, name, v)


@pytest.mark.parametrize("defect,kind", [("z_is_1", "trunc"), ("no_truncation", "trunc"), ("flip_lower", "trunc"), ("flip_lower", "trainer")])
def test_the_law_test_bites(defect, kind):
    """Wrong twins are refused: Z taken as 1 in p = Pa + u Z (the truncation's scale forgotten), on "trunc" -- by KS: the draws past
    p = 1 pile up at the clamp; the truncation forgotten altogether (p = u) -- by the cap on the share left out alone, see this file's
    docstring; 1 - u in place of u where p falls on the lower half -- by KS."""
    v = verdict(*twin_x(kind, torch.float64, defect))
    print(f"control {defect} on {kind}: left out {v['share']:.2e} (cap {LEFT_OUT_CAP:g}), KS / dkw {v['ks']:.3f}, |corr| / corr_bound {v['corr']:.3f}")
    assert v["refused"], (defect, kind, v)
    if defect != "no_truncation":
        assert v["ks"] > 1.0
    else:
        assert v["share"] > LEFT_OUT_CAP
