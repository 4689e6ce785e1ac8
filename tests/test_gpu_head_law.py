"""The LAW of the fused TruncatedNormal output head on the device (csrc/head.hip, tn_head.h): the rule of tests/test_head_law_cpu.py
-- its ranges, seeds, draws -- on the device's own x.  Per raw-operand range one launch of n = 1, pix = 2^20: the share of samples
left out (x = 0, or the float64 composition's p at a bound of its clamp) <= 1e-3, ks_uniform(pit_truncnorm(loc, scale, x)) <= dkw of
the samples kept, the PITs of neighbouring pixels uncorrelated within corr_bound.  The law comes from the closed-form CDF
(tests/np_law.py), not from the twin.

Measured on an MI355X (the figures the test prints; none of them sets a bound):
                left out   KS / dkw   |corr| / corr_bound
    trainer     0          0.281      0.389
    trunc       0          0.199      0.261
    wide        9.5e-7     0.346      0.140"""
import numpy as np
import pytest

from tests import test_head_law_cpu as cpu
from tests import np_twin_head as th
from tests.test_gpu_head import run_head

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", list(th.RANGES))
def test_pooled_range_follows_the_truncated_normal_law(kind):
    alpha, beta, u = cpu.case(kind)
    _, draw = cpu.POOLED[kind]
    x = run_head(alpha, beta, 0, draw, seed=cpu.SEED)[0]
    assert x.shape == alpha.shape and np.isfinite(x).all() and (x >= 0).all()
    v = cpu.verdict(alpha, beta, x, cpu.p_clamped(alpha, beta, u))
    print(f"{kind} device: left out {v['share']:.2e} (cap {cpu.LEFT_OUT_CAP:g}), KS / dkw {v['ks']:.3f}, |corr| / corr_bound {v['corr']:.3f}")
    assert v["share"] <= cpu.LEFT_OUT_CAP and v["ks"] <= 1.0 and v["corr"] <= 1.0, (kind, v)
