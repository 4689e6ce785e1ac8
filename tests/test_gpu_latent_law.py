"""The LAW of the fused Normal latent sampler on the device (csrc/latent.hip): (z - loc) / scale is a standard normal sample.  One
launch of 2^20 samples pooled over tests/test_gpu_latent.py's operand kinds -- object 0 on the "wide" range, object 1 on "trainer",
len = 4 x 256 x 256, ns = 2 -- standardised in float64 with scale = positive_range(log_scale) + sqrt_reg of the float32 operands,
through Phi: ks_uniform <= dkw(N), the Dvoretzky-Kiefer-Wolfowitz bound at 1e-6 (tests/np_law.py).  The law comes from scipy's
Phi, not from the twin.  (The means of the KL term's gradients are not tested here.)

Measured on an MI355X (the figures the test prints; they set no bound):
    KS / dkw of the pooled 2^20: 0.343 (the kinds alone, each against the dkw of its 2^19: wide 0.524, trainer 0.210)"""
import numpy as np
import pytest

from tests import np_law as law
from tests import np_twin_beta as tb
from tests import np_twin_latent as tl
from tests.test_gpu_latent import SEED, run_latent

pytestmark = pytest.mark.gpu

CHW, NS, LEVEL, DRAW = (4, 256, 256), 2, 1, 9
OPERAND_SEED = 300


def test_standardised_latents_follow_the_standard_normal_law():
    length = CHW[0] * CHW[1] * CHW[2]
    kinds = list(tl.RANGES)
    assert kinds == ["wide", "trainer"] and NS * len(kinds) * length == 2 ** 20
    ops = [tl.operands(kind, 1, length, OPERAND_SEED + i) for i, kind in enumerate(kinds)]
    loc, log_scale = (np.concatenate([o[j] for o in ops]) for j in (0, 1))
    d = run_latent(loc, log_scale, NS, 0, LEVEL, CHW, draw=DRAW, seed=SEED)
    z = d["z"].astype(np.float64)
    assert z.shape == (NS, len(kinds), length) and np.isfinite(z).all()
    scale = tb._pr(log_scale, np.float64)[0] + float(np.float32(tl.EPS32))         # positive_range, float64, + sqrt_reg
    p = law.pit_normal((z - loc.astype(np.float64)[None]) / scale[None])
    ratio = law.ks_uniform(p) / law.dkw(p.size)
    per_kind = [law.ks_uniform(p[:, i]) / law.dkw(p[:, i].size) for i in range(len(kinds))]
    print(f"latents device: KS / dkw of the pooled 2^20 {ratio:.3f} (per kind, not asserted: " +
          ", ".join(f"{k} {v:.3f}" for k, v in zip(kinds, per_kind)) + ")")
    assert ratio <= 1.0, ratio
