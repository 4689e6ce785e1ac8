"""recon(algorithm='pml_quad' | 'pml_hybrid' | 'ospml_quad' | 'ospml_hybrid') without a GPU: the names, the ABI, the argument checks
that need no device, and the properties of the numpy twin the GPU tests compare against (tests/np_twin_pml.py) -- that its update
is the surrogate's (the penalized likelihood rises at every iteration, the penalty does what it is for, beta = 0 is mlem), and the
case that shows why the build writes the root in another form than libtomo does."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from ct_pvae_amd import phantoms
from tests import np_twin_mlem as tm
from tests import np_twin_pml as tw
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ctpvae_radon.h")
SYMBOL = "ctpvae_siddon_bwd_sel_pml_f32"
NAMES = ("pml_quad", "pml_hybrid", "ospml_quad", "ospml_hybrid")
N, A, COUNTS = 64, 45, 50.0


@pytest.fixture(scope="module")
def foam(oracle):
    """The input of tests/test_mlem_cpu.py: 3 foam slices at 64^2, 45 angles over pi, pad=True, Poisson-noised at 50 counts per unit
    (seed 0): (theta, noisy sinograms [3][45][94])."""
    img = phantoms.foam_batch(3, N, seed=4, supersample=2)
    theta = np.linspace(0.0, np.pi, A, endpoint=False).astype(np.float32)
    sino = np.ascontiguousarray(np.swapaxes(oracle.siddon_project(img, theta, pad=True), 0, 1))
    noisy = (np.random.default_rng(0).poisson(sino.astype(np.float64) * COUNTS) / COUNTS).astype(np.float32)
    return theta, noisy


@pytest.fixture(scope="module")
def quad_runs(foam):
    """pml_quad's 20 float32 iterates on one block, per beta (shared by the tests below; not modified)."""
    theta, noisy = foam
    runs = {}
    for beta in (0.01, 0.05, 1.0):
        its = []
        tw.pml(noisy, theta, 20, beta, each=lambda it, x: its.append(x.copy()))
        runs[beta] = its
    return runs


def test_names_symbol_and_trainer_flag():
    from ct_pvae_amd import _lib
    from ct_pvae_amd import trainer as tr
    recon = importlib.import_module("ct_pvae_amd.recon")        # (the package exports the function `recon` under the same name)
    assert all(n in recon.ALGORITHMS for n in NAMES)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ctpvae_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    assert SYMBOL in declared and SYMBOL in exported and SYMBOL in _lib.SIGNATURES
    assert SYMBOL in open(HEADER).read().split("#ifndef CTPVAE_RADON_H")[0]            # the header's index comment
    macro = int(re.search(r"#define\s+CTPVAE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert _lib.load().ctpvae_abi_version() == _lib.ABI_VERSION == macro == 3400
    args = tr.get_args("--nsa 20 --td 6 -b 3 --train --algorithms pml_quad ospml_hybrid gridrec".split())
    assert args.algorithms == ["pml_quad", "ospml_hybrid", "gridrec"] and all(a in recon.ALGORITHMS for a in args.algorithms)


def test_entry_point_refuses_bad_arguments():
    """EINVAL before any HIP call (there is no device here): null pointers, x_in == x_out, a 1-wide grid, a bad beta / delta.  The
    pointers are never followed: any non-null value stands for a buffer."""
    from ct_pvae_amd import _lib
    lib = _lib.load()
    p, q = 4096, 8192

    def call(ratio=p, ox=8, oz=8, sin=p, cos=p, quad=p, ws=p, colsum=p, beta=1.0, delta=1.0, hybrid=0, x_in=p, x_out=q):
        return lib.ctpvae_siddon_bwd_sel_pml_f32(ratio, 1, ox, oz, sin, cos, quad, 4, 12, 6.0, None, 0, ws, colsum, beta, delta, hybrid,
                                                 x_in, x_out, None)
    for name in ("ratio", "sin", "cos", "quad", "ws", "colsum", "x_in", "x_out"):
        assert call(**{name: None}) == _lib.EINVAL, name
    assert call(x_in=p, x_out=p) == _lib.EINVAL
    assert call(ox=1) == _lib.EINVAL and call(oz=1) == _lib.EINVAL
    for beta in (-1.0, float("nan"), float("inf")):
        assert call(beta=beta) == _lib.EINVAL
    for delta in (0.0, -1.0, float("nan")):
        assert call(hybrid=1, delta=delta) == _lib.EINVAL


def test_keyword_checks_run_before_any_device_use():
    import torch
    from ct_pvae_amd import _lib
    rc = importlib.import_module("ct_pvae_amd.recon")
    x = torch.zeros((2, 7, 12))                          # a CPU tensor: a call that passes the keyword checks ends at "no CPU path"
    bad = [("pml_quad", -1.0), ("pml_quad", [float("nan")]), ("pml_quad", []), ("ospml_quad", [-0.5, 1.0]), ("pml_hybrid", 1.0),
           ("pml_hybrid", [1.0]), ("pml_hybrid", [1.0, 0.0]), ("ospml_hybrid", [1.0, -2.0]), ("ospml_hybrid", [-1.0, 1.0])]
    for alg, reg_par in bad:
        with pytest.raises(ValueError, match="reg_par"):
            rc.recon(x, np.zeros(7), sinogram_order=True, algorithm=alg, reg_par=reg_par)
    for alg in ("pml_quad", "pml_hybrid"):
        for kw in ({"num_block": 2}, {"ind_block": np.arange(7)}):
            with pytest.raises(ValueError, match="belong to algorithm='osem'"):
                rc.recon(x, np.zeros(7), sinogram_order=True, algorithm=alg, **kw)
    for alg, kw in (("ospml_quad", {"num_block": 2}), ("ospml_hybrid", {"ind_block": np.arange(7)}), ("pml_quad", {"reg_par": 0}),
                    ("pml_hybrid", {"reg_par": [0.5, 0.1]}), ("pml_hybrid", {}), ("ospml_quad", {"reg_par": [2.0, 3.0, 4.0]})):
        with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):
            rc.recon(x, np.zeros(7), sinogram_order=True, algorithm=alg, **kw)
    assert rc._pml_reg_par("pml_quad", None) == (1.0, 1.0, False) and rc._pml_reg_par("ospml_hybrid", None) == (1.0, 1.0, True)
    assert rc._pml_reg_par("pml_hybrid", [0.5, 0.1]) == (0.5, 0.1, True) and rc._pml_reg_par("ospml_quad", 3) == (3.0, 1.0, False)


def test_weights_are_libtomos_tables():
    """On a 3 x 3 grid (one interior pixel, four edges, four corners) the weights of every pixel sum to 1 and are the three tables."""
    w = tw.weights(3, 3)
    assert w.dtype == np.float32 and w.shape == (8, 3, 3)
    np.testing.assert_allclose(w.astype(np.float64).sum(0), 1.0, rtol=0, atol=2e-7)
    assert (np.count_nonzero(w, axis=0) == [[3, 5, 3], [5, 8, 5], [3, 5, 3]]).all()
    s = np.sqrt(2.0)
    for (i, j), n_dir, n_dia in (((1, 1), 4, 4), ((0, 1), 3, 2), ((1, 2), 3, 2), ((0, 0), 2, 1), ((2, 2), 2, 1)):
        a = 1.0 / (n_dir + n_dia / s)
        got = w[:, i, j]
        assert sorted(set(got[got != 0].tolist())) == [np.float32(a / s), np.float32(a)], (i, j)
        assert np.count_nonzero(got[:4]) == n_dir and np.count_nonzero(got[4:]) == n_dia
    assert w[0, 0, 0] == np.float32(0.3693980625) and w[4, 0, 0] == np.float32(0.2612038750)
    assert w[1, 0, 1] == np.float32(0.2265409197) and w[4, 0, 1] == np.float32(0.1601886205)
    assert w[3, 1, 1] == np.float32(0.1464466094) and w[7, 1, 1] == np.float32(0.1035533906)
    assert w[1, 0, 0] == 0 and w[3, 0, 1] == 0                 # (0, -1) of the first column, (-1, 0) of the first row
    with pytest.raises(ValueError):
        tw.weights(1, 5)
    assert tw.penalty(np.full((2, 4, 5), 3.0)) == 0.0
    x = np.zeros((1, 2, 2))
    x[0, 0, 0] = 1.0              # three pairs, each counted from both ends: 1/2 * 2 * (2 * 0.3694 + 0.2612)
    np.testing.assert_allclose(tw.penalty(x), 2 * 0.3693980625 + 0.2612038750, rtol=1e-7)


def test_twin_iterates_are_finite_and_not_negative(foam, quad_runs):
    theta, noisy = foam
    for nb in (1, 5):
        for beta in (0.01, 1.0):
            for hybrid in (False, True):
                if nb == 1 and not hybrid:
                    its = quad_runs[beta]
                else:
                    its = []
                    tw.pml(noisy, theta, 20, beta, 0.1, hybrid, num_block=nb, each=lambda it, x: its.append(x))
                assert len(its) == 20 and all(x.dtype == np.float32 and np.isfinite(x).all() and (x >= 0).all() for x in its), \
                    (nb, beta, hybrid)


def test_twin_raises_the_penalized_likelihood(oracle, foam, quad_runs):
    """The surrogate's guarantee, which a misremembered update would not have: loglik(x) - beta * penalty(x) rises at every
    iteration of one block (observed: strictly, smallest step about 7e1)."""
    theta, noisy = foam
    P = noisy.shape[2]
    for beta in (0.05, 1.0):
        obj = [tm.poisson_loglik(noisy, oracle._project_grid(x, theta, P)) - beta * tw.penalty(x) for x in quad_runs[beta]]
        steps = np.diff(obj)
        print(f"beta {beta}: objective {obj[0]:.5e} -> {obj[-1]:.5e}, smallest step {steps.min():.3e}")
        assert (steps > 0).all(), (beta, steps.min())


def test_twin_penalty_orders_the_estimators(foam, quad_runs):
    """At beta = 1 the quadratic penalty smooths more than the edge-preserving one, and both more than plain mlem (observed: 157.8 <
    175.4 < 188.8); with beta = 0 the update is mlem's up to rounding (observed: 4.7e-7 of the maximum after 5 iterations)."""
    theta, noisy = foam
    quad = tw.penalty(quad_runs[1.0][-1])
    hyb = tw.penalty(tw.pml(noisy, theta, 20, 1.0, 0.1, True))
    ml = tw.penalty(tm.mlem(noisy, theta, 20))
    print(f"penalty after 20 iterations: pml_quad {quad:.1f}, pml_hybrid(delta=0.1) {hyb:.1f}, mlem {ml:.1f}")
    assert quad < hyb < ml
    m5, p5 = tm.mlem(noisy, theta, 5), tw.pml(noisy, theta, 5, 0.0)
    e = float(np.abs(p5.astype(np.float64) - m5).max() / m5.max())
    print(f"beta = 0 against mlem, 5 iterations: {e:.2e}")
    assert e <= 5 * 1e-5


def test_why_the_root_is_rewritten(foam, quad_runs):
    """At beta = 0.01, 20 iterations: the float32 run with the build's form of the root stays within 1e-5 of the same iteration in
    float64, the float32 run with libtomo's form does not (observed: at most 1.5e-6 against 7e-5 and more)."""
    theta, noisy = foam
    ref = tw.pml(noisy, theta, 20, 0.01, dtype=np.float64)
    assert ref.dtype == np.float64
    stable = float(np.abs(quad_runs[0.01][-1] - ref).max() / ref.max())
    libtomo = float(np.abs(tw.pml(noisy, theta, 20, 0.01, rule="libtomo") - ref).max() / ref.max())
    print(f"beta 0.01 against float64: stable {stable:.2e}, libtomo's form {libtomo:.2e}")
    assert stable <= 1e-5 and not libtomo <= 1e-5
