"""recon(algorithm='mlem' | 'osem') without a GPU: the names, the ABI, the argument checks that need no device, and the
properties of the numpy twin the GPU tests compare against (tests/np_twin_mlem.py) -- including the case that shows why the
build guards the ratio where libtomo does not."""
import os
import re
import subprocess

import numpy as np
import pytest

from ct_pvae_amd import phantoms
from tests import np_twin_mlem as tw
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ctpvae_radon.h")
NEW_SYMBOLS = ("ctpvae_siddon_fwd_ratio_f32", "ctpvae_siddon_bwd_sel_mul_f32")
N, A, COUNTS = 64, 45, 50.0


@pytest.fixture(scope="module")
def foam(oracle):
    """3 foam slices at 64^2, 45 angles over pi, pad=True: (phantom, theta, clean sinograms, Poisson-noised at 50 counts per unit),
    sinograms [3][45][94]."""
    img = phantoms.foam_batch(3, N, seed=4, supersample=2)
    theta = np.linspace(0.0, np.pi, A, endpoint=False).astype(np.float32)
    sino = np.ascontiguousarray(np.swapaxes(oracle.siddon_project(img, theta, pad=True), 0, 1))
    noisy = (np.random.default_rng(0).poisson(sino.astype(np.float64) * COUNTS) / COUNTS).astype(np.float32)
    return img, theta, sino, noisy


def test_names_symbols_and_trainer_flag():
    import importlib
    from ct_pvae_amd import _lib
    from ct_pvae_amd import trainer as tr
    recon = importlib.import_module("ct_pvae_amd.recon")        # (the package exports the function `recon` under the same name)
    assert "mlem" in recon.ALGORITHMS and "osem" in recon.ALGORITHMS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ctpvae_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    macro = int(re.search(r"#define\s+CTPVAE_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert _lib.load().ctpvae_abi_version() == _lib.ABI_VERSION == macro == 3400
    args = tr.get_args("--nsa 20 --td 6 -b 3 --train --algorithms mlem osem gridrec".split())
    assert args.algorithms == ["mlem", "osem", "gridrec"] and all(a in recon.ALGORITHMS for a in args.algorithms)
    assert len(args.algorithms) + 1 == 4                              # the encoder's input channels (PVAETrainer: EncodeNet(len + 1, ...))
    assert "art" not in recon.ALGORITHMS


def test_entry_points_refuse_bad_arguments():
    from ct_pvae_amd import _lib
    lib = _lib.load()
    null16 = [None, 1, 8, 8, None, None, None, 4, 12, 6.0, None, 0, None, None, None, None]
    assert lib.ctpvae_siddon_fwd_ratio_f32(*null16) == _lib.EINVAL
    assert lib.ctpvae_siddon_bwd_sel_mul_f32(*null16) == _lib.EINVAL


def test_osem_blocks_and_keyword_checks():
    """The subsets of osem.c, and the checks recon() makes before it touches a device."""
    import importlib
    import torch
    rc = importlib.import_module("ct_pvae_amd.recon")
    assert [b.tolist() for b in rc._osem_blocks(7, 3, None)] == [[0, 1], [2, 3], [4, 5, 6]]
    assert [b.tolist() for b in rc._osem_blocks(4, None, [3, 1, 0, 2])] == [[3, 1, 0, 2]]
    assert [b.tolist() for b in tw.blocks_of(7, 3)] == [[0, 1], [2, 3], [4, 5, 6]]
    assert [len(b) for b in rc._osem_blocks(45, 7, None)] == [6] * 6 + [9]
    for nb, ind in ((0, None), (-1, None), (8, None), (2, [0, 1, 2]), (2, np.arange(7.0)), (2, [0, 1, 2, 3, 4, 5, 7]),
                    (1, [[0, 1, 2, 3, 4, 5, 6]])):
        with pytest.raises(ValueError):
            rc._osem_blocks(7, nb, ind)
    x = torch.zeros((2, 7, 12))
    for kw in ({"num_block": 2}, {"ind_block": np.arange(7)}):
        for alg in ("sirt", "mlem", "fbp", "gridrec", "tv"):
            with pytest.raises(ValueError, match="belong to algorithm='osem'"):
                rc.recon(x, np.zeros(7), sinogram_order=True, algorithm=alg, **kw)


def test_twin_properties(oracle, foam):
    """MLEM's guarantees on the twin: finite iterates, the guarded and libtomo's rule agree bit for bit on plain MLEM, the counts are
    preserved, the Poisson log-likelihood rises, and 20 iterations reconstruct the phantom where 4 do not."""
    img, theta, sino, noisy = foam
    P = sino.shape[2]
    lo = P // 2 - N // 2
    base = float((img ** 2).mean())
    for name, data in (("clean", sino), ("noisy", noisy)):
        guarded, libtomo = [], []
        tw.mlem(data, theta, 20, each=lambda it, x: guarded.append(x.copy()))
        tw.mlem(data, theta, 20, rule="libtomo", each=lambda it, x: libtomo.append(x.copy()))
        assert all(np.isfinite(x).all() for x in guarded)
        assert all(np.array_equal(a, b) for a, b in zip(guarded, libtomo))
        sims = [oracle._project_grid(x, theta, P) for x in guarded]
        total = data.astype(np.float64).sum()
        counts = [s.astype(np.float64).sum() / total for s in sims]
        ll = [tw.poisson_loglik(data, s) for s in sims]
        mse = [float(((x[:, lo:lo + N, lo:lo + N] - img) ** 2).mean()) / base for x in guarded]
        print(f"{name}: count ratio - 1 in [{min(counts) - 1:.1e}, {max(counts) - 1:.1e}]; log-likelihood at 1 / 5 / 20 iterations "
              f"{ll[0]:.4e} {ll[4]:.4e} {ll[19]:.4e}; cropped MSE / mean square at 4 / 20 iterations {mse[3]:.3f} {mse[19]:.3f}")
        assert max(abs(c - 1.0) for c in counts) <= 1e-6
        assert ll[0] < ll[4] < ll[19]
        assert mse[19] < 0.1 and not mse[3] < 0.1


def test_libtomo_rule_breaks_on_contiguous_blocks(foam):
    """Why the ratio is guarded: with 5 contiguous blocks a block drives the pixels outside the object to exactly 0, the next block
    then divides 0 by 0 on rays that do cross pixels, and libtomo's rule (skip only rays without segments) loses the whole image."""
    _, theta, sino, _ = foam
    assert not np.isfinite(tw.mlem(sino, theta, 4, num_block=5, rule="libtomo")).all()
    got = tw.mlem(sino, theta, 4, num_block=5)
    assert np.isfinite(got).all() and (got >= 0).all()
    np.testing.assert_array_equal(tw.mlem(sino, theta, 2, num_block=1), tw.mlem(sino, theta, 2))
