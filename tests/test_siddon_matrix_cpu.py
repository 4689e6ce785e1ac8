"""tests/np_twin_siddon.py against the oracle's own compositions, on the small grids of tests/test_gpu_siddon_matrix.py: the twin
that holds the expected values of every store of the ray-driven projector pair is itself tested, without a GPU.

Every float32 store equals the same operations in float64 rounded to float32 after EACH operation (53 >= 2 * 24 + 2 bits: a float64
sum, product or quotient of two float32 values, rounded once more, is the correctly rounded float32 result) -- a store that numpy had
quietly evaluated in float64, or in another order, would not.  One iteration of mlem, of an osem block, of pml_quad and of the TV
stand-in composed from the twin's pieces equals the iteration the oracle-side restatements compute, bit for bit."""
import numpy as np
import pytest

from tests import np_twin_gauss as tg
from tests import np_twin_mlem as tm
from tests import np_twin_pml as tp
from tests import np_twin_siddon as tw

F, D = np.float32, np.float64
SMALL = tw.GRIDS[:2]


def r32(a):
    return np.asarray(a, D).astype(F).astype(D)


def test_operands_hit_their_edges():
    th = tw.angles()
    assert th.dtype == F and th.size == 17 > 15 and th[0] == 0 and th[1] == F(np.pi / 2) and th[6] > th[2] and th[6] - th[2] < 1e-6
    assert len(set(tw.SUBSET)) < len(tw.SUBSET) and list(tw.SUBSET) != sorted(tw.SUBSET) and max(tw.SUBSET) < th.size
    assert [tw.detector(g) for g in tw.GRIDS] == [200, 59, 200, 200]
    x, y, w = tw.images(3, (12, 70), 1), tw.sinograms(3, 17, 200, 2), tw.weights((17, 200), 3)
    assert (x[1] == 0).all() and (x[0] < 0).any() and (x[0] > 0).any() and (y[:, tw.ZERO_ANGLE] == 0).all() and (y[0, 0] != 0).any()
    assert (w == 0).sum() == -(-w.size // 7) and (w >= 0).all()
    assert (tw.images(3, (12, 70), 1, positive=True)[[0, 2]] > 0).all()


def test_float32_stores_are_correctly_rounded_in_the_kernels_order():
    rng = np.random.default_rng(0)
    sim, meas, p = (rng.standard_normal((3, 17, 40)).astype(F) for _ in range(3))
    sim[0, :4] = 0.0
    w = tw.weights((17, 40), 1)
    s, m, pp, ww = sim.astype(D), meas.astype(D), p.astype(D), w.astype(D)
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(tw.sirt_update(sim, meas, w), np.where(ww != 0, r32(r32(m - s) / ww), 0.0).astype(F))
        np.testing.assert_array_equal(tw.ratio(sim, meas), np.where(s != 0, r32(m / s), 0.0).astype(F))
        np.testing.assert_array_equal(tw.tv_dual(p, sim, meas, w), r32(r32(pp + r32(ww * r32(s - m))) / r32(1.0 + ww)).astype(F))
        x, bp = (rng.standard_normal((3, 9, 11)).astype(F) for _ in range(2))
        cs = tw.weights((9, 11), 2)
        xd, bd, cd = x.astype(D), bp.astype(D), cs.astype(D)
        np.testing.assert_array_equal(tw.sirt_add(x, bp, cs), np.where(cd != 0, r32(xd + r32(bd / cd)), xd).astype(F))
        np.testing.assert_array_equal(tw.multiply(x, bp, cs), np.where(cd != 0, r32(xd * r32(bd / cd)), xd).astype(F))
    sc = rng.uniform(0.5, 2.0, 3).astype(F)
    np.testing.assert_array_equal(tw.scaled(bp, sc), r32(sc.astype(D)[:, None, None] * bd).astype(F))
    np.testing.assert_array_equal(tw.scaled(bp, sc[:1]), r32(D(sc[0]) * bd).astype(F))
    assert tw.scaled(bp) is not None and np.array_equal(tw.scaled(bp), bp)
    # the guards: exactly 0 where the weight or the ray-sum is, the image's own bits where the column sum is
    assert (tw.sirt_update(sim, meas, w)[:, w == 0] == 0).all() and (tw.ratio(sim, meas)[sim == 0] == 0).all()
    assert np.array_equal(tw.sirt_add(x, bp, cs)[:, cs == 0], x[:, cs == 0]) and np.array_equal(tw.multiply(x, bp, cs)[:, cs == 0], x[:, cs == 0])


@pytest.mark.parametrize("grid", SMALL)
def test_one_iteration_from_the_pieces_is_the_restatements(oracle, grid):
    gx, gy = grid
    dx, th = tw.detector(grid), tw.angles()
    data = tw.sinograms(3, th.size, dx, 5, positive=True)
    x0 = np.full((3, gx, gy), 1e-6, F)
    ones = np.ones((1, th.size, dx), F)
    for sub in (None, list(tw.SUBSET)):
        t = th if sub is None else np.ascontiguousarray(th[sub])
        y = data if sub is None else np.ascontiguousarray(data[:, sub])
        cs = tw.backproject(ones[:, :t.size], t, gx, gy)[0]
        bp = tw.backproject(tw.ratio(tw.raysums(x0, t, dx), y), t, gx, gy)
        np.testing.assert_array_equal(tw.multiply(x0, bp, cs), tm.mlem(y, t, 1, ngridx=gx, ngridy=gy))
        np.testing.assert_array_equal(tp.update(x0, bp, cs, 0.3), tp.pml(y, t, 1, beta=0.3, ngridx=gx, ngridy=gy))
        np.testing.assert_array_equal(tw.recon("mlem", y, t, 1, gx, gy), tm.mlem(y, t, 1, ngridx=gx, ngridy=gy))
        np.testing.assert_array_equal(tw.recon("pml_quad", y, t, 1, gx, gy, reg_par=[0.3]), tp.pml(y, t, 1, beta=0.3, ngridx=gx, ngridy=gy))
    # an osem block is an mlem iteration on the block's angles
    blocks = tm.blocks_of(th.size, 3)
    x = x0
    for b in blocks:
        t, y = np.ascontiguousarray(th[b]), np.ascontiguousarray(data[:, b])
        cs = tw.backproject(ones[:, :t.size], t, gx, gy)[0]
        x = tw.multiply(x, tw.backproject(tw.ratio(tw.raysums(x, t, dx), y), t, gx, gy), cs)
    np.testing.assert_array_equal(x, tw.recon("osem", data, th, 1, gx, gy, num_block=3))
    # the TV stand-in from a constant start: grad xbar = 0, so q stays 0 and the first primal step is x - tau A^T p
    rowsum = tw.raysums(np.ones((1, gx, gy), F), th, dx)[0]
    with np.errstate(divide="ignore"):
        sigma = np.where(rowsum > 0, F(1.0) / np.maximum(rowsum, F(1e-30)), F(0.0)).astype(F)
    tau = F(1.0) / (tw.backproject(ones, th, gx, gy)[0] + F(4.0))
    p1 = tw.tv_dual(np.zeros_like(data), tw.raysums(x0, th, dx), data, sigma)
    np.testing.assert_array_equal((x0 - tau * (tw.backproject(p1, th, gx, gy) - F(0.0))).astype(F), tw.recon("tv", data, th, 1, gx, gy))


@pytest.mark.parametrize("grid", SMALL)
def test_the_gaussian_cell_of_the_twin_is_consistent(oracle, grid):
    """The oracle's float32 log-probability and the float32 twins lie inside the bars the device is held to."""
    th = tw.angles()
    dx = tw.detector(grid)
    sim = tw.raysums(tw.images(3, grid, 8, positive=True), th, dx)
    rng = np.random.default_rng(9)
    mask = rng.choice(np.asarray(tg.MASKS, F), size=(3, th.size)).astype(F)
    meas = (rng.poisson(sim.astype(D) * mask[..., None] * 1e4) / 1e4).astype(F)
    g = tw.gauss(sim, mask, meas, 1e4, 1.2e-7)
    e, same = tw.gauss_excess(g["lp_oracle"], g["lp_ref"], g["lp_bar"])
    assert same and e <= 1.0
    e, same = tw.gauss_excess(tg.twin_dlogp(sim, mask, meas, 1e4, 1.2e-7), g["dlp_ref"], g["dlp_bar"])
    assert same and e <= 1.0
    want, atol, rtol = tw.poisson(sim, mask, meas, 1e4)
    from tests import np_twin_poisson as tpo
    e, same = tw.poisson_excess(tpo.twin_logp(sim, mask, meas, 1e4), want, atol, rtol)
    assert same and e <= 1.0
