"""iradon without a GPU: the float64 twin of tests/np_twin_fbp.py is checked before it judges the kernels (tests/test_gpu_fbp.py)
-- against the C oracle in the reference's geometry, against answers worked out by hand in both geometries, and, for the claim in
iradon's docstring that tomopy_geometry is the right one for tomopy.project's sinograms, by where a reconstructed disc lands."""
import numpy as np
import pytest

from tests import np_twin_fbp as tw


def test_the_case_table_holds_what_it_must():
    """The shapes the GPU file relies on (a case edited away would otherwise go unnoticed), restated from csrc/fbp.hip: 256 pixels
    per forward block, two sinograms per thread once cells * ceil(B / 2) >= 512, 64 bins per backward block, 8 sinograms per
    backward thread, 256 lanes per filter row, 2 * P * 8 bytes of LDS <= 64 KiB."""
    C = tw.CASES
    shape = {n: c[:5] for n, c in C.items()}
    assert shape["p2"] == (1, 3, 2, 7, 5) and shape["odd"] == (3, 4, 13, 16, 16) and 16 * 16 == 256
    assert shape["blk257_1x257"] == (1, 3, 24, 1, 257) and shape["blk257_257x1"] == (1, 3, 24, 257, 1)
    assert shape["wide"] == (2, 5, 12, 31, 29)
    assert shape["p257"] == (1, 3, 257, 16, 17) and shape["p300"] == (2, 2, 300, 17, 19) and -(-300 // 64) == 5 and 300 % 64
    assert shape["p64"] == (1, 2, 64, 9, 8) and shape["p65"] == (1, 2, 65, 9, 8)
    assert [shape[n] for n in ("b8", "b9", "b17")] == [(b, 2, 12, 9, 8) for b in (8, 9, 17)] and -(-17 // 8) == 3
    assert shape["nb2"] == (61, 3, 24, 64, 65) and shape["nb1"] == (59, 3, 24, 64, 65)
    cells = -(-64 * 65 // 256)
    assert cells * -(-61 // 2) == 527 >= 512 > 510 == cells * -(-59 // 2) and 61 % 2 == 1
    assert shape["pmax"] == (1, 1, 4096, 4, 4) and 2 * 4096 * 8 == 64 * 1024 and C["pmax"][5] == (tw.REF,)
    assert all(c[5] == tw.BOTH for n, c in C.items() if n != "pmax")
    assert {c[6] for c in C.values()} == {"ramp", "freq", "complex"} and all(c[2] % 2 == 0 for c in C.values() if c[6] == "ramp")
    th = tw.case("wide")["theta"]
    assert np.array_equal(th[:3], [0.0, np.pi / 2, np.pi]) and ((th[3:] >= -1) & (th[3:] < 7)).all()
    drawn = np.concatenate([tw.case(n)["theta"][{"special": 3, "half": 1, "random": 0}[c[7]]:] for n, c in C.items()])
    assert drawn.min() < 0 and drawn.max() > np.pi and drawn.size >= 16
    nb1, nb2 = tw.case("nb1"), tw.case("nb2")                      # nb1 IS nb2's first 59 sinograms
    assert np.array_equal(nb1["sino"], nb2["sino"][:59]) and np.array_equal(nb1["g"], nb2["g"][:59])
    assert np.array_equal(nb1["theta"], nb2["theta"]) and np.array_equal(nb1["filt"], nb2["filt"])
    again = tw.case("wide")
    assert all(np.array_equal(again[k], tw.case("wide")[k]) for k in ("sino", "g", "theta", "filt"))


@pytest.mark.parametrize("name", list(tw.CASES))
def test_twin_against_the_oracle(oracle, name):
    """Reference geometry, every case: within 1e-13 of the largest value.  Measured 2e-16 to 8e-15 up to P = 65, 2.2e-14 at
    P = 257 and 6.3e-14 at P = 300: the difference is the ORACLE's (and the reference's, and the kernel's) index arithmetic
    idx = t + P / 2, which rounds the position to ulp(P / 2) before it takes the fraction, where np.interp subtracts the bin's
    coordinate from t directly -- so it grows with P.  (pmax, P = 4096, measures 3e-15 at its angle 0, where idx is a whole number;
    at an angle drawn from uniform(-1, 7) the same case reads 3.8e-13 = ulp(2048) times the filtered row's slope.  Against an
    80-bit DFT of the same rows the twin's filter is within 5e-16 and the oracle's O(P^2) sums within 4.4e-15.)"""
    ref = tw.reference(name, tw.REF)
    got = oracle.iradon(ref["sino"], ref["theta"], ref["X"], ref["Y"], ref["filt"])
    e = tw.err(ref["want"], got)
    print(f"fbp twin vs oracle {name}: {e:.2e} of max|oracle| = {np.abs(got).max():.3f}")
    assert ref["want"].shape == got.shape == (ref["B"], ref["X"], ref["Y"]) and np.isfinite(ref["want"]).all()
    assert e <= 1e-13


@pytest.mark.parametrize("name,kind", tw.PAIRS)
def test_twin_is_linear_and_its_matrix_is_its_transpose(name, kind):
    """iradon(s) = M^T s for the matrix built from unit sinograms, iradon(a s1 + b s2) = a iradon(s1) + b iradon(s2), and
    <iradon(s), g> = <s, M g>, to 1e-12 (pmax: linearity alone -- its matrix is never needed)."""
    ref = tw.reference(name, kind)
    X, Y, s = ref["X"], ref["Y"], ref["sino"]
    other = np.random.default_rng(3).standard_normal(s.shape)
    mix = tw.iradon(0.5 * s - 4.0 * other, ref["theta"], X, Y, ref["filt"], ref["geom"])
    assert tw.err(mix, 0.5 * ref["want"] - 4.0 * tw.iradon(other, ref["theta"], X, Y, ref["filt"], ref["geom"])) <= 1e-12
    if name not in tw.GRAD_CASES:
        return
    M = ref["M"]
    assert M.shape == (ref["A"] * ref["P"], X * Y)
    assert tw.err((s.reshape(ref["B"], -1) @ M).reshape(ref["want"].shape), ref["want"]) <= 1e-12
    lhs, rhs = float((ref["want"] * ref["g"]).sum()), float((s * ref["gwant"]).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_tomopy_geometry_by_hand():
    """Known answers.  tomopy() is the default geometry moved by exactly half a pixel in x and y and half a bin.  With an identity
    filter (ones(P)) and one angle the twin is interpolation alone, idx = t + t0, scaled by pi / 2:

      theta = 0:     t = j - y0.  X = Y = P: idx = j in BOTH geometries (the half pixel and the half bin cancel), so every row of the
                     image is the sinogram row along j.  Y = P - 1: idx = j + 1/2 in both again -- midpoints (s[j] + s[j + 1]) / 2:
                     at this angle the two cannot differ, whatever Y.
      theta = pi/2:  t = -(i - x0).  tomopy: idx = P - 1 - i, column i holds s[P - 1 - i]: the row reversed, all of it.  Default:
                     idx = P - i, column i holds s[P - i] and column 0 the clamped s[P - 1]: one whole bin off, s[0] never read.
                     Here they differ (idx_default - idx_tomopy = (1 - cos + sin) / 2 in general)."""
    P = 9
    s = np.random.default_rng(0).standard_normal((1, 1, P))
    row = s[0, 0]
    one = np.ones(P)
    assert tw.tomopy(6, 7, P) == (2.5, 3.0, 4.0) and tw.geom_of(tw.TOMOPY, 6, 7, P) == tw.tomopy(6, 7, P)
    assert np.array_equal(np.subtract(tw.geom_of(tw.REF, 6, 7, P), tw.tomopy(6, 7, P)), [0.5, 0.5, 0.5])
    assert tw.geom_of(tw.REF, 6, 7, P) == (3.0, 3.5, 4.5)
    for geom in (None, tw.tomopy(P, P, P)):
        got = tw.iradon(s, [0.0], P, P, one, geom)[0]
        assert np.abs(got - np.pi / 2 * row[None, :]).max() <= 1e-15 * P
    for geom in (None, tw.tomopy(P, P - 1, P)):
        got = tw.iradon(s, [0.0], P, P - 1, one, geom)[0]
        assert np.abs(got - np.pi / 2 * (0.5 * (row[:-1] + row[1:]))[None, :]).max() <= 1e-15 * P
    # cos(pi / 2) = 6e-17, not 0: t is within 4 * 6e-17 of a whole number
    got = tw.iradon(s, [np.pi / 2], P, P, one, tw.tomopy(P, P, P))[0]
    assert np.abs(got - np.pi / 2 * row[::-1][:, None]).max() <= 1e-14
    got = tw.iradon(s, [np.pi / 2], P, P, one)[0]
    want = np.concatenate([row[-1:], row[:0:-1]])                             # s[P - 1], s[P - 1], s[P - 2], ..., s[1]
    assert np.abs(got - np.pi / 2 * want[:, None]).max() <= 1e-14
    assert np.abs(got - np.pi / 2 * row[::-1][:, None]).max() > 0.1


def test_a_half_bin_slip_is_far_outside_the_gpu_bar():
    """A MODEL of the defect, the twin standing in for the kernel: P / 2 for (P - 1) / 2 in the tomopy geometry moves every case by
    0.5 to 1.8 of its largest value -- ten orders above the 1e-10 the GPU tests allow."""
    for name, kind in tw.PAIRS:
        if kind != tw.TOMOPY:
            continue
        ref = tw.reference(name, kind)
        x0, y0, _ = ref["geom"]
        bad = tw.iradon(ref["sino"], ref["theta"], ref["X"], ref["Y"], ref["filt"], (x0, y0, ref["P"] / 2.0))
        assert tw.err(bad, ref["want"]) > 0.1, name


def test_ramp_filter_is_the_packages_and_odd_widths_are_sound():
    """The twin's ramp_filter is ct_pvae_amd.fbp.ramp_filter bit for bit.  Its docstring promises even P; recon('fbp', 'ramp') passes
    the detector width whatever its parity.  At odd P the taps h[k] at odd circular distance are still symmetric (h[k] = h[P - k]),
    so the filter is real; it is 2 |f| everywhere but near f = 0, where it keeps the band-limited ramp's positive value, and that
    value falls steadily through odd and even P alike (0.0335 at 12 and 13, 0.0293 at 14, 0.0252 at 15): an odd width is served by the
    same filter, so recon accepts it and tests/test_gpu_fbp.py holds dx = 13 to the twin."""
    from ct_pvae_amd.fbp import ramp_filter
    dc = []
    for P in (2, 12, 13, 14, 15, 24, 29, 30, 31, 64, 185, 300):
        r = tw.ramp_filter(P)
        assert np.array_equal(r, ramp_filter(P))
        k = np.arange(P)
        n = np.minimum(k, P - k)
        h = np.where(n % 2 == 1, -1.0 / (np.pi * np.maximum(n, 1)) ** 2, 0.0)
        h[0] = 0.25
        assert np.abs(np.fft.fft(h).imag).max() <= 1e-16 and np.allclose(r[1:], r[:0:-1], rtol=0, atol=1e-15)
        if P > 2:
            assert r.min() > 0 and np.abs(r - 2 * np.abs(np.fft.fftfreq(P))).max() <= r[0] * (1 + 1e-12)
        dc.append(r[0])
    assert all(a >= b - 1e-15 for a, b in zip(dc[1:], dc[2:])) and dc[-1] < 0.002


def centroid_offsets(oracle, N, centre, radius, A):
    """A disc whose pixel set is symmetric about `centre` (half-integers), projected by the TomoPy-style projector with padding
    (the object sits npad pixels into the dx x dx grid on every side), reconstructed by the twin with the ramp on that grid;
    the intensity centroid of the values above half the maximum, minus the disc's centre, per geometry."""
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    obj = (((i - centre[0]) ** 2 + (j - centre[1]) ** 2) <= radius ** 2).astype(np.float32)
    assert abs((i * obj).sum() / obj.sum() - centre[0]) < 1e-12 and abs((j * obj).sum() / obj.sum() - centre[1]) < 1e-12
    theta = (np.pi * np.arange(A) / A).astype(np.float32)
    data = oracle.siddon_project(obj[None], theta, pad=True)                 # [dt][1][dx]
    dx = data.shape[2]
    assert (dx - N) % 2 == 0
    npad = (dx - N) // 2
    sino = np.ascontiguousarray(data.transpose(1, 0, 2)).astype(np.float64)
    I, J = np.meshgrid(np.arange(dx), np.arange(dx), indexing="ij")
    out = {}
    for kind in tw.BOTH:
        rec = tw.iradon(sino, theta.astype(np.float64), dx, dx, tw.ramp_filter(dx), tw.geom_of(kind, dx, dx, dx))[0]
        m = np.where(rec > 0.5 * rec.max(), rec, 0.0)
        out[kind] = ((I * m).sum() / m.sum() - (centre[0] + npad), (J * m).sum() / m.sum() - (centre[1] + npad), rec.max())
    return out


def test_a_disc_comes_back_where_it_was_in_the_tomopy_geometry_only(oracle):
    """iradon's docstring: tomopy_geometry is 'the right geometry for sinograms made by create_sinogram / tomopy.project'.  A disc
    of radius 3.3 about (7.5, 14.5) in a 24 x 24 object (36 bins, 45 angles over [0, pi)): measured centroid offsets

        tomopy geometry     (+0.001, -0.002) px      peak 1.036
        reference geometry  (+1.150, +0.376) px      peak 1.045

    (the same to 0.02 px at 90 and 180 angles and for a 32 x 32 object).  The reference geometry is half a pixel off in both axes
    AND half a bin off on the detector, a centre-of-rotation error that smears the disc along an arc -- hence not (0.5, 0.5).  The
    image comes back in the object's own orientation: no flip, no transpose."""
    off = centroid_offsets(oracle, 24, (7.5, 14.5), 3.3, 45)
    for kind, (di, dj, peak) in off.items():
        print(f"fbp centroid, {kind} geometry: offset ({di:+.3f}, {dj:+.3f}) px, peak {peak:.3f}")
    di, dj, peak = off[tw.TOMOPY]
    assert abs(di) < 0.25 and abs(dj) < 0.25 and 0.9 < peak < 1.15
    di, dj, _ = off[tw.REF]
    assert abs(di) > 0.25 or abs(dj) > 0.25
