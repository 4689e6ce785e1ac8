"""The float64 twin of iradon (ct_pvae_amd/fbp.py, csrc/fbp.hip) and of its gradient: numpy only -- no oracle, no torch.

Written from the reference's own formulation (ctvae/fbp_tensorflow.py:49-74): filter in the Fourier domain, fft -> multiply ->
ifft -> real part; a pixel's detector coordinate t = ypr cos(theta) - xpr sin(theta) on an 'ij' meshgrid; linear interpolation
of the filtered row at t with constant extension beyond the detector (np.interp does exactly that); the angles summed in
ascending order; the sum scaled by pi / (2 A).  The kernel computes the same numbers another way -- a circular convolution with
Re(ifft(filter_1d)) out of LDS and tfp's clipped-index arithmetic (floor, above, below) -- and so does the C oracle; the twin
shares neither, and it takes the geometry (x0, y0, t0) as a parameter, which the oracle does not.

    geom = (x0, y0, t0): pixel (i, j) sits at (i - x0, j - y0), detector sample k at k - t0.
    default      (X / 2, Y / 2, P / 2)                          the reference's iradon
    tomopy()     ((X - 1) / 2, (Y - 1) / 2, (P - 1) / 2)        iradon(..., tomopy_geometry=True), what recon('fbp', 'ramp') uses

CASES: each the smallest shape that reaches the path its comment names, shared by tests/test_fbp_cpu.py and
tests/test_gpu_fbp.py through case(name), which builds the same operands from a fixed seed wherever it is called."""
import zlib

import numpy as np

SPECIAL = np.array([0.0, np.pi / 2, np.pi])          # pixels land exactly on bins and on x_min / x_max

REF, TOMOPY = "ref", "tomopy"
BOTH = (REF, TOMOPY)


def tomopy(X, Y, P):
    return ((X - 1) / 2.0, (Y - 1) / 2.0, (P - 1) / 2.0)


def geom_of(kind, X, Y, P):
    return tomopy(X, Y, P) if kind == TOMOPY else (X / 2.0, Y / 2.0, P / 2.0)


def ramp_filter(P):
    """2 Re(fft(h)), h the band-limited ramp's taps: h[0] = 1/4, h[k] = -1 / (pi n)^2 at odd circular distance n = min(k, P - k),
    0 elsewhere (the formula ct_pvae_amd.fbp.ramp_filter documents; tests/test_fbp_cpu.py holds the two to the same bits)."""
    k = np.arange(P)
    n = np.minimum(k, P - k)
    h = np.where(n % 2 == 1, -1.0 / (np.pi * np.maximum(n, 1)) ** 2, 0.0)
    h[0] = 0.25
    return 2 * np.real(np.fft.fft(h))


def filtered(sino, filt):
    return np.real(np.fft.ifft(np.fft.fft(np.asarray(sino, np.float64).astype(np.complex128), axis=-1) * np.asarray(filt), axis=-1))


def iradon(sino, theta, X, Y, filt, geom=None):
    """sino [B][A][P] -> [B][X][Y], float64."""
    sino = np.asarray(sino, np.float64)
    theta = np.asarray(theta, np.float64)
    B, A, P = sino.shape
    assert theta.shape == (A,) and np.asarray(filt).shape == (P,)
    x0, y0, t0 = (X / 2.0, Y / 2.0, P / 2.0) if geom is None else geom
    rows = filtered(sino, filt)
    xpr, ypr = np.meshgrid(np.arange(X, dtype=np.float64) - x0, np.arange(Y, dtype=np.float64) - y0, indexing="ij")
    bins = np.arange(P, dtype=np.float64) - t0
    out = np.zeros((B, X, Y))
    for a in range(A):
        t = ypr * np.cos(theta[a]) - xpr * np.sin(theta[a])
        for b in range(B):
            out[b] += np.interp(t, bins, rows[b, a])
    return out * np.pi / (2 * A)


def matrix(theta, A, P, X, Y, filt, geom=None):
    """The dense (A P) x (X Y) operator M with iradon(s) = M^T s, row by row from unit sinograms through iradon."""
    return iradon(np.eye(A * P).reshape(A * P, A, P), theta, X, Y, filt, geom).reshape(A * P, X * Y)


def grad(g, theta, A, P, X, Y, filt, geom=None, M=None):
    """d <iradon(s), g> / d s = M g: g [B][X][Y] -> [B][A][P]."""
    g = np.asarray(g, np.float64)
    M = matrix(theta, A, P, X, Y, filt, geom) if M is None else M
    return (M @ g.reshape(g.shape[0], X * Y).T).T.reshape(g.shape[0], A, P)


def err(got, want):
    """max |got - want| over max |want|: the project's rel_err."""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


# name: (B, A, P, X, Y, geometries, filter kind, angle set, seed name)
# filter kinds   "ramp" ramp_filter(P) (even P), "freq" |fftfreq| * 2, "complex" random complex (the transposed kernel is not symmetric)
# angle sets     "special" 0, pi/2, pi then uniform(-1, 7); "half" pi/2 then uniform(-1, 7); "random" uniform(-1, 7) alone -- so that a
#                case of two or three angles is not made of exact hits only.  Angles lie outside [0, pi) in every set that draws.
# seed name      cases with the same one draw the same stream: nb1's operands are nb2's first 59 sinograms.
CASES = {
    "p2":           (1, 3, 2, 7, 5, BOTH, "complex", "special", "p2"),         # smallest legal P; every pixel beyond the detector
    "odd":          (3, 4, 13, 16, 16, BOTH, "freq", "special", "odd"),        # odd P; X Y = 256 ends the block exactly
    "blk257_1x257": (1, 3, 24, 1, 257, BOTH, "ramp", "special", "blk257r"),    # one thread in the second block; i = p / Y = 0
    "blk257_257x1": (1, 3, 24, 257, 1, BOTH, "ramp", "special", "blk257c"),    # ... and j = 0 throughout
    "wide":         (2, 5, 12, 31, 29, BOTH, "complex", "special", "wide"),    # X, Y >> P: both clamps on most pixels; odd X, Y
    "p257":         (1, 3, 257, 16, 17, BOTH, "freq", "random", "p257"),       # second trip of the filter loop, one lane of it live
    "p300":         (2, 2, 300, 17, 19, BOTH, "ramp", "half", "p300"),         # ... 44 lanes; backward blockIdx.x to 4, idle tail
    "p64":          (1, 2, 64, 9, 8, BOTH, "ramp", "random", "p64"),           # backward: last block full
    "p65":          (1, 2, 65, 9, 8, BOTH, "complex", "half", "p65"),          # backward: one live lane in the last block
    "b8":           (8, 2, 12, 9, 8, BOTH, "complex", "random", "b8"),         # backward slice groups: one full
    "b9":           (9, 2, 12, 9, 8, BOTH, "ramp", "half", "b9"),              # ... full + a ragged one of 1
    "b17":          (17, 2, 12, 9, 8, BOTH, "freq", "special", "b17"),         # ... blockIdx.z = 2
    "nb2":          (61, 3, 24, 64, 65, BOTH, "complex", "half", "nb"),        # 17 cells x 31 = 527 >= 512: NB = 2, ragged last pair
    "nb1":          (59, 3, 24, 64, 65, BOTH, "complex", "half", "nb"),        # 17 x 30 = 510 < 512: NB = 1 on the same grid
    "pmax":         (1, 1, 4096, 4, 4, (REF,), "freq", "special", "pmax"),     # the largest P the LDS check admits; angle 0 alone
}
GRAD_CASES = [n for n in CASES if n != "pmax"]
PAIRS = [(n, k) for n, c in CASES.items() for k in c[5]]
GRAD_PAIRS = [(n, k) for n, k in PAIRS if n != "pmax"]


def make_theta(kind, A, rng):
    lead = {"special": SPECIAL, "half": SPECIAL[1:2], "random": SPECIAL[:0]}[kind][:A]
    return np.concatenate([lead, rng.uniform(-1.0, 7.0, A - lead.size)])


def make_filter(kind, P, rng):
    if kind == "ramp":
        assert P % 2 == 0
        return ramp_filter(P)
    if kind == "freq":
        return np.abs(np.fft.fftfreq(P)) * 2
    assert kind == "complex"
    return rng.standard_normal(P) + 1j * rng.standard_normal(P)


def _seed(tag):
    return zlib.crc32(tag.encode())


def case(name):
    """The operands of a case: sino [B][A][P], g [B][X][Y] (the cotangent of the gradient tests), theta, filt -- fresh arrays,
    the same values at every call."""
    B, A, P, X, Y, geoms, fkind, akind, seed = CASES[name]
    rng = np.random.default_rng(_seed(seed))
    theta = make_theta(akind, A, rng)
    filt = make_filter(fkind, P, rng)
    sino = np.random.default_rng(_seed(seed + "/sino")).standard_normal((B, A, P))
    g = np.random.default_rng(_seed(seed + "/g")).standard_normal((B, X, Y))
    return dict(name=name, B=B, A=A, P=P, X=X, Y=Y, geoms=geoms, theta=theta, filt=filt, sino=sino, g=g)


_REFS = {}


def reference(name, kind):
    """case(name) with the twin's forward ("want"), and for the gradient cases M and M g ("gwant"), computed once per session
    and geometry; callers leave the arrays as they are."""
    key = (name, kind)
    if key not in _REFS:
        c = case(name)
        geom = geom_of(kind, c["X"], c["Y"], c["P"])
        c.update(kind=kind, geom=geom, want=iradon(c["sino"], c["theta"], c["X"], c["Y"], c["filt"], geom))
        if name in GRAD_CASES:
            c["M"] = matrix(c["theta"], c["A"], c["P"], c["X"], c["Y"], c["filt"], geom)
            c["gwant"] = grad(c["g"], c["theta"], c["A"], c["P"], c["X"], c["Y"], c["filt"], geom, M=c["M"])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = c
    return _REFS[key]
