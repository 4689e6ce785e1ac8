"""iradon on the device (ct_pvae_amd/fbp.py, csrc/fbp.hip) and its gradient against the float64 twin of tests/np_twin_fbp.py, in
the reference's geometry AND in tomopy_geometry=True (which the oracle cannot judge: it has no geometry parameters), at the shapes
where each kernel takes another path: the filter loop's second trip, both back-projection variants and the switch between them,
ragged pixel blocks, the backward's slice groups and bin blocks.  Then recon('fbp', 'ramp'), the input forms, the table cache, a
side stream, the refusals and the empty batch.

The bar is the project's standing one for the fp64 FBP (tests/test_gpu_parity.py: convolution against DFT ordering):
max |got - twin| <= 1e-10 max |twin|, forward and gradient; adjointness to 1e-11; every output finite (outputs start as NaN in a
test session); a second call gives the same bits.  Measured on the MI355X: see README.md."""
import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib, fbp, forward_functions
from ct_pvae_amd.recon import recon
from tests import np_twin_fbp as tw

pytestmark = pytest.mark.gpu

BAR = 1e-10


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


def on_dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))                                         # (a copy: the shared references stay untouched)
    return (t if dtype is None else t.to(dtype)).to(dev())


def call(ref, sino, **kw):
    """iradon with the case's angles, grid, filter and geometry; keywords replace an operand."""
    theta = kw.pop("theta", None)
    filt = kw.pop("filt", None)
    assert not kw
    return fbp.iradon(sino, ref["theta"].copy() if theta is None else theta, ref["X"], ref["Y"],
                      ref["filt"].copy() if filt is None else filt, tomopy_geometry=ref["kind"] == tw.TOMOPY)


def forward_and_gradient(ref, sino, g):
    s = sino.detach().clone().requires_grad_(True)
    out = call(ref, s)
    out.backward(g)
    return out.detach(), s.grad


@pytest.mark.parametrize("name,kind", tw.PAIRS)
def test_forward_against_the_twin(name, kind):
    assert forward_functions.POISON_OUTPUTS                                   # an element no launch writes reads NaN
    ref = tw.reference(name, kind)
    s = on_dev(ref["sino"])
    got = call(ref, s)
    assert got.dtype is torch.float64 and tuple(got.shape) == ref["want"].shape and got.grad_fn is None
    assert bool(torch.isfinite(got).all())
    e = tw.err(to_np(got), ref["want"])
    print(f"fbp forward {name} {kind}: err {e:.3e} = {e / BAR:.2e} of the bar, max|twin| {np.abs(ref['want']).max():.3f}")
    assert e <= BAR
    assert torch.equal(call(ref, s), got)


@pytest.mark.parametrize("name,kind", tw.GRAD_PAIRS)
def test_gradient_against_the_twin(name, kind):
    """grad = M g for the twin's dense matrix; <iradon(s), g> = <s, grad>; a float32 sinogram's gradient is the float64 one
    rounded once (iradon is linear: the gradient does not depend on the sinogram)."""
    ref = tw.reference(name, kind)
    s, g = on_dev(ref["sino"]), on_dev(ref["g"])
    out, grad = forward_and_gradient(ref, s, g)
    assert grad.dtype is torch.float64 and tuple(grad.shape) == ref["gwant"].shape and bool(torch.isfinite(grad).all())
    e_out, e = tw.err(to_np(out), ref["want"]), tw.err(to_np(grad), ref["gwant"])
    lhs, rhs = float((to_np(out) * ref["g"]).sum()), float((ref["sino"] * to_np(grad)).sum())
    adj = abs(lhs - rhs) / max(abs(lhs), 1.0)
    print(f"fbp gradient {name} {kind}: err {e:.3e} = {e / BAR:.2e} of the bar, adjointness {adj:.2e}")
    assert e_out <= BAR and e <= BAR and adj <= 1e-11
    out2, grad2 = forward_and_gradient(ref, s, g)
    assert torch.equal(out2, out) and torch.equal(grad2, grad)
    out32, grad32 = forward_and_gradient(ref, s.to(torch.float32), g)
    assert out32.dtype is torch.float64 and grad32.dtype is torch.float32 and torch.equal(grad32, grad.to(torch.float32))


@pytest.mark.parametrize("kind", tw.BOTH)
@pytest.mark.parametrize("name", ["nb2", "nb1", "b9", "b17"])
def test_a_sinogram_does_not_depend_on_its_batch(name, kind):
    """The first, a middle and the last sinogram of a batch -- alone in a pair or a slice group, or sharing it -- give the bits of
    a call of their own, forward and gradient; nb2's first 59 sinograms are nb1's."""
    ref = tw.reference(name, kind)
    s, g = on_dev(ref["sino"]), on_dev(ref["g"])
    out, grad = forward_and_gradient(ref, s, g)
    for b in (0, ref["B"] // 2, ref["B"] - 1):
        out1, grad1 = forward_and_gradient(ref, s[b:b + 1], g[b:b + 1])
        assert torch.equal(out1[0], out[b]) and torch.equal(grad1[0], grad[b]), b
    if name == "nb2":
        out59, grad59 = forward_and_gradient(tw.reference("nb1", kind), s[:59], g[:59])
        assert torch.equal(out59, out[:59]) and torch.equal(grad59, grad[:59])
        assert np.array_equal(tw.reference("nb1", kind)["sino"], ref["sino"][:59])


@pytest.mark.parametrize("dx,grid", [(30, (24, 30)), (13, None)])
def test_recon_fbp_ramp_against_the_twin(dx, grid):
    """recon(algorithm='fbp', filter_name='ramp'): float32 data -> the twin in tomopy geometry with ramp_filter(dx) on the data
    widened to float64, rounded once to float32: |got - want| <= 2^-23 |want| + 1e-10 max |want| per element.  dx = 13: an odd
    width is not what ramp_filter's docstring speaks of, but the same taps make a sound filter there (tests/test_fbp_cpu.py), so
    recon serves it and is held to the twin like any other."""
    rng = np.random.default_rng(dx)
    theta = tw.make_theta("special", 6, rng)
    data = rng.random((3, 6, dx), dtype=np.float32)
    gx, gy = grid if grid else (dx, dx)
    want = tw.iradon(data.astype(np.float64), theta, gx, gy, tw.ramp_filter(dx), tw.tomopy(gx, gy, dx))
    got = recon(on_dev(data), theta.copy(), center=None, sinogram_order=True, algorithm="fbp", filter_name="ramp",
                num_gridx=grid[0] if grid else None, num_gridy=grid[1] if grid else None)
    assert got.dtype is torch.float32 and tuple(got.shape) == (3, gx, gy) and bool(torch.isfinite(got).all())
    excess = np.abs(to_np(got).astype(np.float64) - want) - 2.0 ** -23 * np.abs(want)
    print(f"recon fbp/ramp dx {dx}: worst excess over one float32 rounding {excess.max() / np.abs(want).max():.2e} of max|want| (bar 1e-10)")
    assert (excess <= BAR * np.abs(want).max()).all()
    by_angle = recon(on_dev(np.ascontiguousarray(data.transpose(1, 0, 2))), theta.copy(), algorithm="fbp", filter_name="ramp",
                     num_gridx=gx, num_gridy=gy)                              # projection order [angles][slices][dx]
    assert torch.equal(by_angle, got)


@pytest.mark.parametrize("kind", tw.BOTH)
def test_input_forms_give_the_plain_calls_bits(kind):
    """Observed on the MI355X: every form below is bit-equal, the angles given as a device tensor included (the host path also takes
    cos / sin on the device, of the same float64 values)."""
    ref = tw.reference("wide", kind)
    d = dev()
    s = on_dev(ref["sino"])
    plain = call(ref, s)
    assert tw.err(to_np(plain), ref["want"]) <= BAR
    # a permuted view of other strides
    view = s.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert not view.is_contiguous() and torch.equal(view, s)
    assert torch.equal(call(ref, view), plain)
    # float32 sinogram = its float64 widening
    s32 = s.to(torch.float32)
    wide32 = call(ref, s32)
    assert wide32.dtype is torch.float64 and torch.equal(wide32, call(ref, s32.to(torch.float64)))
    # theta as a list, a float32 array, a device tensor, a host tensor
    assert torch.equal(call(ref, s, theta=ref["theta"].tolist()), plain)
    th32 = ref["theta"].astype(np.float32)
    got32 = call(ref, s, theta=th32)
    assert torch.equal(got32, call(ref, s, theta=th32.astype(np.float64)))
    assert tw.err(to_np(got32), tw.iradon(ref["sino"], th32.astype(np.float64), ref["X"], ref["Y"], ref["filt"], ref["geom"])) <= BAR
    on_device = call(ref, s, theta=on_dev(ref["theta"]))
    same = torch.equal(on_device, plain)
    print(f"fbp input forms {kind}: theta as a device tensor {'equals the plain call bit for bit' if same else 'differs in bits'}, "
          f"err {tw.err(to_np(on_device), ref['want']):.2e}")
    assert tw.err(to_np(on_device), ref["want"]) <= BAR
    assert same
    assert torch.equal(call(ref, s, theta=torch.from_numpy(ref["theta"].copy())), plain)
    assert torch.equal(call(ref, s, theta=on_dev(th32)), got32)
    # the filter as a tensor (host and device) and in single precision (complex64 here; a real float32 one as well)
    assert torch.equal(call(ref, s, filt=torch.from_numpy(ref["filt"].copy())), plain)
    assert torch.equal(call(ref, s, filt=on_dev(ref["filt"])), plain)
    f64c = ref["filt"].astype(np.complex64)
    assert torch.equal(call(ref, s, filt=f64c), call(ref, s, filt=f64c.astype(np.complex128)))
    f32 = (np.abs(np.fft.fftfreq(ref["P"])) * 2).astype(np.float32)
    got_f32 = call(ref, s, filt=f32)
    assert torch.equal(got_f32, call(ref, s, filt=f32.astype(np.float64))) and torch.equal(got_f32, call(ref, s, filt=torch.from_numpy(f32).to(d)))
    assert tw.err(to_np(got_f32), tw.iradon(ref["sino"], ref["theta"], ref["X"], ref["Y"], f32.astype(np.float64), ref["geom"])) <= BAR
    # no gradient wanted: no graph
    sg = s.clone().requires_grad_(True)
    with torch.no_grad():
        quiet = call(ref, sg)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, plain)
    assert call(ref, sg).grad_fn is not None


def test_the_table_cache_evicts_and_rebuilds():
    """40 filters x 40 angle sets through a store of 32 entries (two per forward call, three with a gradient): the store never
    grows past 32, and the first calls -- their tables long evicted -- come back with the bits they had."""
    ref = tw.reference("odd", tw.TOMOPY)
    rng = np.random.default_rng(40)
    s, g = on_dev(ref["sino"][:1]), on_dev(ref["g"][:1])
    thetas = [tw.make_theta("random", ref["A"], rng) for _ in range(40)]
    filts = [tw.make_filter("complex", ref["P"], rng) for _ in range(40)]
    fbp._CACHE.clear()

    def one(i):
        if i % 4 == 0:
            sg = s.clone().requires_grad_(True)
            out = call(ref, sg, theta=thetas[i].copy(), filt=filts[i].copy())
            out.backward(g)
            return out.detach(), sg.grad
        return call(ref, s, theta=thetas[i].copy(), filt=filts[i].copy()), None

    first = []
    for i in range(40):
        first.append(one(i))
        assert 0 < len(fbp._CACHE) <= fbp._CACHE_MAX == 32, i
    assert len(fbp._CACHE) == 32                                              # 90 tables were made: the store did evict
    for i in (0, 1, 2, 3, 4, 39, 20):
        out, grad = one(i)
        assert len(fbp._CACHE) <= 32
        assert torch.equal(out, first[i][0]) and (grad is None or torch.equal(grad, first[i][1])), i
    for i in (0, 5, 39):
        want = tw.iradon(ref["sino"][:1], thetas[i], ref["X"], ref["Y"], filts[i], ref["geom"])
        assert tw.err(to_np(first[i][0]), want) <= BAR, i


@pytest.mark.parametrize("kind", tw.BOTH)
def test_a_side_stream_gives_the_default_streams_bits(kind):
    ref = tw.reference("wide", kind)
    s, g = on_dev(ref["sino"]), on_dev(ref["g"])
    out, grad = forward_and_gradient(ref, s, g)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out_s, grad_s = forward_and_gradient(ref, s, g)
        side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(out_s, out) and torch.equal(grad_s, grad)
    assert tw.err(to_np(out_s), ref["want"]) <= BAR and tw.err(to_np(grad_s), ref["gwant"]) <= BAR


def test_refusals_and_limits():
    """Every refusal is a host-side check that comes before a launch.  P = 4096 fills the filter kernel's 64 KiB of LDS and is
    accepted (test_forward_against_the_twin[pmax-ref] holds it to the bar); one more bin is refused."""
    d = dev()
    with pytest.raises(_lib.RadonLibraryError, match="4097 detector bins"):
        fbp.iradon(torch.zeros((1, 1, 4097), dtype=torch.float64, device=d), [0.3], 4, 4, np.ones(4097))
    big = tw.reference("pmax", tw.REF)
    assert tw.err(to_np(call(big, on_dev(big["sino"]))), big["want"]) <= BAR
    with pytest.raises(ValueError, match="at least 2"):
        fbp.iradon(torch.zeros((1, 2, 1), dtype=torch.float64, device=d), [0.3, 0.4], 4, 4, np.ones(1))
    s = torch.zeros((2, 3, 12), dtype=torch.float64, device=d)
    with pytest.raises(ValueError, match="does not match the number of projections"):
        fbp.iradon(s, [0.1, 0.2], 4, 4, np.ones(12))
    with pytest.raises(ValueError, match="filter_1d must hold num_proj_pix=12"):
        fbp.iradon(s, [0.1, 0.2, 0.3], 4, 4, np.ones(11))
    with pytest.raises(ValueError, match="batch x angles x num_proj_pix"):
        fbp.iradon(s[0], [0.1, 0.2, 0.3], 4, 4, np.ones(12))
    with pytest.raises(_lib.RadonLibraryError, match="no CPU path"):
        fbp.iradon(s.cpu(), [0.1, 0.2, 0.3], 4, 4, np.ones(12))


def test_more_angles_than_a_grid_dimension():
    """A = 65536: the forward has no grid dimension over angles and matches the twin; the backward indexes angles with blockIdx.y
    and says so instead of launching."""
    rng = np.random.default_rng(65536)
    A = 65536
    theta = rng.uniform(-1.0, 7.0, A)
    sino = rng.random((1, A, 2))
    filt = np.array([1.0, 0.5])                                               # filtered = 0.75 s[n] + 0.25 s[1 - n] > 0: a sum without cancellation
    want = tw.iradon(sino, theta, 1, 1, filt)
    s = on_dev(sino).requires_grad_(True)
    out = fbp.iradon(s, theta, 1, 1, filt)
    e = tw.err(to_np(out), want)
    print(f"fbp forward, 65536 angles: err {e:.3e}")
    assert tuple(out.shape) == (1, 1, 1) and e <= BAR
    with pytest.raises(ValueError, match="exceeds the grid"):
        out.sum().backward()
    assert s.grad is None


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tomopy_geometry", [False, True])
def test_an_empty_batch_is_an_empty_result(dtype, tomopy_geometry):
    d = dev()
    theta, filt = np.array([0.1, 0.7, 2.0]), np.ones(12) * (1 + 0.5j)        # (tables nothing else in the session has made)
    before = dict(fbp._CACHE)
    out = fbp.iradon(torch.empty((0, 3, 12), dtype=dtype, device=d), theta, 5, 7, filt, tomopy_geometry=tomopy_geometry)
    assert tuple(out.shape) == (0, 5, 7) and out.dtype is torch.float64 and out.device.type == "cuda" and out.grad_fn is None
    s = torch.empty((0, 3, 12), dtype=dtype, device=d, requires_grad=True)
    out = fbp.iradon(s, theta, 5, 7, filt, tomopy_geometry=tomopy_geometry)
    assert tuple(out.shape) == (0, 5, 7) and out.dtype is torch.float64
    out.sum().backward()
    assert tuple(s.grad.shape) == (0, 3, 12) and s.grad.dtype is dtype
    assert fbp._CACHE.keys() == before.keys()                                 # no table was built for it
    with pytest.raises(ValueError, match="does not match the number of projections"):
        fbp.iradon(torch.empty((0, 3, 12), dtype=dtype, device=d), theta[:2], 5, 7, filt)
