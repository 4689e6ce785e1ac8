"""gridrec on the device (ct_pvae_amd/csrc/gridrec.hip) against the float64 twin of tests/np_twin_gridrec.py at every padded row
size from 16 to 2048 and against the fp32 oracle, through recon() and through the raw entry points (shifted centres, stale and
offset workspaces), the refusals, the table cache of ct_pvae_amd/recon.py and a side stream.

The rule (np_twin_gridrec): err(got, twin) <= MARGIN max(e_oracle, 2^-23), e_oracle recomputed here on the same operands, and
rel_err(got, oracle) <= REL; a second call gives the same bits; every output is finite."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from ct_pvae_amd import _lib
from ct_pvae_amd.forward_functions import _stream_ptr
from ct_pvae_amd.recon import recon
from tests import np_twin_gridrec as tw

pytestmark = pytest.mark.gpu

CENTRED = [n for n, c in tw.CASES.items() if c[6] == 0.0]
SHIFTED = [n for n, c in tw.CASES.items() if c[6] != 0.0]
STALE = {"dx15": 16, "dx185": 256, "c5_512": 1024}           # one case per padded row size for the workspace checks


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def c5_width():
    return _lib.load().ctpvae_num_proj_pix(512, 512)


def run_recon(ref):
    return recon(torch.from_numpy(ref["data"].copy()).to(dev()), ref["theta"].copy(), center=None, sinogram_order=True,
                 algorithm="gridrec", filter_name=ref["filt"], num_gridx=ref["gx"], num_gridy=ref["gy"])


def device_tables(dt, dx, center, theta, filt, par=tw.BUTTERWORTH_PAR):
    lib = _lib.load()
    nbytes = _lib.check(lib.ctpvae_gridrec_tables_bytes(dt, dx), "gridrec_tables_bytes")
    host = np.empty(int(nbytes), np.uint8)
    par = np.ascontiguousarray(par, np.float32)
    theta = np.ascontiguousarray(theta, np.float32)
    _lib.check(lib.ctpvae_gridrec_tables_host_f32(dt, dx, ctypes.c_float(center), theta.ctypes.data, tw.FILTERS.index(filt),
                                                  par.ctypes.data, host.ctypes.data), "gridrec_tables")
    return torch.from_numpy(host).to(dev())


def run_raw(ref, ws_byte=0, ws_offset=0):
    """tables -> device, ctpvae_gridrec_workspace_bytes, ctpvae_gridrec_f32 on the current stream.  The workspace is `ws_byte` in
    every byte and starts `ws_offset` bytes into its buffer; the output starts as NaN."""
    lib = _lib.load()
    dy, dt, dx = ref["data"].shape
    data = torch.from_numpy(ref["data"].copy()).to(dev())
    tab = device_tables(dt, dx, ref["center"], ref["theta"], ref["filt"])
    need = _lib.check(lib.ctpvae_gridrec_workspace_bytes(dy, dt, dx), "gridrec_workspace_bytes")
    buf = torch.full((int(need) + ws_offset,), ws_byte, dtype=torch.uint8, device=dev())
    out = torch.full((dy, ref["gx"], ref["gy"]), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(lib.ctpvae_gridrec_f32(data.data_ptr(), dy, dt, dx, tab.data_ptr(), ref["gx"], ref["gy"], buf.data_ptr() + ws_offset,
                                      out.data_ptr(), _stream_ptr()), "gridrec")
    torch.cuda.synchronize()
    return out


def assert_within_bounds(tag, got, ref):
    got = to_np(got)
    assert got.shape == ref["twin"].shape and got.dtype == np.float32
    assert np.isfinite(got).all()
    e_twin, e_orc = tw.err(got, ref["twin"]), tw.err(got, ref["oracle"])
    bound = tw.MARGIN * max(ref["e_oracle"], tw.ONE_ROUNDING)
    print(f"gridrec {tag} {ref['name']}: pdim {ref['pdim']}, err vs twin {e_twin:.3e} (bound {bound:.3e}), e_oracle {ref['e_oracle']:.3e}, "
          f"vs oracle {e_orc:.2e}, {int((got != ref['oracle']).sum())} of {got.size} values differ from the oracle")
    assert e_twin <= bound
    assert e_orc <= tw.REL


@pytest.mark.parametrize("name", CENTRED)
def test_recon_against_the_twin(oracle, c5_width, name):
    ref = tw.reference(oracle, name, c5_width)
    got = run_recon(ref)
    assert_within_bounds("recon()", got, ref)
    assert torch.equal(run_recon(ref), got)                  # deterministic: a gather, no atomics


@pytest.mark.parametrize("name", SHIFTED)
def test_raw_entry_points_at_a_shifted_centre(oracle, c5_width, name):
    ref = tw.reference(oracle, name, c5_width)
    assert ref["center"] != ref["data"].shape[2] / 2.0
    got = run_raw(ref)
    assert_within_bounds("raw", got, ref)
    assert torch.equal(run_raw(ref), got)


@pytest.mark.parametrize("name", list(STALE))
def test_a_stale_workspace_cannot_reach_the_result(oracle, c5_width, name):
    """The workspace's contents are undefined (include/ctpvae_radon.h): every float a NaN, or the workspace 256 bytes into a larger
    NaN buffer, gives the bits of a zeroed workspace and of recon(); no output element keeps its NaN."""
    ref = tw.reference(oracle, name, c5_width)
    assert ref["pdim"] == STALE[name] and ref["offset"] == 0.0
    clean = run_raw(ref, ws_byte=0)
    assert_within_bounds("raw, zeroed workspace", clean, ref)
    assert torch.equal(run_raw(ref, ws_byte=0xFF), clean)
    assert torch.equal(run_raw(ref, ws_byte=0xFF, ws_offset=256), clean)
    assert torch.equal(run_recon(ref), clean)


def test_small_cases_are_the_oracles_bits(oracle, c5_width):
    """"In practice the bits" (README): same tables, same butterflies, and the gather adds in gridrec.c's scatter order -- where a
    sample reaches a cell directly and through its mirror, or the cell is its own mirror, the order of the two additions is
    gridrec.c's.  Special angles, many angles, ragged pairs; the padded rows small enough for every cell to be near the origin.
    This is STRICTER than the documented contract (<= 1e-5): it is the one test that sees the order of two additions, and it holds
    as long as host and device compile the butterflies and the gather unfused (-ffp-contract=off); a toolchain that contracts them
    would turn it red without a defect in the kernel, and the 1e-5 tests above would still decide."""
    for name in ("dx1", "dx15", "dx16", "dx17", "dt300", "dy5", "dy11", "grid33x47"):
        ref = tw.reference(oracle, name, c5_width)
        got = to_np(run_recon(ref))
        differ = int((got.view(np.uint32) != ref["oracle"].view(np.uint32)).sum())
        print(f"gridrec {name}: {differ} of {got.size} values differ from the oracle")
        assert differ == 0, name


def raw_refused(dy, dt, dx, gx, gy, match):
    """ctpvae_gridrec_f32 with these sizes returns EINVAL and leaves the output as it was (nothing is launched: the operands
    behind the pointers are far smaller than the sizes claim)."""
    lib = _lib.load()
    d = dev()
    small = torch.zeros(4096, dtype=torch.float32, device=d)
    out = torch.full((4096,), 7.0, dtype=torch.float32, device=d)
    rc = lib.ctpvae_gridrec_f32(small.data_ptr(), dy, dt, dx, small.data_ptr(), gx, gy, small.data_ptr(), out.data_ptr(), _stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.EINVAL and match in _lib.last_error(), (rc, _lib.last_error())
    assert bool((out == 7.0).all())


def test_refusals_launch_nothing():
    d = dev()
    raw_refused(1, 3, 2049, 16, 16, "2048")
    raw_refused(1, 3, 30, 33, 16, "must not exceed")          # pdim = 32
    raw_refused(1, 3, 30, 16, 33, "must not exceed")
    raw_refused(1, 4097, 16, 16, 16, "4096")
    raw_refused(0, 3, 16, 16, 16, "positive")
    theta = np.linspace(0, 3, 5, dtype=np.float32)
    with pytest.raises(ValueError, match="2048"):
        recon(torch.zeros((1, 5, 2049), device=d), theta, sinogram_order=True, algorithm="gridrec")
    with pytest.raises(ValueError, match="must not exceed"):
        recon(torch.zeros((1, 5, 30), device=d), theta, sinogram_order=True, algorithm="gridrec", num_gridx=33)
    with pytest.raises(ValueError, match="4096"):
        recon(torch.zeros((1, 4097, 16), device=d), np.zeros(4097, np.float32), sinogram_order=True, algorithm="gridrec")
    with pytest.raises(ValueError, match="filter_name"):
        recon(torch.zeros((1, 5, 30), device=d), theta, sinogram_order=True, algorithm="gridrec", filter_name="lanczos")
    lib = _lib.load()
    host = np.full(int(lib.ctpvae_gridrec_tables_bytes(5, 30)), 0xA5, np.uint8)
    par = np.array(tw.BUTTERWORTH_PAR, np.float32)
    assert lib.ctpvae_gridrec_tables_host_f32(5, 30, ctypes.c_float(15.0), theta.ctypes.data, 8, par.ctypes.data, host.ctypes.data) == _lib.EINVAL
    assert (host == 0xA5).all()


def test_table_cache_eviction(oracle):
    """ct_pvae_amd/recon.py keeps the tables of 16 (angles, width, filter) keys: seventeen distinct angle sets evict the first, and
    using it again rebuilds tables that give its first result's bits."""
    rm = importlib.import_module("ct_pvae_amd.recon")
    d = dev()
    rng = np.random.default_rng(17)
    data = rng.random((1, 4, 16), dtype=np.float32)
    thetas = [tw.make_theta("special", 4, rng) for _ in range(17)]
    assert len({t.tobytes() for t in thetas}) == 17
    rm._GRIDREC_TABLES.clear()
    run = lambda t: recon(torch.from_numpy(data).to(d), t, sinogram_order=True, algorithm="gridrec")
    firsts = [run(t) for t in thetas]
    assert len(rm._GRIDREC_TABLES) == 16 and not any(k[0] == thetas[0].tobytes() for k in rm._GRIDREC_TABLES)
    again = run(thetas[0])
    assert torch.equal(again, firsts[0]) and len(rm._GRIDREC_TABLES) == 16
    assert tw.err(to_np(again), oracle.gridrec(data, thetas[0])) <= tw.REL
    assert torch.equal(run(thetas[16]), firsts[16])           # a cached entry: the same bits as well


def test_on_a_side_stream(oracle):
    """The data are produced and recon() runs inside torch.cuda.stream(side): every launch goes to that stream, and the result is
    the default stream's, bit for bit."""
    d = dev()
    rng = np.random.default_rng(3)
    host = rng.random((3, 9, 30), dtype=np.float32)
    theta = tw.make_theta("special", 9, rng)

    def produce_and_run():
        x = torch.from_numpy(host).to(d)
        for _ in range(20):                                  # a chain of launches ahead of gridrec's on the same stream
            x = x * 2.0
            x = x * 0.5
        return recon(x, theta, sinogram_order=True, algorithm="gridrec", filter_name="hann")

    want = produce_and_run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=d)
    with torch.cuda.stream(side):
        got = produce_and_run()
    side.synchronize()
    assert torch.equal(got, want)
    assert tw.err(to_np(got), oracle.gridrec(host, theta, filter_name="hann")) <= tw.REL
