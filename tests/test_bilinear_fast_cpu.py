"""precision="fast" without a GPU: the two entry points exist (header, library, binding), refuse bad arguments before any HIP call,
the Python layer refuses what has no fast form, and -- in the gfx950 assembly of rotate_bilin.hip (tools/count_bilin_isa.py) --
every bilinear forward instantiation has a fast twin whose blend is v_pk_fma_f32, whose walk loops hold fewer vector instructions
than the exact twin's, and which uses no scratch; the exact instantiations hold no fused multiply-add at all."""
import importlib.util
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "count_bilin_isa.py")
spec = importlib.util.spec_from_file_location("count_bilin_isa", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)

NEW = ("ctpvae_rotate_fwd_fast_f32", "ctpvae_rotate_fwd_tiled_fast_f32")


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def test_fast_entry_points_are_declared_exported_and_bound(built_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctpvae_radon.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in exported and name in built_lib.SIGNATURES, name
    # the exact functions' argument lists without `interp`
    sig = built_lib.SIGNATURES
    assert len(sig["ctpvae_rotate_fwd_fast_f32"][1]) == len(sig["ctpvae_rotate_fwd_f32"][1]) - 1
    assert len(sig["ctpvae_rotate_fwd_tiled_fast_f32"][1]) == len(sig["ctpvae_rotate_fwd_tiled_interp_f32"][1]) - 1
    assert built_lib.load().ctpvae_abi_version() == 3400      # added entry points, the same ABI


def test_fast_entry_points_report_bad_arguments(built_lib):
    """Null pointers and bad geometry are rejected before any HIP call, so this is safe without a GPU."""
    import ctypes
    lib = built_lib.load()
    fake = ctypes.c_void_p(256)
    assert lib.ctpvae_rotate_fwd_fast_f32(None, 1, 8, 8, 8, 8, 0, 0, None, 1, None, None) == built_lib.EINVAL
    assert "rotate_fwd_fast" in built_lib.last_error() and "null" in built_lib.last_error()
    assert lib.ctpvae_rotate_fwd_fast_f32(fake, 1, 8, 8, 4, 8, 0, 0, fake, 1, fake, None) == built_lib.EINVAL      # canvas smaller than the slice
    assert lib.ctpvae_rotate_fwd_tiled_fast_f32(None, 1, 512, 512, 728, 728, 108, 108, None, 1, None, None, None) == built_lib.EINVAL
    assert "null" in built_lib.last_error()
    # a slice that fits LDS whole is not a tiled geometry, as for the exact function
    assert lib.ctpvae_rotate_fwd_tiled_fast_f32(fake, 1, 64, 64, 92, 92, 14, 14, fake, 4, fake, fake, None) == built_lib.EINVAL
    assert "fits LDS whole" in built_lib.last_error()
    # a 512 x 512 slice does not fit LDS whole, nor do the tables of 4300 angles: no fast form, and no exact kernel instead
    assert lib.ctpvae_rotate_fwd_fast_f32(fake, 1, 512, 512, 728, 728, 108, 108, fake, 6, fake, None) == built_lib.EINVAL
    assert "no fast form" in built_lib.last_error()
    assert lib.ctpvae_rotate_fwd_fast_f32(fake, 1, 40, 40, 58, 58, 9, 9, fake, 4300, fake, None) == built_lib.EINVAL
    assert "no fast form" in built_lib.last_error()


def test_python_layer_refuses_before_touching_a_device():
    import torch

    import ct_pvae_amd as cp
    from ct_pvae_amd.forward_functions import RotatePlan, _check_precision
    _check_precision("exact", "nearest"), _check_precision("exact", "bilinear"), _check_precision("fast", "bilinear")
    with pytest.raises(ValueError, match="bilinear"):
        _check_precision("fast", "nearest")
    with pytest.raises(ValueError, match="precision"):
        _check_precision("quick", "bilinear")
    # the checks come before the device is looked at: a CPU tensor / device gets the ValueError, not "no CPU path"
    with pytest.raises(ValueError, match="bilinear"):
        RotatePlan([0.0, 0.5], 16, 16, True, "cpu", interp="nearest", precision="fast")
    with pytest.raises(ValueError, match="precision"):
        RotatePlan([0.0, 0.5], 16, 16, True, "cpu", interp="bilinear", precision="quick")
    with pytest.raises(ValueError, match="bilinear"):
        cp.project_tf_fast(torch.zeros(16, 16, 1), [0.0, 0.5], pad=True, precision="fast")
    with pytest.raises(ValueError, match="precision"):
        cp.project_tf_low_mem(torch.zeros(16, 16, 1), [0.0, 0.5], pad=True, precision="quick")


@pytest.fixture(scope="module")
def isa():
    if tool.find_hipcc() is None:
        pytest.skip("hipcc is not installed")
    return tool.count(tool.assembly())


def test_every_bilinear_forward_form_has_a_fast_twin_without_scratch(isa):
    pairs = tool.twins(isa)
    forms = {tool.template_args(ex)[:5] for ex, _ in pairs}
    # NS = 1 / 2 / 4 x (whole | tiles) x (padded | not) x (plain | sorted), and the row-split form of whole slices
    want = {(ns, tiled, padded, srt, False) for ns in (1, 2, 4) for tiled in (False, True) for padded in (False, True) for srt in (False, True)}
    want |= {(ns, False, padded, False, True) for ns in (1, 2, 4) for padded in (False, True)}
    assert forms == want, forms ^ want
    assert len(isa) == 2 * len(want), sorted(isa)              # ... and no instantiation without a twin
    for name, r in isa.items():
        assert r["scratch"] == 0, (name, r)


def test_fast_blend_is_packed_fma_and_the_exact_kernels_hold_none(isa):
    for ex, fa in tool.twins(isa):
        e, f = isa[ex], isa[fa]
        print(ex, e, "->", f)
        assert e["v_pk_fma_f32"] == 0 and e["v_fma_f32"] == 0, (ex, e)     # -ffp-contract=off: TensorFlow's unfused blend stays unfused
        ns = tool.template_args(fa)[0]
        if ns in (2, 4):
            assert f["v_pk_fma_f32"] > 0 and f["v_fma_f32"] == 0, (fa, f)  # slice pairs: packed lerps, no scalar ones
        else:
            assert f["v_pk_fma_f32"] + f["v_fma_f32"] > 0, (fa, f)
        assert e["walk_valu"] > 0 and f["walk_valu"] > 0, (ex, e, f)       # the parser found the walk loops
        assert f["walk_valu"] < e["walk_valu"], (fa, f["walk_valu"], e["walk_valu"])
