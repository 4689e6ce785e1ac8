"""The likelihood training call on the ray-driven projector (model="siddon"): what can be checked without a GPU -- the two
entry points in header, binding table and library, their argument checks, the keyword's validation, the trainer's flag, and
the register budget of siddon.hip's kernels."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.conftest import ROOT

NEW = ("ctpvae_siddon_fwd_loglik_f32", "ctpvae_siddon_bwd_sel_scaled_f32")


@pytest.fixture(scope="module")
def built_lib():
    from ct_pvae_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ct_pvae_amd", "csrc"), "-s"], check=True)
    return _lib


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "ctpvae_radon.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (ctpvae_[a-z0-9_]+)", out))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in built_lib.SIGNATURES and name in exported, name
    assert len(built_lib.SIGNATURES[NEW[0]][1]) == 22 and len(built_lib.SIGNATURES[NEW[1]][1]) == 17
    macro = int(re.search(r"#define\s+CTPVAE_ABI_VERSION\s+(\d+)", header).group(1))
    assert built_lib.load().ctpvae_abi_version() == built_lib.ABI_VERSION == macro == 3400


def test_null_pointers_and_bad_sizes_are_refused_before_any_hip_call(built_lib):
    import ctypes
    lib = built_lib.load()
    f = ctypes.c_float
    rc = lib.ctpvae_siddon_fwd_loglik_f32(None, 2, 8, 8, None, None, None, 4, 12, f(6.0), None, 4, None, None, 0, None, f(1e-7),
                                          None, None, None, None, None)
    assert rc == built_lib.EINVAL and "null" in built_lib.last_error()
    rc = lib.ctpvae_siddon_bwd_sel_scaled_f32(None, 2, 8, 8, None, None, None, 4, 12, f(6.0), None, 4, None, None, 0, None, None)
    assert rc == built_lib.EINVAL and "null" in built_lib.last_error()
    # sizes are looked at before anything is launched: host buffers stand in for the device pointers (never dereferenced)
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    rc = lib.ctpvae_siddon_fwd_loglik_f32(p, 2, 0, 8, p, p, p, 4, 12, f(6.0), None, 4, p, p, 0, p, f(1e-7), None, None, p, None, None)
    assert rc == built_lib.EINVAL and "sizes" in built_lib.last_error()
    rc = lib.ctpvae_siddon_fwd_loglik_f32(p, 2, 8, 8, p, p, p, 4, 12, f(6.0), p, 0, p, p, 1, p, f(1e-7), None, None, p, None, None)
    assert rc == built_lib.EINVAL and "n_sel" in built_lib.last_error()
    rc = lib.ctpvae_siddon_fwd_loglik_f32(p, 2, 8, 8, p, p, p, 4, 12, f(6.0), None, 4, p, p, 2, p, f(1e-7), None, None, p, None, None)
    assert rc == built_lib.EINVAL and "dense" in built_lib.last_error()
    rc = lib.ctpvae_siddon_bwd_sel_scaled_f32(p, 2, 8, 8, p, p, p, 0, 12, f(6.0), None, 0, p, None, 0, p, None)
    assert rc == built_lib.EINVAL and "sizes" in built_lib.last_error()
    rc = lib.ctpvae_siddon_bwd_sel_scaled_f32(p, 2, 8, 8, p, p, p, 4, 12, f(6.0), None, 3, p, None, 0, p, None)
    assert rc == built_lib.EINVAL and "n_sel" in built_lib.last_error()
    rc = lib.ctpvae_siddon_bwd_sel_scaled_f32(p, 2, 8, 8, p, p, p, 4, 12, f(6.0), None, 4, p, p, -1, p, None)
    assert rc == built_lib.EINVAL and "stride" in built_lib.last_error()
    # an empty batch is not an error and launches nothing
    assert lib.ctpvae_siddon_fwd_loglik_f32(p, 0, 8, 8, p, p, p, 4, 12, f(6.0), None, 4, p, p, 0, p, f(1e-7), None, None, p, None, None) == 0
    assert lib.ctpvae_siddon_bwd_sel_scaled_f32(p, 0, 8, 8, p, p, p, 4, 12, f(6.0), None, 4, p, None, 0, p, None) == 0


def test_model_keyword_is_validated_before_the_device(built_lib):
    import ct_pvae_amd as cp
    x = torch.zeros((1, 8, 8, 1))
    mask, meas = torch.zeros((1, 3)), torch.zeros((1, 3, 14))
    with pytest.raises(ValueError, match="model must be"):
        cp.calculate_log_prob_M_given_R(x, mask, meas, 1e4, 1e-7, theta=[0.0, 0.5, 1.0], model="fan")
    with pytest.raises(built_lib.RadonLibraryError, match="no CPU path"):
        cp.calculate_log_prob_M_given_R(x, mask, meas, 1e4, 1e-7, theta=[0.0, 0.5, 1.0], model="siddon")
    with pytest.raises(ValueError, match="reduce must be"):
        cp.calculate_log_prob_M_given_R(x, mask, meas, 1e4, 1e-7, theta=[0.0, 0.5, 1.0], model="siddon", reduce="all")


def test_trainer_flag():
    from ct_pvae_amd import trainer as tr
    assert tr.get_args([]).model == "rotate"
    assert tr.get_args(["--model", "siddon"]).model == "siddon"
    with pytest.raises(SystemExit):
        tr.get_args(["--model", "fan"])
    import inspect
    assert inspect.signature(tr.find_loss_vae_unsup).parameters["model"].default == "rotate"


def test_no_siddon_kernel_spills_registers():
    """tests/test_abi.py's gate (hipcc's own resource report shows no scratch) on siddon.hip, which now holds the likelihood
    store of the forward kernels and the scaled, angle-subset store of the gather -- every instantiation, old and new."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "siddon.hip", "-o", os.devnull],
                         cwd=os.path.join(ROOT, "ct_pvae_amd", "csrc"), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen, bad = None, set(), []
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen.add(name)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and int(m.group(1)) > 0:
            bad.append((name, int(m.group(1))))
    assert not bad, f"kernels with scratch (register spills): {bad}"
    # the new instantiations are in the report: forward LL = true (three LDS forms, two packed), gather EPI 3 (four slice counts),
    # the degenerate rays' pass with an angle subset
    for frag, n in (("siddon_fwd_kernelILb1ELi1ELb1E", 1), ("siddon_fwd_kernelILb1ELi2ELb1E", 1), ("siddon_fwd_kernelILb0ELi1ELb1E", 1),
                    ("siddon_fwd_packed_kernelILi4ELb1E", 1), ("siddon_fwd_packed_kernelILi8ELb1E", 1),
                    ("siddon_bwd_degenerate_kernelILb1E", 1)):
        assert sum(frag in s for s in seen) == n, (frag, sorted(seen))
    assert sum(re.search(r"siddon_bwd_gather_kernelILi\dELi3E", s) is not None for s in seen) == 4
