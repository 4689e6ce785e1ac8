"""Developer tool (no GPU needed): the static prologue of a planned kernel (default: the planned backward), per instantiation.

Compiles ct_pvae_amd/csrc/rotate_plan.hip device-only to gfx950 assembly with the library's flags and prints, for every
instantiation whose name holds the given kernel name (default rotate_bwd_planned_kernel), the number of instructions ahead of its first s_barrier and how many of them belong to
integer-division expansions (v_rcp_iflag_f32: one per unsigned / signed 32-bit division; s_abs_i32: the sign handling of a signed
one).  Static order is not the dynamic path, but a division by a launch constant that is still in the listing is still paid.

    python tools/count_prologue_isa.py [kernel name, e.g. rotate_fwd_planned_kernel] [more hipcc flags ...]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SRC = os.path.join(ROOT, "ct_pvae_amd", "csrc", "rotate_plan.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S"]
KERNEL = "rotate_bwd_planned_kernel"


def find_hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def assembly(extra=()):
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "rotate_plan.s")
        subprocess.run([hipcc, *FLAGS, *extra, SRC, "-o", out], check=True, capture_output=True)
        return open(out).read()


def demangle(names):
    if not names or shutil.which("c++filt") is None:
        return {n: n for n in names}
    res = subprocess.run(["c++filt", *names], capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: r.split("(")[0].replace("void ", "").replace("ctpvae::", "") for n, r in zip(names, res)}


def count(asm, kernel=KERNEL):
    """{instantiation: {"prologue": n, "total": n, "v_rcp_iflag_f32": n, "s_abs_i32": n}} (the last two inside the prologue)"""
    bodies = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)^\s*s_endpgm" % kernel, asm, re.M | re.S):
        bodies[m.group(1)] = m.group(2)
    names = demangle(list(bodies))
    res = {}
    for sym, body in bodies.items():
        ins = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            ins.append(line.split()[0])
        first = ins.index("s_barrier") if "s_barrier" in ins else len(ins)
        pro = ins[:first]
        res[names[sym]] = {"prologue": len(pro), "total": len(ins), "v_rcp_iflag_f32": sum(i.startswith("v_rcp_iflag_f32") for i in pro),
                           "s_abs_i32": pro.count("s_abs_i32")}
    return res


if __name__ == "__main__":
    argv = sys.argv[1:]
    kernel = argv.pop(0) if argv and not argv[0].startswith("-") else KERNEL
    for name, r in sorted(count(assembly(argv), kernel).items()):
        print("%-58s prologue %4d of %5d instructions, v_rcp_iflag_f32 %2d, s_abs_i32 %2d"
              % (name, r["prologue"], r["total"], r["v_rcp_iflag_f32"], r["s_abs_i32"]))
