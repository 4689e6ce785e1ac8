"""Developer tool (no GPU needed): the bilinear forward's instantiations, exact and precision="fast" twins side by side.

Compiles ct_pvae_amd/csrc/rotate_bilin.hip device-only to gfx950 assembly with the library's flags and prints, for every
rotate_fwd_bilin_kernel<NS, TILED, PADDED, SORTED, RS, FAST> instantiation: scratch bytes per lane, the fused multiply-adds it holds
(v_pk_fma_f32 / v_fma_f32: the file is compiled -ffp-contract=off, so the exact kernels hold none and the fast ones only their lerps)
and the static number of vector instructions inside its WALK loops -- the loops (a label and a later branch back to it) that hold the
sample's v_cvt_flr_i32_f32.  Static counts are not dynamic ones, but the walk loops are where the kernel spends its time, and a twin
pair differs in the blend alone.

    python tools/count_bilin_isa.py [more hipcc flags ...]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SRC = os.path.join(ROOT, "ct_pvae_amd", "csrc", "rotate_bilin.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S"]
KERNEL = "rotate_fwd_bilin_kernel"


def find_hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def assembly(extra=()):
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "rotate_bilin.s")
        subprocess.run([hipcc, *FLAGS, *extra, SRC, "-o", out], check=True, capture_output=True)
        return open(out).read()


def demangle(names):
    if not names or shutil.which("c++filt") is None:
        return {n: n for n in names}
    res = subprocess.run(["c++filt", *names], capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: r.split("(")[0].replace("void ", "").replace("ctpvae::", "").replace(" ", "") for n, r in zip(names, res)}


def template_args(name):
    """'rotate_fwd_bilin_kernel<2,false,true,false,false,true>' -> (2, False, True, False, False, True)"""
    m = re.search(r"<(.*)>", name)
    if not m:
        return None
    conv = {"true": True, "false": False}
    return tuple(conv[a] if a in conv else int(re.sub(r"[^0-9-]", "", a)) for a in m.group(1).split(","))


def count(asm, kernel=KERNEL):
    """{instantiation: {"scratch", "v_pk_fma_f32", "v_fma_f32", "walk_valu", "walk_total", "total"}}"""
    bodies = {}
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)^\s*s_endpgm(.*?)^\s*\.end_amdhsa_kernel" % kernel, asm, re.M | re.S):
        bodies[m.group(1)] = (m.group(2), m.group(3))
    names = demangle(list(bodies))
    res = {}
    for sym, (body, desc) in bodies.items():
        ins, labels, loops = [], {}, []          # instructions in order; label -> index of the next instruction
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if line.endswith(":"):
                labels[line[:-1]] = len(ins)
                continue
            if not line or line.startswith("."):
                continue
            ins.append(line)
        for i, line in enumerate(ins):           # a branch to a label that lies behind it closes a loop
            op = line.split()
            if op[0].startswith(("s_cbranch", "s_branch")) and len(op) > 1 and labels.get(op[-1], len(ins)) <= i:
                loops.append((labels[op[-1]], i))
        inside = set()
        for a, b in loops:
            if any(l.startswith("v_cvt_flr_i32_f32") for l in ins[a:b + 1]):
                inside.update(range(a, b + 1))
        scratch = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc)
        res[names[sym]] = {"scratch": int(scratch.group(1)) if scratch else -1,
                           "v_pk_fma_f32": sum(l.startswith("v_pk_fma_f32") for l in ins),
                           "v_fma_f32": sum(l.startswith(("v_fma_f32", "v_fmac_f32")) for l in ins),
                           "walk_valu": sum(ins[i].startswith("v_") for i in inside), "walk_total": len(inside), "total": len(ins)}
    return res


def twins(res):
    """[(exact name, fast name)] of the instantiations that differ in the FAST flag alone"""
    by_args = {template_args(n): n for n in res}
    return sorted((by_args[a[:5] + (False,)], n) for a, n in by_args.items() if a and len(a) == 6 and a[5] and a[:5] + (False,) in by_args)


if __name__ == "__main__":
    res = count(assembly(sys.argv[1:]))
    for name, r in sorted(res.items()):
        print("%-62s scratch %3d  v_pk_fma_f32 %3d  v_fma_f32 %3d  walk loops: %4d vector of %4d instructions (kernel %5d)"
              % (name, r["scratch"], r["v_pk_fma_f32"], r["v_fma_f32"], r["walk_valu"], r["walk_total"], r["total"]))
    for ex, fa in twins(res):
        print("%-62s walk-loop vector instructions %4d -> %4d fast (%+.1f %%)"
              % (ex, res[ex]["walk_valu"], res[fa]["walk_valu"], 100.0 * (res[fa]["walk_valu"] - res[ex]["walk_valu"]) / max(res[ex]["walk_valu"], 1)))
