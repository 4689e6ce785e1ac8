"""Developer tool (no GPU needed): the index requests of the planned backward's SHORT forms (at most 32 angles) in the gfx950 assembly.

    python tools/count_bwd_tail_isa.py [other.s]
    python tools/count_bwd_tail_isa.py --fingerprint other.s      (JSON: what tests/golden/r17_rotate_plan_isa.json records of a build)

A SHORT launch requests its index data ahead of everything else, each request in a block of its own that the launch constant idx_req
selects (rotate_bwd_planned_kernel.h): the last index vector whole (PPT global_load_dwordx4), or its 1, 2 or 3 live dwords from the plan's
compact tail section (PPT global_load_dword, _dwordx2, _dwordx3), and the full first vector (PPT global_load_dwordx4).  For each of the
four SHORT instantiations and their write-through twins this prints the widths of the index requests ahead of the first s_barrier in static
order (they are addressed by the plan's address in scalar registers and a 32-bit offset; the cotangent rows requested behind them by a
register pair, `off`), with the kernel's VGPRs and scratch bytes; with the assembly of another build of rotate_plan.hip (hipcc -S
--cuda-device-only with the library's flags) the same for that build, and which kernels of the file differ between the two."""
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_prologue_isa as base
import count_store_isa as stores

SHORT = re.compile(r"^rotate_bwd_planned_kernel(_wt)?<(\d+), (\d+), (\d+), 1, true>$")
LOAD = re.compile(r"^global_load_dword(x[234])? (\S+), (\S+), (\S+)")


def vgprs(asm):
    """{symbol: VGPRs}"""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(?:.*\n)*?\s*\.amdhsa_next_free_vgpr (\d+)", asm)}


def kernels(asm):
    """{demangled name: (listing, VGPRs, scratch bytes)} of every kernel of the file (branch labels normalised)"""
    lst, vg, scr = stores.listings(asm), vgprs(asm), stores.scratch_bytes(asm)
    names = base.demangle([s for s in lst if s.startswith("_Z")])
    return {names[s]: (lst[s], vg.get(s), scr.get(s)) for s in names if s in vg}


def requests(listing):
    """widths in dwords of the index requests: the global loads ahead of the first s_barrier (static order) that are addressed by a
    scalar base and a 32-bit offset"""
    out = []
    for ins in listing:
        if ins == "s_barrier":
            break
        m = LOAD.match(ins)
        if m and m.group(4).startswith("s["):
            out.append(int(m.group(1)[1]) if m.group(1) else 1)
    return out


def count(asm):
    """{SHORT instantiation: {"ppt", "requests": [widths], "vgprs", "scratch"}}"""
    res = {}
    for name, (listing, vg, scr) in kernels(asm).items():
        m = SHORT.match(name)
        if m:
            res[name] = {"ppt": int(m.group(2)), "requests": requests(listing), "vgprs": vg, "scratch": scr}
    return res


def fingerprint(asm):
    """{"short_vgprs": {SHORT form: VGPRs}, "others": {every other kernel of the file: sha256 of its listing}}"""
    ks = kernels(asm)
    return {"short_vgprs": {n: k[1] for n, k in sorted(ks.items()) if SHORT.match(n)},
            "others": {n: hashlib.sha256("\n".join(k[0]).encode()).hexdigest() for n, k in sorted(ks.items()) if not SHORT.match(n)}}


def report(asm, tag):
    for name, r in sorted(count(asm).items()):
        w = r["requests"]
        print("%-8s %-56s index requests ahead of the barrier: %-32s = %d x4, %d x3, %d x2, %d x1 (PPT = %d); %3d VGPRs, scratch %s"
              % (tag, name, " ".join(map(str, w)), w.count(4), w.count(3), w.count(2), w.count(1), r["ppt"], r["vgprs"], r["scratch"]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--fingerprint":
        print(json.dumps(fingerprint(open(sys.argv[2]).read()), indent=1))
        sys.exit(0)
    asm = base.assembly()
    if len(sys.argv) > 1:
        other = open(sys.argv[1]).read()
        report(other, "other")
        a, b = fingerprint(other)["others"], fingerprint(asm)["others"]
        for n in sorted(set(a) | set(b)):
            print("%-8s %-64s %s" % ("both", n, "the same instructions" if a.get(n) == b.get(n) else "DIFFERENT"))
    report(asm, "tree")
