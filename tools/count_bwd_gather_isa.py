"""Developer tool (no GPU needed): the gather phase of the planned backward's SHORT forms (at most 32 angles) in the gfx950 assembly.

    python tools/count_bwd_gather_isa.py [other.s]

For each of the four SHORT instantiations of rotate_bwd_planned_kernel and their write-through twins, in the region BEHIND the kernel's
last s_barrier (static order): the registers zeroed (`v_mov_b32 vN, 0`: the accumulators may be, a tap may not), the scratch bytes, and
one line per basic block that holds gathers -- its SDWA unpacks (v_lshlrev_b32_sdwa), LDS reads (ds_read_b32 / ds_read_b64: one per
tap) and tap adds (v_add_f32 of single slices, v_pk_add_f32 of pairs; a v_pk_add_f32 of the single-slice form adds two rows' taps and
counts twice).  A launch of A angles consumes na4 / 4 = 1 .. 8 index dwords per owned row: a full vector of four when A > 16, and a
tail of t = 1 .. 4; a block that is the straight-line code of t dwords holds 4 t PPT of each.  With the assembly of another build of
rotate_plan.hip (hipcc -S --cuda-device-only with the library's flags) the same is printed for that build."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_prologue_isa as base
import count_store_isa as stores

SHORT = re.compile(r"^rotate_bwd_planned_kernel(_wt)?<(\d+), (\d+), (\d+), 1, true>$")
ZERO = re.compile(r"^v_mov_b32(_e32)? v\d+, 0$")
BRANCH = ("s_branch", "s_cbranch", "s_endpgm", "s_setpc")


def bodies(asm):
    """{symbol: [line, ...]}: instructions and the labels between them"""
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        lines = []
        for line in m.group(2).split("\n"):
            line = re.sub(r"\s+", " ", line.split(";")[0].strip())
            if line and (not line.startswith(".") or re.match(r"^\.LBB\d+_\d+:$", line)):
                lines.append(line)
        out[m.group(1)] = lines
    return out


def blocks(lines):
    """basic blocks: a label starts one, a branch ends one"""
    res, cur = [], []
    for line in lines:
        if line.endswith(":"):
            if cur:
                res.append(cur)
            cur = []
            continue
        cur.append(line)
        if line.startswith(BRANCH):
            res.append(cur)
            cur = []
    if cur:
        res.append(cur)
    return res


def taps(block, ns):
    """(unpacks, LDS reads, tap adds) of a block"""
    op = [i.split()[0] for i in block]
    pk, single = sum(o.startswith("v_pk_add_f32") for o in op), sum(o.startswith("v_add_f32") for o in op)
    return (sum(o.startswith("v_lshlrev_b32_sdwa") for o in op), sum(o in ("ds_read_b32", "ds_read_b64") for o in op),
            pk if ns == 2 else single + 2 * pk)


def count(asm):
    """{instantiation: {"ppt", "ns", "zero_movs", "scratch", "behind": instructions behind the last barrier,
                        "blocks": [(unpacks, reads, adds), ...] of the blocks behind it that hold a gather}}"""
    raw, scratch = bodies(asm), stores.scratch_bytes(asm)
    names = base.demangle([s for s in raw if s.startswith("_Z")])
    res = {}
    for sym, name in names.items():
        m = SHORT.match(name)
        if not m:
            continue
        ppt, ns = int(m.group(2)), int(m.group(4))
        lines = raw[sym]
        last = max(i for i, line in enumerate(lines) if line == "s_barrier")
        behind = lines[last + 1:]
        res[name] = {"ppt": ppt, "ns": ns, "scratch": scratch.get(sym),
                     "behind": sum(not line.endswith(":") for line in behind),
                     "zero_movs": sum(bool(ZERO.match(line)) for line in behind),
                     "blocks": [t for t in (taps(b, ns) for b in blocks(behind)) if any(t)]}
    return res


def report(asm, tag):
    for name, r in sorted(count(asm).items()):
        print("%-8s %-56s behind the last barrier: %4d instructions, %3d zeroing moves (allowance PPT x NS = %d), scratch %s"
              % (tag, name, r["behind"], r["zero_movs"], r["ppt"] * r["ns"], r["scratch"]))
        for u, l, a in r["blocks"]:
            print("%-8s     block: %3d unpacks %3d LDS reads %3d adds  (per row: %g / %g / %g)"
                  % (tag, u, l, a, u / r["ppt"], l / r["ppt"], a / r["ppt"]))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        report(open(sys.argv[1]).read(), "other")
    report(base.assembly(), "tree")
