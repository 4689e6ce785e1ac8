"""Developer tool (no GPU needed): the store policies (StorePolicy, ct_pvae_amd/csrc/common.h; knob WT_STORES) in the gfx950 assembly.

    python tools/count_store_isa.py [parent.s]

Prints (1) what each store helper compiles to -- a probe kernel per helper and policy --, (2) for every write-through form of the planned
backward (rotate_bwd_planned_kernel_wt<...>) its plain twin, both instruction counts, the cache bits of their global stores, their scratch
bytes and whether the two listings are equal once the bits are taken off the stores, and (3) with the assembly of another build of
rotate_plan.hip (hipcc -S --cuda-device-only with the library's flags), whether every kernel of that build is in this one instruction for
instruction (branch labels aside)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_prologue_isa as base

CSRC = os.path.join(base.ROOT, "ct_pvae_amd", "csrc")
PROBE = """
#include "common.h"
using namespace ctpvae;
#define PROBE(NAME, ST)                                                                                                  \\
    extern "C" __global__ void probe_f32_##NAME(float *p, float v) { store_f32<ST>(v, p + threadIdx.x); }               \\
    extern "C" __global__ void probe_f32x2_##NAME(float *p, float v, float w) { store_f32x2<ST>(v, w, p + 2 * threadIdx.x); }
PROBE(plain, kStorePlain)
PROBE(wt, kStoreWriteThrough)
PROBE(nt, kStoreNonTemporal)
"""
STORE = re.compile(r"^(global|flat|buffer|scratch)_(store|atomic)")


def listings(asm):
    """{symbol: [instruction, ...]} with whitespace and branch labels normalised"""
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):   # (a kernel may hold several s_endpgm)
        ins = []
        for line in m.group(2).split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") or line.endswith(":"):
                continue
            ins.append(re.sub(r"\.LBB\d+_", "L", re.sub(r"\s+", " ", line)))
        out[m.group(1)] = ins
    return out


def scratch_bytes(asm):
    """{symbol: private segment bytes}"""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(?:.*\n)*?\s*\.amdhsa_private_segment_fixed_size (\d+)", asm)}


def stores(ins):
    return [i for i in ins if STORE.match(i)]


def bits(store):
    return sorted(w for w in store.split() if w in ("sc0", "sc1", "nt"))


def without_bits(ins):
    return [" ".join(w for w in i.split() if w not in ("sc0", "sc1", "nt")) if STORE.match(i) else i for i in ins]


def probe_assembly():
    hipcc = base.find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "probe.hip"), os.path.join(tmp, "probe.s")
        open(src, "w").write(PROBE)
        subprocess.run([hipcc, *base.FLAGS, "-I", CSRC, src, "-o", out], check=True, capture_output=True)
        return open(out).read()


def twins(asm, suffix="_wt"):
    """[(plain name, twin name, plain listing, twin listing, plain scratch, twin scratch)] of the planned backward"""
    lst, scr = listings(asm), scratch_bytes(asm)
    names = base.demangle([s for s in lst if s.startswith("_Z")])
    by_name = {n: s for s, n in names.items()}
    res = []
    for n, s in sorted(by_name.items()):
        if n.startswith("rotate_bwd_planned_kernel%s<" % suffix):
            plain = by_name.get(n.replace("rotate_bwd_planned_kernel%s<" % suffix, "rotate_bwd_planned_kernel<"))
            res.append((n.replace(suffix + "<", "<"), n, lst.get(plain), lst[s], scr.get(plain), scr.get(s)))
    return res


if __name__ == "__main__":
    for sym, ins in sorted(listings(probe_assembly()).items()):
        print("%-20s %d instructions, stores: %s" % (sym, len(ins), stores(ins)))
    asm = base.assembly()
    for plain, twin, a, b, sa, sb in twins(asm):
        print("%-52s %5d | %-56s %5d instructions | store bits %s | %s | scratch %s / %s | equal but for the bits: %s"
              % (plain, len(a or ()), twin, len(b), sorted({" ".join(bits(s)) for s in stores(a or ())}), sorted({" ".join(bits(s)) for s in stores(b)}),
                 sa, sb, a is not None and without_bits(a) == without_bits(b)))
    if len(sys.argv) > 1:
        old, new = listings(open(sys.argv[1]).read()), listings(asm)
        names = base.demangle([s for s in old if s.startswith("_Z")])
        for s, n in sorted(names.items(), key=lambda kv: kv[1]):
            print("%-60s %5d instructions in the other build, %s" % (n, len(old[s]), "the same here" if old[s] == new.get(s) else "DIFFERENT here"))
