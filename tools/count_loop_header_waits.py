"""Developer tool (no GPU needed): the s_waitcnt at every loop header of a .hip file's kernels, and the deepest wait inside each
innermost loop.

Compiles the file device-only to gfx950 assembly with the library's flags (as tools/count_prologue_isa.py does) and prints, per kernel
and per loop of the listing (hipcc marks them: "Loop Header: Depth=d", "in Loop: Header=BBk_n"):
  - the s_waitcnt instructions that open the header block (ahead of its first other instruction): what every trip pays before it starts;
  - for an innermost loop, the smallest vmcnt / lgkmcnt any s_waitcnt of the loop asks for (the header's included), and its LDS reads
    and global loads -- a pipelined loop that keeps k loads in flight never asks for less than k.
A wait that names no counter leaves it alone ("-").

    python tools/count_loop_header_waits.py [file.hip, default ct_pvae_amd/csrc/rotate_plan.hip] [kernel name part] [more hipcc flags ...]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ct_pvae_amd", "csrc")
SRC = os.path.join(CSRC, "rotate_plan.hip")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only", "-S"]


def find_hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def assembly(src=SRC, extra=()):
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        subprocess.run([hipcc, *FLAGS, *extra, src, "-o", out], check=True, capture_output=True)
        return open(out).read()


def demangle(names):
    if not names or shutil.which("c++filt") is None:
        return {n: n for n in names}
    res = subprocess.run(["c++filt", *names], capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: r.split("(")[0].replace("void ", "").replace("ctpvae::", "") for n, r in zip(names, res)}


def parse_wait(ins):
    """'s_waitcnt vmcnt(0) lgkmcnt(7)' -> {'vmcnt': 0, 'lgkmcnt': 7}"""
    return {k: int(v) for k, v in re.findall(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)", ins)}


def loops(asm, kernel=""):
    """{kernel: [loop, ...]} in listing order; loop = {"header": label, "depth": d, "inner": bool, "header_waits": [{counter: n}, ...],
    "min_vmcnt": n or None, "min_lgkmcnt": n or None, "ds_reads": n, "global_loads": n, "waits": [...]} (the last five over the blocks whose
    innermost loop it is, the header block included)"""
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        if kernel in m.group(1) and ".amdhsa_kernel " + m.group(1) in asm:
            bodies[m.group(1)] = m.group(2)
    names = demangle(list(bodies))
    res = {}
    for sym, body in bodies.items():
        found, cur, opening, label = {}, None, False, None

        def header(name, m):
            return found.setdefault(name, {"header": name, "depth": int(m.group(2)), "inner": bool(m.group(1)), "header_waits": [],
                                           "waits": [], "ds_reads": 0, "global_loads": 0})

        for line in body.split("\n"):
            code, _, comment = line.partition(";")
            code = code.strip()
            mark = re.search(r"This (Inner )?Loop Header: Depth=(\d+)", comment)
            m = re.match(r"(?:\.L)?(BB\d+_\d+):", code)
            if m or comment.lstrip().startswith("%bb."):   # a new block: this line names its innermost loop, if it is in one
                label = m.group(1) if m else None
                inside = re.search(r"in Loop: Header=(BB\d+_\d+)", comment)
                cur, opening = (found.get(inside.group(1)) if inside else None), False
                if label and mark:
                    cur, opening = header(label, mark), True
                continue
            if not code:   # (a nested header's label line names its parent loops, the marker follows on a line of its own)
                if mark and label:
                    cur, opening = header(label, mark), True
                continue
            label = None
            if code.startswith(".") or cur is None:
                continue
            if code.startswith("s_waitcnt"):
                w = parse_wait(code)
                cur["waits"].append(w)
                if opening:
                    cur["header_waits"].append(w)
                continue
            opening = False
            cur["ds_reads"] += code.startswith("ds_read")
            cur["global_loads"] += code.startswith("global_load")
        out = []
        for lp in found.values():
            for c in ("vmcnt", "lgkmcnt"):
                vals = [w[c] for w in lp["waits"] if c in w]
                lp["min_" + c] = min(vals) if vals else None
            out.append(lp)
        res[names[sym]] = out
    return res


def fmt(w):
    return " ".join("%s(%d)" % kv for kv in w.items()) or "-"


def report(res):
    lines = []
    for name, lps in sorted(res.items()):
        lines.append(name)
        if not lps:
            lines.append("    (no loop)")
        for lp in lps:
            head = ", ".join(fmt(w) for w in lp["header_waits"]) or "none"
            text = "    %-10s depth %d  header wait: %-28s" % (lp["header"], lp["depth"], head)
            if lp["inner"]:
                text += "  innermost: min vmcnt %s, min lgkmcnt %s, %d ds_read, %d global_load" % (
                    "-" if lp["min_vmcnt"] is None else lp["min_vmcnt"], "-" if lp["min_lgkmcnt"] is None else lp["min_lgkmcnt"],
                    lp["ds_reads"], lp["global_loads"])
            lines.append(text.rstrip())
    return "\n".join(lines)


if __name__ == "__main__":
    argv = sys.argv[1:]
    src = argv.pop(0) if argv and argv[0].endswith(".hip") else SRC
    kernel = argv.pop(0) if argv and not argv[0].startswith("-") else ""
    print(report(loops(assembly(src, argv), kernel)))
