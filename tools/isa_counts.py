#!/usr/bin/env python3
"""Static figures of the k_scan5 instantiations from the compiler's assembly: needs hipcc, no GPU.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o scan5.s gofindthem_amd/csrc/gft_scan5.hip
    python3 tools/isa_counts.py scan5.s [kernel-name-substring]

Per kernel: the registers and spills of its .amdhsa / metadata lines, its size in bytes, and instruction counts by kind in the whole
kernel and inside the unit loop.  Kinds: VALU = v_* without the two lane-spill moves and without v_readfirstlane, SALU = s_* without
s_load* / s_buffer_load* (scalar memory), s_waitcnt, s_nop, s_endpgm, s_barrier and the branches (s_branch, s_cbranch_*, counted as
`branch`); LDS = ds_*; VMEM = global_* / flat_* / buffer_* / scratch_*.  The unit loop is the largest top-level loop of the
kernel by the compiler's loop comments (the `for (; u < P.n_units; u = nu)` loop encloses everything but table staging and the
epilogue); `once` = the instructions of the loop's blocks that are NOT inside any inner loop, i.e. that run once per unit or less.  `vmcnt(0)` = the s_waitcnt instructions
that drain the vector-memory counter (loads AND stores), counted in the same three scopes.

    python3 tools/isa_counts.py scan5.s [kernel-name-substring] --once-vmem

lists, per kernel and in layout order, the vector-memory instructions and the vmcnt waits of the `once` part: what a unit issues
and waits for between the flush of the unit before and its own filter ("The unit boundary").
"""
import re
import subprocess
import sys
from collections import Counter


def kind(m):
    if m in ("v_readlane_b32", "v_writelane_b32"):
        return m[:-4]
    if m.startswith("v_readfirstlane"):
        return "v_readfirstlane"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if m.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if m.startswith(("s_branch", "s_cbranch")):
        return "branch"
    if m.startswith(("s_waitcnt", "s_nop", "s_endpgm", "s_barrier", "s_sleep", "s_setprio", "s_trap", "s_code_end")):
        return "other"
    if m.startswith("s_"):
        return "SALU"
    return "other"


def demangle(n):
    try:
        return subprocess.run(["c++filt", n], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return n


def kernels(path):
    """-> {symbol: [lines of the body]} and {symbol: {amdhsa / metadata figures}}"""
    bodies, cur, name = {}, None, None
    meta = {}
    mname = None
    for line in open(path):
        t = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if t.startswith(".Lfunc_end"):
                bodies[name] = cur
                cur = None
            else:
                cur.append(t)
            continue
        m = re.match(r"\.amdhsa_kernel (\S+)", t)
        if m:
            mname = m.group(1)
            meta.setdefault(mname, {})
        m = re.match(r"\.amdhsa_next_free_([vs]gpr) (\d+)", t)
        if m and mname:
            meta[mname][m.group(1) + "s"] = int(m.group(2))
        m = re.match(r"\.name:\s+(\S+)", t)
        if m:
            mname = m.group(1)
            meta.setdefault(mname, {})
        m = re.match(r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|sgpr_count|vgpr_count):\s+(\d+)", t)
        if m and mname:
            meta[mname][m.group(1)] = int(m.group(2))
    return bodies, meta


def analyse(body):
    """The loops are the compiler's own: its comments name every block's innermost loop ("in Loop: Header=BB10_59 Depth=1") and
    every header ("Loop Header: Depth=2").  The unit loop is the top-level loop with the most instructions; `once` = its blocks
    of depth 1.  (Backward branches do not find it: the layout puts blocks of the epilogue in front of the loop.)"""
    ins = []                                   # (mnemonic, the instruction's text, top-level loop header or None, loop depth)
    top, depth = None, 0
    for raw in body:
        code, _, comment = raw.partition(";")
        code = code.strip()
        label = re.match(r"^(\.LBB\w+):", code)
        block = label or re.match(r"^\s*%bb\.\d+:", comment)
        m = re.search(r"in Loop: Header=(BB\w+) Depth=(\d+)", comment)
        if m:
            depth = int(m.group(2))
            if depth == 1:
                top = m.group(1)
        elif re.search(r"Loop Header: Depth=(\d+)", comment):
            depth = int(re.search(r"Loop Header: Depth=(\d+)", comment).group(1))
            if depth == 1 and label:
                top = label.group(1)[2:]
        elif block and "Parent Loop" not in comment:
            top, depth = None, 0               # (a block outside every loop)
        if label or not code or code.startswith("."):
            continue
        parts = code.split()
        ins.append((parts[0], " ".join(parts), top if depth else None, depth))

    def count(sel):
        c = Counter(kind(m) for m, _, _, _ in sel)
        c["vmcnt(0)"] = sum(1 for m, t, _, _ in sel if m == "s_waitcnt" and "vmcnt(0)" in t)
        return c

    whole = count(ins)
    sizes = Counter(t for _, _, t, _ in ins if t)
    if not sizes:
        return whole, Counter(), Counter(), len(ins), []
    unit = sizes.most_common(1)[0][0]
    loop = count([i for i in ins if i[2] == unit])
    sel = [i for i in ins if i[2] == unit and i[3] == 1]
    vmem = [t for m, t, _, _ in sel if kind(m) == "VMEM" or (m == "s_waitcnt" and "vmcnt" in t)]
    return whole, loop, count(sel), len(ins), vmem


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0]
    want = args[1] if len(args) > 1 else "k_scan5"
    listing = "--once-vmem" in sys.argv
    bodies, meta = kernels(path)
    cols = ["VALU", "SALU", "v_readlane", "v_writelane", "LDS", "VMEM", "SMEM", "branch", "vmcnt(0)"]
    for sym in sorted(bodies):
        if want not in sym:
            continue
        whole, loop, once, n, vmem = analyse(bodies[sym])
        mt = meta.get(sym, {})
        print(demangle(sym).replace("gft::(anonymous namespace)::", "").replace("(gft::Scan2Params)", ""))
        print("  VGPRs %s  SGPRs %s  spilled SGPRs %s  spilled VGPRs %s  scratch %s B  instructions %d" % (
            mt.get("vgpr_count", mt.get("vgprs", "?")), mt.get("sgpr_count", mt.get("sgprs", "?")), mt.get("sgpr_spill_count", "?"),
            mt.get("vgpr_spill_count", "?"), mt.get("private_segment_fixed_size", "?"), n))
        for tag, c in (("whole kernel", whole), ("unit loop", loop), ("  once per unit", once)):
            print("  %-16s" % tag + "  ".join("%s %d" % (k, c.get(k, 0)) for k in cols))
        if listing:
            for t in vmem:
                print("      " + t)


if __name__ == "__main__":
    main()
