#!/usr/bin/env python3
"""Static figures of the k_scan5 instantiations from the compiler's assembly: needs hipcc, no GPU.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o scan5.s gofindthem_amd/csrc/gft_scan5.hip
    python3 tools/isa_counts.py scan5.s [kernel-name-substring]

Per kernel: the registers and spills of its .amdhsa / metadata lines, its size in bytes, and instruction counts by kind in the whole
kernel and inside the unit loop.  Kinds: VALU = v_* without the two lane-spill moves and without v_readfirstlane, SALU = s_* without
s_load* / s_buffer_load* (scalar memory), s_waitcnt, s_nop, s_endpgm, s_barrier and the branches (s_branch, s_cbranch_*, counted as
`branch`); LDS = ds_*; VMEM = global_* / flat_* / buffer_* / scratch_*.  The unit loop is the widest backward branch of the kernel
(the `for (; u < P.n_units; u = nu)` loop encloses everything but table staging and the epilogue); `once` = the instructions of the
loop's blocks that are NOT inside any inner loop, i.e. that run once per unit or less.
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
    ins = []                                   # (mnemonic, branch target or None)
    labels = {}
    for t in body:
        t = t.split(";")[0].strip()
        if not t or t.startswith("."):
            m = re.match(r"^(\.LBB\w+):", t)
            if m:
                labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        parts = t.split()
        tgt = parts[1] if parts[0].startswith(("s_branch", "s_cbranch")) and len(parts) > 1 else None
        ins.append((parts[0], tgt))
    back = [(labels[tg], i) for i, (m, tg) in enumerate(ins) if tg in labels and labels[tg] <= i]
    whole = Counter(kind(m) for m, _ in ins)
    if not back:
        return whole, Counter(), Counter(), len(ins)
    lo, hi = max(back, key=lambda b: b[1] - b[0])
    loop = Counter(kind(m) for m, _ in ins[lo:hi + 1])
    inner = [b for b in back if lo <= b[0] and b[1] <= hi and (b[0], b[1]) != (lo, hi)]
    covered = [False] * len(ins)
    for a, b in inner:
        for i in range(a, b + 1):
            covered[i] = True
    once = Counter(kind(ins[i][0]) for i in range(lo, hi + 1) if not covered[i])
    return whole, loop, once, len(ins)


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_scan5"
    bodies, meta = kernels(path)
    cols = ["VALU", "SALU", "v_readlane", "v_writelane", "LDS", "VMEM", "SMEM", "branch"]
    for sym in sorted(bodies):
        if want not in sym:
            continue
        whole, loop, once, n = analyse(bodies[sym])
        mt = meta.get(sym, {})
        print(demangle(sym).replace("gft::(anonymous namespace)::", "").replace("(gft::Scan2Params)", ""))
        print("  VGPRs %s  SGPRs %s  spilled SGPRs %s  spilled VGPRs %s  scratch %s B  instructions %d" % (
            mt.get("vgpr_count", mt.get("vgprs", "?")), mt.get("sgpr_count", mt.get("sgprs", "?")), mt.get("sgpr_spill_count", "?"),
            mt.get("vgpr_spill_count", "?"), mt.get("private_segment_fixed_size", "?"), n))
        for tag, c in (("whole kernel", whole), ("unit loop", loop), ("  once per unit", once)):
            print("  %-16s" % tag + "  ".join("%s %d" % (k, c.get(k, 0)) for k in cols))


if __name__ == "__main__":
    main()
