#!/usr/bin/env python3
"""The group-finder row in its three forms, same content, same process: JSON documents through
GroupFinder.ProcessJsons (host: JSON decode + walk + rule recursion), the same leaves as records through ProcessRecords (host
arrays up, rule bitmap down) and device-resident through ProcessRecordsDevice (nothing but the status crosses the link).
tools/bench_group.py's shape: documents of ~4 KB over 8 string leaves, 1 000 expressions in 50 tags, 100 rule expressions.
Identical rule results are asserted.  Not part of the bench.py contract.

    python tools/bench_group_records.py [--docs N] [--terms T] [--exprs E]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gofindthem_amd import _lib, group  # noqa: E402
from gofindthem_amd.engine import pack  # noqa: E402
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402
from gofindthem_amd.workload import Workload, make_expressions  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=50000)
ap.add_argument("--terms", type=int, default=10000)
ap.add_argument("--exprs", type=int, default=1000)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

w = Workload(args.terms)
exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
tags = ["tag%d" % (i % 50) for i in range(len(exprs))]
f = Finder(GpuEngine(), EmptyRgxEngine(), False)
for e, t in zip(exprs, tags):
    f.AddExpressionWithTag(e, t)
rules = {"rule%d" % i: ['"tag%d" and not "tag%d:Body"' % (i, (i + 7) % 50), '"tag%d:Meta" or "tag%d:Comments"' % ((i + 3) % 50, i)]
         for i in range(50)}
g = group.NewFinderWithRules(f, rules)
SCHEMA = ["Title", "Body.index(0)", "Body.index(1)", "Body.index(2)", "Meta.Author", "Meta.Notes.index(0)", "Comments.index(0).Text",
          "Comments.index(1).Text"]
g.SetSchema(SCHEMA)

text, off = w.docs_host(0, args.docs)
raws, leaves = [], []
for d in range(args.docs):
    t = bytes(text[int(off[d]):int(off[d + 1])]).decode("ascii")
    n = len(t) // 8
    p = [t[i * n:(i + 1) * n] for i in range(8)]
    raws.append(json.dumps({"Id": d, "Title": p[0], "Body": [p[1], p[2], p[3]], "Meta": {"Author": p[4], "Notes": [p[5]]},
                            "Comments": [{"Text": p[6], "Score": 3}, {"Text": p[7], "Score": 5}]}))
    leaves += p
L = _lib.load()
eh = f.engine_handle()
jblob, joff = pack([r.encode() for r in raws])
lblob, loff = pack(leaves)
lblob = np.concatenate([lblob, np.zeros(64, dtype=np.uint8)])
field = np.tile(np.arange(8, dtype=np.uint32), args.docs)
rec_off = np.arange(args.docs + 1, dtype=np.uint64) * 8
words = g.rule_words()
d_text, d_off = torch.from_numpy(lblob).cuda(), torch.from_numpy(loff.astype(np.int64)).cuda()
d_field, d_rec = torch.from_numpy(field.astype(np.int32)).cuda(), torch.from_numpy(rec_off.astype(np.int64)).cuda()


def run_jsons():
    need = C.c_uint64(0)
    cap = 2 * int(jblob.size)
    buf = C.create_string_buffer(cap)
    t0 = time.perf_counter()
    rc = L.gft_group_process_jsons(g._h, jblob.ctypes.data, joff.ctypes.data, len(raws), None, 0, None, 0, 0, C.cast(buf, C.c_void_p), cap,
                                   C.byref(need))
    dt = time.perf_counter() - t0
    assert rc == 0, L.gft_group_last_error(g._h)
    return dt, buf


def run_records():
    out = np.zeros((args.docs, words), dtype=np.uint32)
    t0 = time.perf_counter()
    rc = L.gft_group_process_records(g._h, lblob.ctypes.data, loff.ctypes.data, field.ctypes.data, rec_off.ctypes.data, args.docs,
                                     len(leaves), out.ctypes.data)
    dt = time.perf_counter() - t0
    assert rc == 0, L.gft_group_last_error(g._h)
    return dt, out


def run_device():
    out = torch.zeros((args.docs, words), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = L.gft_group_process_records_device(g._h, d_text.data_ptr(), d_off.data_ptr(), d_field.data_ptr(), d_rec.data_ptr(), args.docs,
                                            len(leaves), out.data_ptr())
    dt = time.perf_counter() - t0
    assert rc == 0, L.gft_group_last_error(g._h)
    return dt, out




def h2d_reference():
    """what a plain copy of the same pageable text buffer to the device costs in this process: the floor under ProcessRecords"""
    dst = torch.empty(lblob.size, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(lblob)
    best_dt = 1e9
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        best_dt = min(best_dt, time.perf_counter() - t0)
    return best_dt


g.ProcessJsons(raws[:100])               # warm-up: engine build, program and rule-set upload
g.ProcessRecords([[(SCHEMA[0], "warm up")]])
best = {}
for name, fn in (("jsons", run_jsons), ("records", run_records), ("records_device", run_device)):
    for _ in range(args.reps):
        L.gft_profile_enable(eh, 1)
        L.gft_profile_reset(eh)
        dt, out = fn()
        ms = {}
        for cat in (b"scan", b"solve", b"aux", b"group_tags", b"group_rules"):
            a, n = C.c_double(), C.c_uint64()
            L.gft_profile_read(eh, cat, C.byref(a), C.byref(n))
            ms[cat.decode()] = a.value
        L.gft_profile_enable(eh, 0)
        if name not in best or dt < best[name][0]:
            best[name] = (dt, out, ms)

# identical rule results: the JSON route's dicts against the rows of both record routes
numbering = g.rule_exprs()
from_json = json.loads(best["jsons"][1].value.decode())
want = np.zeros((args.docs, words), dtype=np.uint32)
index = {}
for i, key in enumerate(numbering):
    index.setdefault(key, i)
for d, r in enumerate(from_json):
    for name, es in r["rules"].items():
        for e in es:
            i = index[(name, e)]
            want[d, i >> 5] |= np.uint32(1 << (i & 31))
rows_host = best["records"][1]
rows_dev = best["records_device"][1].cpu().numpy().astype(np.uint32)
assert np.array_equal(rows_host, want), "ProcessRecords differs from ProcessJsons"
assert np.array_equal(rows_dev, want), "ProcessRecordsDevice differs from ProcessJsons"
print(json.dumps({
    "row": "SURVEY 8(f) #2 group finder: JSON documents / records / device-resident records", "docs": args.docs, "leaves": len(leaves),
    "leaf_bytes": int(loff[-1]), "json_bytes": int(joff[-1]), "rule_expressions": len(numbering), "finder_expressions": len(exprs),
    "rule_hits": int(np.unpackbits(want.view(np.uint8)).sum()), "identical_rule_results": True,
    **{name + "_per_s": args.docs / best[name][0] for name in best},
    **{name + "_call_s": best[name][0] for name in best},
    "pageable_text_copy_s": h2d_reference(), "text_pinned": bool(torch.from_numpy(lblob).is_pinned()),
    "kernels_ms": {name: best[name][2] for name in best}}))
