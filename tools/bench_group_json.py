#!/usr/bin/env python3
"""Measurement of the group finder's four ways through a batch of JSON documents, in one process, on the shape of
tools/bench_group.py (50 000 documents of about 4.2 KB with 8 string leaves, 1 000 finder expressions in 50 tags, 100 rules):

    ProcessJsons         the JSON reader and the walk on host threads (the baseline)
    ProcessJsonsSchema   host memory in, the documents decoded on the device (csrc/gft_json.hip)
    ProcessJsonsAuto     as ProcessJsonsSchema without SetSchema: the schema is discovered from the batch on the device
    ProcessJsonsDevice   the same with the blob resident in HBM; status and rule bitmap stay there

Identical rule results are asserted.  One warm-up call each, then the median of --reps calls; the json_* kernel times come
from gft_profile_read in a run of their own.  Not part of the bench.py contract.

    python tools/bench_group_json.py [--docs N] [--terms T] [--exprs E] [--reps R]
"""
import argparse
import ctypes as C
import json
import os
import statistics
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
ap.add_argument("--reps", type=int, default=5)
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
g.SetSchema(["Title", "Body.index(0)", "Body.index(1)", "Body.index(2)", "Meta.Author", "Meta.Notes.index(0)", "Comments.index(0).Text",
             "Comments.index(1).Text"])

text, off = w.docs_host(0, args.docs)
raws = []
for d in range(args.docs):
    t = bytes(text[int(off[d]):int(off[d + 1])]).decode("ascii")
    n = len(t) // 8
    p = [t[i * n:(i + 1) * n] for i in range(8)]
    raws.append(json.dumps({"Id": d, "Title": p[0], "Body": [p[1], p[2], p[3]], "Meta": {"Author": p[4], "Notes": [p[5]]},
                            "Comments": [{"Text": p[6], "Score": 3}, {"Text": p[7], "Score": 5}]}).encode())
blob, boff = pack(raws)
json_bytes = int(blob.size)
L = _lib.load()
eh = f.engine_handle()
cap = 2 * json_bytes + (1 << 16)
buf = C.create_string_buffer(cap)
need = C.c_uint64(0)


def host_route():
    rc = L.gft_group_process_jsons(g._h, blob.ctypes.data, boff.ctypes.data, len(raws), None, 0, None, 0, 0, C.cast(buf, C.c_void_p), cap, C.byref(need))
    assert rc == 0, L.gft_group_last_error(g._h)


def schema_route():
    rc = L.gft_group_process_jsons_schema(g._h, blob.ctypes.data, boff.ctypes.data, len(raws), C.cast(buf, C.c_void_p), cap, C.byref(need))
    assert rc == 0, L.gft_group_last_error(g._h)


def auto_route():
    rc = L.gft_group_process_jsons_auto(g._h, blob.ctypes.data, boff.ctypes.data, len(raws), None, 0, None, 0, C.cast(buf, C.c_void_p), cap, C.byref(need))
    assert rc == 0, L.gft_group_last_error(g._h)


d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(64, dtype=np.uint8)])).cuda()
d_off = torch.from_numpy(boff.astype(np.int64)).cuda()
d_rows = torch.zeros((len(raws), g.rule_words()), dtype=torch.int32, device="cuda")
d_status = torch.zeros(len(raws), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()


def device_route():
    rc = L.gft_group_process_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), len(raws), d_status.data_ptr(), d_rows.data_ptr())
    assert rc == 0, L.gft_group_last_error(g._h)


def timed(fn):
    fn()                                         # warm-up: engine build, buffers grown, pages touched
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


host_s, host_all = timed(host_route)
want = json.loads(buf.value.decode())
schema_s, schema_all = timed(schema_route)
got = json.loads(buf.value.decode())
split = g.json_last()
assert got == want, "ProcessJsonsSchema differs from ProcessJsons"
auto_s, auto_all = timed(auto_route)
got = json.loads(buf.value.decode())
auto_split, auto_last = g.json_last(), g.json_auto_last()
assert got == want, "ProcessJsonsAuto differs from ProcessJsons"
assert auto_s < host_s, "ProcessJsonsAuto (median %.3f s) is not faster than ProcessJsons (%.3f s)" % (auto_s, host_s)
device_s, device_all = timed(device_route)
assert not bool(d_status.any().item())
assert g.rules_from_bitmap(d_rows.cpu().numpy().view(np.uint32)) == [r["rules"] for r in want], "ProcessJsonsDevice differs from ProcessJsons"
leaves, leaf_bytes = g.last_batch()

# the kernels, in calls of their own (events between the launches)
kern = {}
L.gft_profile_enable(eh, 1)
for name in ("json_count", "json_scan", "json_write", "scan", "solve", "group_tags", "group_rules"):
    kern[name] = []
for _ in range(args.reps):
    L.gft_profile_reset(eh)
    device_route()
    for name in kern:
        a, n = C.c_double(), C.c_uint64()
        L.gft_profile_read(eh, name.encode(), C.byref(a), C.byref(n))
        kern[name].append(a.value)
paths_ms = []
for _ in range(args.reps):
    L.gft_profile_reset(eh)
    g.JsonPathsDevice(d_blob, d_off)
    a, n = C.c_double(), C.c_uint64()
    L.gft_profile_read(eh, b"json_paths", C.byref(a), C.byref(n))
    paths_ms.append(a.value)
L.gft_profile_enable(eh, 0)
kern_ms = {k: statistics.median(v) for k, v in kern.items()}
kern_ms["json_paths"] = statistics.median(paths_ms)

print(json.dumps({
    "row": "group finder: JSON batches", "docs": args.docs, "json_bytes": json_bytes, "leaves": leaves, "leaf_bytes": leaf_bytes,
    "rules": len(rules) * 2, "finder_expressions": len(exprs), "reps": args.reps,
    "ProcessJsons": {"median_s": host_s, "docs_per_s": args.docs / host_s, "all_s": host_all},
    "ProcessJsonsSchema": {"median_s": schema_s, "docs_per_s": args.docs / schema_s, "all_s": schema_all, "json_last": split},
    "ProcessJsonsAuto": {"median_s": auto_s, "docs_per_s": args.docs / auto_s, "all_s": auto_all, "json_last": auto_split, "auto_last": auto_last},
    "auto_faster_than_host": auto_s < host_s,
    "ProcessJsonsDevice": {"median_s": device_s, "docs_per_s": args.docs / device_s, "all_s": device_all},
    "schema_not_slower_than_host": schema_s <= host_s,
    "kernels_ms": kern_ms,
    "kernels_all_ms": {"json_count": kern["json_count"], "json_write": kern["json_write"], "json_paths": paths_ms},
    "json_paths_GBps": json_bytes / (kern_ms["json_paths"] * 1e-3) / 1e9 if kern_ms["json_paths"] else None,
    "json_count_GBps": json_bytes / (kern_ms["json_count"] * 1e-3) / 1e9 if kern_ms["json_count"] else None,
    "json_write_GBps": json_bytes / (kern_ms["json_write"] * 1e-3) / 1e9 if kern_ms["json_write"] else None}))
