#!/usr/bin/env python3
"""Measurement of the group finder's ways to the tags of a batch of JSON documents, in one process, on the shape of
tools/bench_group_json.py (50 000 documents of about 4.2 KB with 8 string leaves, 1 000 finder expressions in 50 tags):

    TagJsons             the JSON reader and the walk on host threads, the leaf bitmap turned into maps bit by bit (the baseline)
    TagJsonsSchema       host memory in, the documents decoded and tagged on the device (csrc/gft_json.hip, csrc/gft_tags.hip)
    TagJsonsAuto         as TagJsonsSchema without SetSchema: the schema is discovered from the batch on the device
    TagJsonsDevice       the blob resident in HBM; status and the entries stay there
    ProcessJsonsDevice   the rule route on the same blob, for scale

In this shape a document has about 2 160 tag entries, and an expression string about 170 bytes: the result document of the three
calls that build one is about 450 KB per input document, 22 GB for the whole batch.  Those three legs therefore run on the first
--map-docs documents of the batch (one sub-batch, the same for all three); the two device legs run on all of it.  Identical tag
maps are asserted on the sub-batch, for the device leg from the entries of its first --map-docs rows.  One warm-up call each,
then the median of --reps calls; the kernel times come from gft_profile_read in calls of their own.  Not part of the bench.py
contract.

    python tools/bench_group_tags.py [--docs N] [--map-docs M] [--terms T] [--exprs E] [--reps R]
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
ap.add_argument("--map-docs", type=int, default=500)
ap.add_argument("--terms", type=int, default=10000)
ap.add_argument("--exprs", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
M = min(args.map_docs, args.docs)


def stage(what):
    print("[bench_group_tags] %s" % what, file=sys.stderr, flush=True)


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
sub_bytes = int(boff[M])                   # the sub-batch of the legs that build a result document: the first M documents
cap = 1 << 20
buf = C.create_string_buffer(cap)
need = C.c_uint64(0)


def result():
    """the result document of the last host-pointer call"""
    return json.loads(buf.value.decode())


def ok(rc):
    global buf, cap
    assert rc == 0 or (rc == _lib.GFT_E_INVALID and need.value > cap), L.gft_group_last_error(g._h)
    if need.value > cap:                         # (the warm-up call sizes the buffer for the timed ones)
        cap = int(need.value) + (1 << 16)
        buf = C.create_string_buffer(cap)
        assert L.gft_group_last_result(g._h, C.cast(buf, C.c_void_p), cap, C.byref(need)) == 0


def host_route():
    ok(L.gft_group_process_jsons(g._h, blob.ctypes.data, boff.ctypes.data, M, None, 0, None, 0, 1, C.cast(buf, C.c_void_p), cap, C.byref(need)))


def schema_route():
    ok(L.gft_group_tag_jsons_schema(g._h, blob.ctypes.data, boff.ctypes.data, M, C.cast(buf, C.c_void_p), cap, C.byref(need)))


def auto_route():
    ok(L.gft_group_tag_jsons_auto(g._h, blob.ctypes.data, boff.ctypes.data, M, None, 0, None, 0, C.cast(buf, C.c_void_p), cap, C.byref(need)))


d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(64, dtype=np.uint8)])).cuda()
d_off = torch.from_numpy(boff.astype(np.int64)).cuda()
d_rows = torch.zeros((len(raws), g.rule_words()), dtype=torch.int32, device="cuda")
d_status = torch.zeros(len(raws), dtype=torch.uint8, device="cuda")
d_row_off = torch.zeros(len(raws) + 1, dtype=torch.int64, device="cuda")
total = C.c_uint64(0)
torch.cuda.synchronize()
stage("batch built: %d documents, %d bytes; counting the entries" % (len(raws), json_bytes))
# the entries of the batch, counted once: the arrays of the timed calls have that size
assert L.gft_group_tag_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), len(raws), d_status.data_ptr(), d_row_off.data_ptr(), None, None, None,
                                    0, C.byref(total)) == 0, L.gft_group_last_error(g._h)
n_entries = int(total.value)
d_ent = [torch.zeros(n_entries + 8, dtype=torch.int32, device="cuda") for _ in range(3)]
torch.cuda.synchronize()


def device_tags():
    rc = L.gft_group_tag_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), len(raws), d_status.data_ptr(), d_row_off.data_ptr(),
                                      d_ent[0].data_ptr(), d_ent[1].data_ptr(), d_ent[2].data_ptr(), n_entries, C.byref(total))
    assert rc == 0, L.gft_group_last_error(g._h)


def device_rules():
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


stage("%d entries; TagJsons on %d documents" % (n_entries, M))
host_s, host_all = timed(host_route)
want = result()
result_bytes = int(need.value)
stage("TagJsonsSchema")
schema_s, schema_all = timed(schema_route)
split = g.json_last()
assert result() == want, "TagJsonsSchema differs from TagJsons"
stage("TagJsonsAuto")
auto_s, auto_all = timed(auto_route)
auto_split, auto_last = g.json_last(), g.json_auto_last()
assert result() == want, "TagJsonsAuto differs from TagJsons"
stage("TagJsonsDevice on %d documents" % len(raws))
dtags_s, dtags_all = timed(device_tags)
assert not bool(d_status.any().item()) and int(total.value) == n_entries
row_off = d_row_off.cpu().numpy()
assert int(row_off[-1]) == n_entries
sub_entries = int(row_off[M])
maps = g.tags_from_entries(row_off[:M + 1], d_ent[0][:sub_entries].cpu().numpy(), d_ent[1][:sub_entries].cpu().numpy())
assert maps == [r["tags"] for r in want], "TagJsonsDevice differs from TagJsons"
stage("ProcessJsonsDevice")
drules_s, drules_all = timed(device_rules)
leaves, leaf_bytes = g.last_batch()

stage("kernel times")
# the kernels, in calls of their own (events between the launches)
names = ("json_count", "json_scan", "json_write", "scan", "solve", "tags_count", "tags_scan", "tags_fill")
kern = {name: [] for name in names}
L.gft_profile_enable(eh, 1)
for _ in range(args.reps):
    L.gft_profile_reset(eh)
    device_tags()
    for name in kern:
        a, n = C.c_double(), C.c_uint64()
        L.gft_profile_read(eh, name.encode(), C.byref(a), C.byref(n))
        kern[name].append(a.value)
L.gft_profile_enable(eh, 0)
kern_ms = {k: statistics.median(v) for k, v in kern.items()}
bitmap_bytes = leaves * ((len(exprs) + 31) // 32) * 4
# what TagJsonsSchema fetches for its sub-batch: status, row_off, two entry columns; beside the dense leaf bitmap of the same documents
bytes_down = M + (M + 1) * 8 + 2 * sub_entries * 4
sub_bitmap_bytes = 8 * M * ((len(exprs) + 31) // 32) * 4

print(json.dumps({
    "row": "group finder: tags of JSON batches", "docs": args.docs, "json_bytes": json_bytes, "leaves": leaves, "leaf_bytes": leaf_bytes,
    "finder_expressions": len(exprs), "tags": 50, "reps": args.reps, "entries": n_entries, "entries_per_doc": n_entries / args.docs,
    "leaf_bitmap_bytes": bitmap_bytes, "entry_bytes": 3 * n_entries * 4 + (len(raws) + 1) * 8,
    "map_docs": M, "map_json_bytes": sub_bytes, "map_entries": sub_entries, "map_result_document_bytes": result_bytes,
    "map_bytes_down": bytes_down, "map_leaf_bitmap_bytes": sub_bitmap_bytes,
    "TagJsons": {"median_s": host_s, "docs_per_s": M / host_s, "all_s": host_all},
    "TagJsonsSchema": {"median_s": schema_s, "docs_per_s": M / schema_s, "all_s": schema_all, "json_last": split},
    "TagJsonsAuto": {"median_s": auto_s, "docs_per_s": M / auto_s, "all_s": auto_all, "json_last": auto_split, "auto_last": auto_last},
    "TagJsonsDevice": {"median_s": dtags_s, "docs_per_s": args.docs / dtags_s, "all_s": dtags_all},
    "ProcessJsonsDevice": {"median_s": drules_s, "docs_per_s": args.docs / drules_s, "all_s": drules_all},
    "schema_faster_than_host": schema_s < host_s,
    "kernels_ms": kern_ms,
    "kernels_all_ms": {k: kern[k] for k in ("tags_count", "tags_scan", "tags_fill", "json_count", "json_write")},
    "tags_count_bitmap_GBps": bitmap_bytes / (kern_ms["tags_count"] * 1e-3) / 1e9 if kern_ms["tags_count"] else None,
    "tags_fill_GBps": (bitmap_bytes + 3 * n_entries * 4) / (kern_ms["tags_fill"] * 1e-3) / 1e9 if kern_ms["tags_fill"] else None}))
