#!/usr/bin/env python3
"""Measurement of the tag result document written on the device (csrc/gft_tagdoc.hip), on the shape of tools/bench_group_tags.py:
documents of about 4.2 KB with 8 string leaves, 1 000 finder expressions in 50 tags.  A document's tag document is about 450 KB,
so the calls that return one run on --docs documents (500: what a build of the parent commit can serialise, about 224 MB).  One
process, one warm-up call per leg, then the median of --reps calls; only the C calls are timed, never json.loads.

    python tools/bench_group_tag_result.py [--docs N] [--path-docs P] [--big-docs B] [--terms T] [--exprs E] [--reps R]
        one run of the library in use (GFT_LIBRARY, else the package's): gft_group_tag_jsons_schema and _auto and the SHA-256 of
        their documents; on --path-docs documents the paths that exist in both builds (ProcessJsonsDevice, TagJsonsDevice,
        ProcessJsonsSchema); slots per tag, SW, result bytes per document and the fraction of the slot rows' bits that are set.
        With a library that has the tag document calls also: the kernels of a schema call from gft_profile_read (tagdoc_slots,
        _count, _scan, _fill beside the decode and the scan), tagdoc_fill's bytes per second, the upload of the blob, the download
        of the text and the copy into the caller's buffer each on its own, and one larger leg of --big-docs documents (0: none).
        Prints one JSON line.

    python tools/bench_group_tag_result.py --ab PARENT_LIBRARY [--runs 3] [--bench PARENT_TREE]
        alternates --runs runs of this build and of a build of the parent commit, each in a process of its own, and asserts that
        every median of this build lies below the lowest of the parent's medians, for both calls, that all runs return the same
        bytes, and that every median of this build on the existing paths lies inside the range of the parent's single calls.
        --bench: python bench.py --gpus 1 --steps 20 --warmup 3 alternated the same way -- this tree's, and the one of a built
        checkout of the parent commit in PARENT_TREE --, its value reported beside them.
        Prints one JSON line with all medians and ranges.

Not part of the bench.py contract."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=500)
ap.add_argument("--path-docs", type=int, default=5000)
ap.add_argument("--big-docs", type=int, default=0)
ap.add_argument("--terms", type=int, default=10000)
ap.add_argument("--exprs", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ab", metavar="PARENT_LIBRARY")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--bench", metavar="PARENT_TREE")
args = ap.parse_args()
PATHS = ("ProcessJsonsDevice", "TagJsonsDevice", "ProcessJsonsSchema")


def ab():
    shape = ["--docs", str(args.docs), "--path-docs", str(args.path_docs), "--terms", str(args.terms), "--exprs", str(args.exprs), "--reps", str(args.reps)]
    runs = {"this": [], "parent": []}
    bench = {"this": [], "parent": []}
    for k in range(args.runs):
        for which in ("this", "parent"):
            env = dict(os.environ)
            env.pop("GFT_LIBRARY", None)
            if which == "parent":
                env["GFT_LIBRARY"] = os.path.abspath(args.ab)
            big = ["--big-docs", str(args.big_docs)] if which == "this" and k == args.runs - 1 else []
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + shape + big, env=env, check=True, stdout=subprocess.PIPE).stdout
            runs[which].append(json.loads(out.decode().strip().splitlines()[-1]))
            print("%s: schema %.4f s, auto %.4f s" % (which, runs[which][-1]["schema"]["median_s"], runs[which][-1]["auto"]["median_s"]), file=sys.stderr, flush=True)
            if args.bench:
                tree = ROOT if which == "this" else os.path.abspath(args.bench)
                env.pop("GFT_LIBRARY", None)
                out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], env=env, check=True,
                                     stdout=subprocess.PIPE, cwd=tree).stdout
                bench[which].append(json.loads(out.decode().strip().splitlines()[-1])["value"])
                print("%s: bench.py %.0f" % (which, bench[which][-1]), file=sys.stderr, flush=True)
    res = {"row": "group finder: tag result documents, this build against the parent's", "runs": args.runs, "reps": args.reps, "docs": args.docs}
    ok = True
    for call in ("schema", "auto"):
        mine = [r[call]["median_s"] for r in runs["this"]]
        theirs = [r[call]["median_s"] for r in runs["parent"]]
        same = len({r[c]["sha256"] for r in runs["this"] + runs["parent"] for c in ("schema", "auto")}) == 1
        faster = max(mine) < min(theirs)
        res[call] = {"this_medians_s": mine, "parent_medians_s": theirs, "factor": statistics.median(theirs) / statistics.median(mine),
                     "identical_bytes": same, "every_median_below_the_parents_lowest": faster}
        ok = ok and same and faster
    inside = True
    for name in PATHS:
        mine = [r["paths_ms"][name]["median"] for r in runs["this"]]
        single = [t for r in runs["parent"] for t in r["paths_ms"][name]["all"]]
        within = all(min(single) <= m <= max(single) for m in mine)
        res[name] = {"this_medians_ms": mine, "parent_medians_ms": [r["paths_ms"][name]["median"] for r in runs["parent"]],
                     "parent_single_calls_ms": [min(single), max(single)], "inside_the_parents_range": within}
        inside = inside and within
    if args.bench:
        res["bench_py"] = {"this": bench["this"], "parent": bench["parent"],
                           "inside_the_parents_range": all(min(bench["parent"]) <= v <= max(bench["parent"]) for v in bench["this"]),
                           "not_below_the_parents_lowest": min(bench["this"]) >= min(bench["parent"])}       # (documents/s: higher is faster)
    res["existing_paths_inside_the_parents_range"] = inside
    res["this_build"] = runs["this"][-1]
    print(json.dumps(res))
    assert ok, "this build is not below the parent's lowest median in both calls, or the documents differ"


if args.ab:
    ab()
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gofindthem_amd import _lib, group  # noqa: E402
from gofindthem_amd.engine import pack  # noqa: E402
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402
from gofindthem_amd.workload import Workload, make_expressions  # noqa: E402

# a build of the parent commit lacks the tag document calls: bind what it has
probe = C.CDLL(_lib.LIB_PATH)
HAVE_TAGDOC = hasattr(probe, "gft_group_tags_json_device")
for name in [n for n in _lib.SYMBOLS if not hasattr(probe, n)]:
    del _lib.SYMBOLS[name]

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
L = _lib.load()
eh = f.engine_handle()
n_all = max(args.docs, args.path_docs, args.big_docs)
text, off = w.docs_host(0, n_all)
raws = []
for d in range(n_all):
    t = bytes(text[int(off[d]):int(off[d + 1])]).decode("ascii")
    n = len(t) // 8
    p = [t[i * n:(i + 1) * n] for i in range(8)]
    raws.append(json.dumps({"Id": d, "Title": p[0], "Body": [p[1], p[2], p[3]], "Meta": {"Author": p[4], "Notes": [p[5]]},
                            "Comments": [{"Text": p[6], "Score": 3}, {"Text": p[7], "Score": 5}]}).encode())
blob, boff = pack(raws)
need = C.c_uint64(0)
state = {"buf": C.create_string_buffer(1 << 20), "cap": 1 << 20}


def ok(rc):
    """(the warm-up call sizes the buffer for the timed ones: the library kept the document, it is fetched, not made again)"""
    assert rc == 0 or (rc == _lib.GFT_E_INVALID and need.value > state["cap"]), L.gft_group_last_error(g._h)
    if need.value > state["cap"]:
        state["cap"] = int(need.value) + (1 << 16)
        state["buf"] = C.create_string_buffer(state["cap"])
        assert L.gft_group_last_result(g._h, C.cast(state["buf"], C.c_void_p), state["cap"], C.byref(need)) == 0


def schema_route(n=None):
    ok(L.gft_group_tag_jsons_schema(g._h, blob.ctypes.data, boff.ctypes.data, n or args.docs, C.cast(state["buf"], C.c_void_p), state["cap"], C.byref(need)))


def auto_route():
    ok(L.gft_group_tag_jsons_auto(g._h, blob.ctypes.data, boff.ctypes.data, args.docs, None, 0, None, 0, C.cast(state["buf"], C.c_void_p), state["cap"],
                                  C.byref(need)))


def rules_schema_route():
    ok(L.gft_group_process_jsons_schema(g._h, blob.ctypes.data, boff.ctypes.data, args.path_docs, C.cast(state["buf"], C.c_void_p), state["cap"], C.byref(need)))


def timed(fn, reps=None):
    fn()                                         # warm-up: engine build, buffers grown, pages touched
    times = []
    for _ in range(reps or args.reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def document():
    return C.string_at(C.addressof(state["buf"]), int(need.value) - 1)


out = {"row": "group finder: tag result documents", "library": _lib.LIB_PATH, "device_result": HAVE_TAGDOC and os.environ.get("GFT_DEVICE_RESULT") != "0",
       "docs": args.docs, "json_bytes": int(boff[args.docs]), "finder_expressions": len(exprs), "reps": args.reps}
for name, fn in (("schema", schema_route), ("auto", auto_route)):
    med, every = timed(fn)
    doc = document()
    out[name] = {"median_s": med, "all_s": every, "docs_per_s": args.docs / med, "bytes": len(doc), "sha256": hashlib.sha256(doc).hexdigest(),
                 "json_last": g.json_last()}
assert out["schema"]["sha256"] == out["auto"]["sha256"], "TagJsonsAuto's document differs from TagJsonsSchema's"
text_bytes = out["schema"]["bytes"]

# ---- what nobody has counted: the slots, and how full the slot rows are
per_tag = {}
for e, t in zip(exprs, tags):
    per_tag.setdefault(t, set()).add(e)
SW = sum((len(v) + 31) // 32 for v in per_tag.values())
P = args.path_docs
d_blob = torch.from_numpy(np.concatenate([blob[:int(boff[P])], np.zeros(64, dtype=np.uint8)])).cuda()
d_off = torch.from_numpy(boff[:P + 1].astype(np.int64)).cuda()
d_rows = torch.zeros((P, g.rule_words()), dtype=torch.int32, device="cuda")
d_status = torch.zeros(P, dtype=torch.uint8, device="cuda")
d_row_off = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
total = C.c_uint64(0)
torch.cuda.synchronize()
assert L.gft_group_tag_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), P, d_status.data_ptr(), d_row_off.data_ptr(), None, None, None, 0,
                                    C.byref(total)) == 0, L.gft_group_last_error(g._h)
n_entries = int(total.value)
leaves, _ = g.last_batch()
d_ent = [torch.zeros(n_entries + 8, dtype=torch.int32, device="cuda") for _ in range(3)]
torch.cuda.synchronize()
# (every (tag, expression string) pair is one expression here: an entry is a set slot bit)
assert sum(len(v) for v in per_tag.values()) == len(exprs)
out["slots"] = {"tags": len(per_tag), "slots_per_tag": [min(len(v) for v in per_tag.values()), max(len(v) for v in per_tag.values())], "SW": SW,
                "result_bytes_per_document": text_bytes / args.docs, "entries_per_document": n_entries / P,
                "slot_row_bits_set": n_entries / (leaves * SW * 32.0), "slot_rows_bytes": leaves * SW * 4}


def device_rules():
    rc = L.gft_group_process_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), P, d_status.data_ptr(), d_rows.data_ptr())
    assert rc == 0, L.gft_group_last_error(g._h)


def device_tags():
    rc = L.gft_group_tag_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), P, d_status.data_ptr(), d_row_off.data_ptr(), d_ent[0].data_ptr(),
                                      d_ent[1].data_ptr(), d_ent[2].data_ptr(), n_entries, C.byref(total))
    assert rc == 0, L.gft_group_last_error(g._h)


out["path_docs"] = P
out["paths_ms"] = {}
for name, fn in zip(PATHS, (device_rules, device_tags, rules_schema_route)):
    med, every = timed(fn)
    out["paths_ms"][name] = {"median": med * 1e3, "all": [t * 1e3 for t in every]}


def kernels(fn, names):
    got = {k: [] for k in names}
    L.gft_profile_enable(eh, 1)
    for _ in range(args.reps):
        L.gft_profile_reset(eh)
        fn()
        for k in names:
            a, n = C.c_double(), C.c_uint64()
            L.gft_profile_read(eh, k.encode(), C.byref(a), C.byref(n))
            got[k].append(a.value)
    L.gft_profile_reset(eh)
    L.gft_profile_enable(eh, 0)
    return {k: {"median": statistics.median(v), "all": v} for k, v in got.items()}


if HAVE_TAGDOC:
    schema_route()
    names = ("json_count", "json_scan", "json_write", "scan", "solve", "tagdoc_slots", "tagdoc_count", "tagdoc_scan", "tagdoc_fill")
    out["kernels_ms"] = kernels(schema_route, names)
    fill = out["kernels_ms"]["tagdoc_fill"]["median"]
    out["tagdoc_fill_GBps"] = text_bytes / (fill * 1e-3) / 1e9 if fill else None
    out["device_span_ms"] = sum(v["median"] for v in out["kernels_ms"].values())
    # where else a call's time goes, each part on its own (the call itself does them one after the other)
    sub = blob[:int(boff[args.docs])]
    d_text = torch.zeros(text_bytes, dtype=torch.uint8, device="cuda")
    host_text = np.empty(text_bytes, dtype=np.uint8)
    host_view = torch.from_numpy(host_text)
    dst = C.create_string_buffer(text_bytes + 1)

    def upload():
        torch.from_numpy(sub).cuda()
        torch.cuda.synchronize()

    def download():
        host_view.copy_(d_text)
        torch.cuda.synchronize()

    def copy_out():
        C.memmove(dst, host_text.ctypes.data, text_bytes)

    out["parts_ms"] = {name: {"median": m * 1e3, "all": [t * 1e3 for t in e]} for name, (m, e) in
                       (("upload_of_the_blob", timed(upload)), ("download_of_the_text", timed(download)), ("copy_into_the_callers_buffer", timed(copy_out)))}
    if args.big_docs:
        del d_text, host_view, host_text, dst
        med, every = timed(lambda: schema_route(args.big_docs), reps=3)
        big_bytes = int(need.value) - 1
        out["big"] = {"docs": args.big_docs, "median_s": med, "all_s": every, "bytes": big_bytes, "json_last": g.json_last(),
                      "kernels_ms": kernels(lambda: schema_route(args.big_docs), names)}
        fill = out["big"]["kernels_ms"]["tagdoc_fill"]["median"]
        out["big"]["tagdoc_fill_GBps"] = big_bytes / (fill * 1e-3) / 1e9 if fill else None
print(json.dumps(out))
