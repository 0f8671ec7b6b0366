#!/usr/bin/env python3
"""Measurement of the rule result document written on the device (csrc/gft_result.hip), on the shape of tools/bench_group_json.py:
50 000 documents of about 4.2 KB with 8 string leaves, 1 000 finder expressions in 50 tags, 100 rule expressions in 50 rules.  One
process, one warm-up call per leg, then the median of --reps calls; only the C calls are timed, never json.loads.

    python tools/bench_group_result.py [--docs N] [--terms T] [--exprs E] [--reps R]
        one run of the library in use (GFT_LIBRARY, else the package's): gft_group_process_jsons_schema and _auto, the SHA-256 of
        their documents, gft_group_process_jsons_device; with a library that has the result calls also result_count / _scan / _fill
        from gft_profile_read in calls of their own, the fill's bytes per second, the text's size, the true rule expressions per
        document, and where a call's time goes, each part timed on its own: the upload of the blob, the device span on the
        resident blob (decode to rule rows, then the three result launches), the download of the text, the copy into the caller's
        buffer.  Prints one JSON line.

    python tools/bench_group_result.py --ab PARENT_LIBRARY [--runs 3]
        alternates --runs runs of this build and of a build of the parent commit, each in a process of its own, and asserts
        that every median of this build lies below the lowest of the parent's medians, for both calls, and that both builds
        return the same bytes.  Prints one JSON line with all medians and ranges.

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
ap.add_argument("--docs", type=int, default=50000)
ap.add_argument("--terms", type=int, default=10000)
ap.add_argument("--exprs", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ab", metavar="PARENT_LIBRARY")
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()


def ab():
    shape = ["--docs", str(args.docs), "--terms", str(args.terms), "--exprs", str(args.exprs), "--reps", str(args.reps)]
    runs = {"this": [], "parent": []}
    for _ in range(args.runs):
        for which in ("this", "parent"):
            env = dict(os.environ)
            env.pop("GFT_LIBRARY", None)
            if which == "parent":
                env["GFT_LIBRARY"] = os.path.abspath(args.ab)
            out = subprocess.run([sys.executable, os.path.abspath(__file__)] + shape, env=env, check=True, stdout=subprocess.PIPE).stdout
            runs[which].append(json.loads(out.decode().strip().splitlines()[-1]))
            print("%s: schema %.3f s, auto %.3f s" % (which, runs[which][-1]["schema"]["median_s"], runs[which][-1]["auto"]["median_s"]), file=sys.stderr, flush=True)
    res = {"row": "group finder: result documents, this build against the parent's", "runs": args.runs, "reps": args.reps}
    ok = True
    for call in ("schema", "auto"):
        mine = [r[call]["median_s"] for r in runs["this"]]
        theirs = [r[call]["median_s"] for r in runs["parent"]]
        same = len({r[call]["sha256"] for r in runs["this"] + runs["parent"]}) == 1
        faster = max(mine) < min(theirs)
        res[call] = {"this_medians_s": mine, "parent_medians_s": theirs,
                     "this_range_s": [min(min(r[call]["all_s"]) for r in runs["this"]), max(max(r[call]["all_s"]) for r in runs["this"])],
                     "parent_range_s": [min(min(r[call]["all_s"]) for r in runs["parent"]), max(max(r[call]["all_s"]) for r in runs["parent"])],
                     "identical_bytes": same, "every_median_below_the_parents_lowest": faster}
        ok = ok and same and faster
    for name in ("ProcessJsonsDevice_ms", "kernels_ms"):
        res[name] = {which: [r[name] for r in runs[which]] for which in runs}
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

# a build of the parent commit lacks the result calls: bind what it has
probe = C.CDLL(_lib.LIB_PATH)
HAVE_RESULT = hasattr(probe, "gft_group_rules_json_device")
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


def schema_route():
    rc = L.gft_group_process_jsons_schema(g._h, blob.ctypes.data, boff.ctypes.data, len(raws), C.cast(buf, C.c_void_p), cap, C.byref(need))
    assert rc == 0, L.gft_group_last_error(g._h)


def auto_route():
    rc = L.gft_group_process_jsons_auto(g._h, blob.ctypes.data, boff.ctypes.data, len(raws), None, 0, None, 0, C.cast(buf, C.c_void_p), cap, C.byref(need))
    assert rc == 0, L.gft_group_last_error(g._h)


def timed(fn, reps=None):
    fn()                                         # warm-up: engine build, buffers grown, pages touched
    times = []
    for _ in range(reps or args.reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def document():
    return C.string_at(C.addressof(buf), int(need.value) - 1)


out = {"row": "group finder: result documents", "library": _lib.LIB_PATH, "device_result": HAVE_RESULT and os.environ.get("GFT_DEVICE_RESULT") != "0",
       "docs": args.docs, "json_bytes": json_bytes, "rules": len(rules) * 2, "finder_expressions": len(exprs), "reps": args.reps}
for name, fn in (("schema", schema_route), ("auto", auto_route)):
    med, every = timed(fn)
    doc = document()
    out[name] = {"median_s": med, "all_s": every, "docs_per_s": args.docs / med, "bytes": len(doc), "sha256": hashlib.sha256(doc).hexdigest(),
                 "json_last": g.json_last()}
assert out["schema"]["sha256"] == out["auto"]["sha256"], "ProcessJsonsAuto's document differs from ProcessJsonsSchema's"

# the resident route: decode to rule rows (the path the result launches sit behind), its kernels in calls of their own
d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(64, dtype=np.uint8)])).cuda()
d_off = torch.from_numpy(boff.astype(np.int64)).cuda()
d_rows = torch.zeros((len(raws), g.rule_words()), dtype=torch.int32, device="cuda")
d_status = torch.zeros(len(raws), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()


def device_route():
    rc = L.gft_group_process_jsons_device(g._h, d_blob.data_ptr(), d_off.data_ptr(), len(raws), d_status.data_ptr(), d_rows.data_ptr())
    assert rc == 0, L.gft_group_last_error(g._h)


med, every = timed(device_route)
out["ProcessJsonsDevice_ms"] = {"median": med * 1e3, "all": [t * 1e3 for t in every]}
assert not bool(d_status.any().item())
rows = d_rows.cpu().numpy().view(np.uint32)
out["true_rule_expressions_per_document"] = float(np.unpackbits(rows.view(np.uint8), axis=1).sum()) / len(raws)


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


out["kernels_ms"] = kernels(device_route, ("json_count", "json_scan", "json_write", "scan", "solve", "group_tags", "group_rules"))

if HAVE_RESULT:
    total = C.c_uint64(0)
    d_out_off = torch.zeros(len(raws) + 1, dtype=torch.int64, device="cuda")
    rc = L.gft_group_rules_json_device(g._h, d_rows.data_ptr(), len(raws), None, None, 0, d_out_off.data_ptr(), C.byref(total))
    assert rc == 0, L.gft_group_last_error(g._h)
    d_text = torch.zeros(int(total.value) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def result_route():
        rc = L.gft_group_rules_json_device(g._h, d_rows.data_ptr(), len(raws), None, d_text.data_ptr(), int(total.value), d_out_off.data_ptr(),
                                           C.byref(total))
        assert rc == 0, L.gft_group_last_error(g._h)

    med, every = timed(result_route)
    text_bytes = int(total.value)
    assert bytes(d_text[:text_bytes].cpu().numpy()) == document(), "gft_group_rules_json_device differs from the schema call's document"
    out["RulesJsonDevice_ms"] = {"median": med * 1e3, "all": [t * 1e3 for t in every]}
    out["text_bytes"] = text_bytes
    out["result_kernels_ms"] = kernels(result_route, ("result_count", "result_scan", "result_fill"))
    fill = out["result_kernels_ms"]["result_fill"]["median"]
    out["result_fill_GBps"] = text_bytes / (fill * 1e-3) / 1e9 if fill else None
    # where a call's time goes, each part on its own (the call itself does them one after the other)
    host_text = np.empty(text_bytes, dtype=np.uint8)
    host_view = torch.from_numpy(host_text)
    dst = C.create_string_buffer(text_bytes + 1)

    def upload():
        torch.from_numpy(blob).cuda()
        torch.cuda.synchronize()

    def download():
        host_view.copy_(d_text[:text_bytes])
        torch.cuda.synchronize()

    def copy_out():
        C.memmove(dst, host_text.ctypes.data, text_bytes)

    def device_span():
        device_route()
        result_route()

    out["parts_ms"] = {name: {"median": m * 1e3, "all": [t * 1e3 for t in e]} for name, (m, e) in
                       (("upload_of_the_blob", timed(upload)), ("device_span_resident", timed(device_span)),
                        ("download_of_the_text", timed(download)), ("copy_into_the_callers_buffer", timed(copy_out)))}
print(json.dumps(out))
