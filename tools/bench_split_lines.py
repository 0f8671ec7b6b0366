#!/usr/bin/env python
"""What the offsets of a resident blob of lines cost: gft_split_lines_device (gft_split.hip) against the split on the host with
numpy that it replaces -- np.flatnonzero(blob == 10), plus the blank-line rule for JSON Lines --, in the same run on the same box.
Two blobs: JSON Lines made of the documents of tools/bench_group_json.py (the same generator, restated here), split with
GFT_SPLIT_JSON_LINES, and the plain text lines of the workload generator, split with GFT_SPLIT_AFTER_NL.  Per blob, medians of
--steps calls after --warmup:

  * the three launches from gft_profile_read in a pass of their own, and their share of the bound "the kernels' two reads of the
    text at the read ceiling measured here" (workload.read_ceiling_gbps, what bench.py --full reports);
  * the whole call (synchronous: wall clock), the blob's upload, the numpy split and the upload of its offsets;
  * the two routes to (resident blob, resident offsets): upload + device split, and numpy split + upload of blob and offsets.

For the JSON blob also GroupFinder.ProcessJsonLines against ProcessJsonsSchema over the pre-split list plus the numpy split it
replaces; their result documents must be equal.  Prints one JSON line and writes it to --out.

    python tools/bench_split_lines.py [--docs 200000] [--text-docs 1000000] [--steps 10] [--warmup 2] [--out profiles/split_lines_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def numpy_split(blob, json_lines):
    """the offsets on the host: what a caller does today in front of the device routes"""
    import numpy as np
    n = blob.size
    nl = np.flatnonzero(blob == 10)
    starts = np.concatenate([np.zeros(1, dtype=np.int64), nl + 1])
    if starts[-1] == n:
        starts = starts[:-1]
    if json_lines and starts.size:
        nonws = (blob != 32) & (blob != 9) & (blob != 10) & (blob != 13)
        seen = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(nonws, dtype=np.int64)])
        ends = np.concatenate([starts[1:], np.asarray([n], dtype=np.int64)])
        starts = starts[seen[ends] > seen[starts]]
        if starts.size:
            starts[0] = 0
    if not starts.size:
        return np.zeros(1, dtype=np.int64)
    return np.concatenate([starts, np.asarray([n], dtype=np.int64)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--text-docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "split_lines_bench.json"))
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 (the figures are medians)")

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_split_lines.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib, group
    from gofindthem_amd.engine import pack
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions, read_ceiling_gbps

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for i, e in enumerate(exprs):
        f.AddExpressionWithTag(e, "tag%d" % (i % 50))
    rules = {"rule%d" % i: ['"tag%d" and not "tag%d:Body"' % (i, (i + 7) % 50), '"tag%d:Meta" or "tag%d:Comments"' % ((i + 3) % 50, i)]
             for i in range(50)}
    g = group.NewFinderWithRules(f, rules)
    g.SetSchema(["Title", "Body.index(0)", "Body.index(1)", "Body.index(2)", "Meta.Author", "Meta.Notes.index(0)", "Comments.index(0).Text",
                 "Comments.index(1).Text"])

    def lines_of(n):
        text, off = w.docs_host(0, n)
        return [bytes(text[int(off[d]):int(off[d + 1])]).replace(b"\n", b" ") for d in range(n)]

    raws = []
    for d, t in enumerate(lines_of(args.docs)):
        t = t.decode("ascii")
        n = len(t) // 8
        p = [t[i * n:(i + 1) * n] for i in range(8)]
        raws.append(json.dumps({"Id": d, "Title": p[0], "Body": [p[1], p[2], p[3]], "Meta": {"Author": p[4], "Notes": [p[5]]},
                                "Comments": [{"Text": p[6], "Score": 3}, {"Text": p[7], "Score": 5}]}).encode())
    blobs = {"json_lines": (np.frombuffer(b"\n".join(raws) + b"\n", dtype=np.uint8), 1),
             "text_lines": (np.frombuffer(b"\n".join(lines_of(args.text_docs)) + b"\n", dtype=np.uint8), 0)}

    def median_ms(fn):
        times = []
        for step in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times)

    eh = f.engine_handle()
    results = {}
    for name, (blob, mode) in blobs.items():
        size = int(blob.size)
        padded = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
        want = numpy_split(blob, mode == 1)
        d_blob = torch.from_numpy(padded).cuda()
        d_off = torch.zeros(want.size, dtype=torch.int64, device="cuda")
        n = C.c_uint64(0)

        def device_split():
            assert L.gft_split_lines_device(eh, d_blob.data_ptr(), size, mode, d_off.data_ptr(), d_off.numel(), C.byref(n)) == 0

        device_split()
        assert int(n.value) + 1 == want.size and np.array_equal(d_off.cpu().numpy(), want), "the device split and the numpy split differ"
        split_ms = median_ms(device_split)
        assert L.gft_profile_enable(eh, 1) == 0
        for step in range(args.warmup + args.steps):
            if step == args.warmup:
                assert L.gft_profile_reset(eh) == 0
            device_split()
        launches = {}
        for cat in ("split_count", "split_scan", "split_write"):
            ms, cnt = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
            launches[cat] = {"ms": round(ms.value / max(cnt.value, 1), 4), "launches": int(cnt.value)}
        L.gft_profile_enable(eh, 0)
        ceiling = read_ceiling_gbps(d_blob)
        launch_ms = sum(v["ms"] for v in launches.values())
        bound_ms = 2 * size / (ceiling * 1e9) * 1e3
        numpy_ms = median_ms(lambda: numpy_split(blob, mode == 1))
        upload_blob_ms = median_ms(lambda: torch.from_numpy(padded).cuda())
        upload_off_ms = median_ms(lambda: torch.from_numpy(want).cuda())
        device_route, host_route = upload_blob_ms + split_ms, numpy_ms + upload_blob_ms + upload_off_ms
        results[name] = {
            "bytes": size, "documents": int(want.size) - 1, "mode": mode,
            "launches": launches, "launches_ms": round(launch_ms, 4),
            "read_ceiling_GBps": round(ceiling, 1), "bound_ms_2x_text_at_ceiling": round(bound_ms, 4),
            "fraction_of_bound": round(bound_ms / launch_ms, 4) if launch_ms > 0 else None,
            "device_split_call_ms": round(split_ms, 4), "numpy_split_ms": round(numpy_ms, 3),
            "upload_blob_ms": round(upload_blob_ms, 3), "upload_offsets_ms": round(upload_off_ms, 3),
            "route_upload_then_device_split_ms": round(device_route, 3), "route_numpy_split_then_upload_ms": round(host_route, 3),
            "device_route_is_faster": bool(device_route < host_route),
        }

    # ProcessJsonLines against ProcessJsonsSchema over the pre-split list, plus the host split it replaces
    blob = blobs["json_lines"][0]
    lblob, loff = pack(raws)                                 # (the list form: the documents without their newlines)
    cap = 2 * int(blob.size) + (1 << 16)
    buf = C.create_string_buffer(cap)
    need = C.c_uint64(0)

    def lines_call():
        assert L.gft_group_process_json_lines(g._h, blob.ctypes.data, blob.size, None, 0, None, 0, C.cast(buf, C.c_void_p), cap, C.byref(need)) == 0

    def schema_call():
        assert L.gft_group_process_jsons_schema(g._h, lblob.ctypes.data, loff.ctypes.data, len(raws), C.cast(buf, C.c_void_p), cap, C.byref(need)) == 0

    lines_call()
    lines_doc = buf.value
    schema_call()
    assert buf.value == lines_doc, "ProcessJsonLines and ProcessJsonsSchema give different result documents"
    lines_ms, schema_ms = median_ms(lines_call), median_ms(schema_call)
    split_ms = results["json_lines"]["numpy_split_ms"]
    results["process_json_lines"] = {
        "documents": len(raws), "ProcessJsonLines_ms": round(lines_ms, 3), "ProcessJsonsSchema_presplit_ms": round(schema_ms, 3),
        "numpy_split_ms": split_ms, "ProcessJsonsSchema_plus_split_ms": round(schema_ms + split_ms, 3),
        "lines_not_slower": bool(lines_ms <= schema_ms + split_ms), "json_last": list(g.json_last()),
    }
    out = {"tool": "bench_split_lines", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "text_docs": args.text_docs, "terms": args.terms, "exprs": args.exprs, "steps": args.steps,
                      "warmup": args.warmup},
           "results": results}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
