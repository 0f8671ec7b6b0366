#!/usr/bin/env python
"""What saying where the expressions matched costs: gft_hit_spans_device (gft_spans.hip) against gft_scan_device alone on the same
batch -- the scan is existing code, the three added launches are the difference --, gft_redact_spans_device against a plain
device-to-device copy of the masked bytes' volume, and Finder.RedactLines against the host route it replaces.

  (a) the headline corpus of bench.py (--docs documents of about 4 KB, --terms terms, --exprs expressions), rows from the real finder;
  (b) the same text cut into lines (one document per line of about 100 bytes): many documents, few matches each -- the shape on
      which the per-lane document search of span_mark (a binary search over n_docs + 1 offsets per match) is deepest.

Per shape: both calls alternate in the same run (host clock round calls that end in a stream synchronise; medians over the repeats
that fill a window of --window seconds), the launches' own times from gft_profile_read ("span_mark", "span_scan", "span_place",
"redact_fill"), the matches and the spans kept.  span_mark holds the document search: its time per match on (b) against (a) is what
the search costs as the offsets array grows.  Then the number a user sees: Finder.RedactLines over --lines lines from host memory
against gft_scan from host memory, the join of the match list with the rows and the witness sets in Python, and the masking of a
bytearray.  No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_spans.py [--docs 200000] [--lines 20000] [--out profiles/spans_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LAUNCHES = ("span_mark", "span_scan", "span_place")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per shape")
    ap.add_argument("--out", default=os.path.join("profiles", "spans_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_spans.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(exprs)
    eh = f.engine_handle()
    E = f.n_expressions
    W = (E + 31) // 32

    def read(cat):
        ms, cnt = C.c_double(), C.c_uint64()
        assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
        return ms.value / max(cnt.value, 1)

    def measure(text, off):
        n = int(off.numel()) - 1
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())
        so, st, ln, tm = _spans(text, off, bm)
        total = int(st.numel())
        m = _lib.GftMatches()
        tot = C.c_uint64(0)

        def scan():
            assert L.gft_scan_device(eh, text.data_ptr(), off.data_ptr(), n, _lib.GFT_FOLD_ASCII, C.byref(m)) == 0

        def spans():
            assert L.gft_hit_spans_device(eh, text.data_ptr(), off.data_ptr(), n, _lib.GFT_FOLD_ASCII, bm.data_ptr(), None, None, so.data_ptr(),
                                          st.data_ptr(), ln.data_ptr(), tm.data_ptr(), total, C.byref(tot)) == 0
        masked = int(ln.sum().item())
        clone = text.clone()
        src = torch.empty(max(masked, 1), dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty_like(src)

        def redact():
            assert L.gft_redact_spans_device(eh, clone.data_ptr(), off.data_ptr(), n, so.data_ptr(), st.data_ptr(), ln.data_ptr(), 42) == 0

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()
        for fn in (scan, spans, redact, copy) * 2:                  # warm-up: buffers grown, clocks up
            fn()
        torch.cuda.synchronize()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        times = {"scan": [], "spans": [], "redact": [], "copy": []}
        t0 = time.perf_counter()
        while len(times["scan"]) < 5 or time.perf_counter() - t0 < args.window:
            for name, fn in (("scan", scan), ("spans", spans), ("redact", redact), ("copy", copy)):
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - a) * 1e3)
        res = {"documents": n, "text_bytes": int(off[-1].item() - off[0].item()), "matches": int(m.n_matches), "spans": total, "masked_bytes": masked,
               "repeats": len(times["scan"])}
        for name, v in times.items():
            res[name + "_call_ms"] = round(statistics.median(v), 4)
        for cat in LAUNCHES + ("redact_fill", "scan"):
            res[cat + "_ms"] = round(read(cat), 4)
        L.gft_profile_enable(eh, 0)
        res["spans_over_scan"] = round(res["spans_call_ms"] / res["scan_call_ms"], 3)
        res["added_launches_ms"] = round(sum(res[c + "_ms"] for c in LAUNCHES), 4)
        res["span_mark_ns_per_match"] = round(res["span_mark_ms"] * 1e6 / max(res["matches"], 1), 3)
        res["redact_over_copy"] = round(res["redact_call_ms"] / res["copy_call_ms"], 3)
        return res

    def _spans(text, off, bm):
        from gofindthem_amd.engine import hit_spans_tensor
        return hit_spans_tensor(lambda t, o, n, *a: _ok(L.gft_hit_spans_device(eh, t, o, n, _lib.GFT_FOLD_ASCII, *a)), text, off, bm, E, None, None)

    def _ok(rc):
        assert rc == 0, L.gft_last_error(eh)

    shapes = {}
    text, off = w.docs_device(0, args.docs)
    shapes["a: documents of 4 KB"] = measure(text, off)
    # (b) the same bytes, a document per line of about 100 bytes: every 100th byte becomes a newline, the split makes the offsets
    n_bytes = int(off[-1].item())
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    shapes["b: lines of 100 bytes"] = measure(lined, loff)
    del text, off, lined, loff
    torch.cuda.empty_cache()

    # the number a user sees
    t, o = w.docs_host(0, max(args.lines // 40, 1))
    a = np.array(t[:int(o[-1])], dtype=np.uint8)
    a[a == 10] = 32
    a[99::100] = 10
    data = a.tobytes()[:args.lines * 100]

    def host_route():
        from gofindthem_amd.engine import split_lines_host
        n, doff = split_lines_host(data, 0)
        doff = doff[:n + 1]
        rows = f.ProcessTexts(blob=np.frombuffer(data + b"\0" * 64, dtype=np.uint8), doc_off=doff)
        low = data.lower()
        eng = host_route.eng
        moff, tid, pos = eng.scan(np.frombuffer(low + b"\0" * 64, dtype=np.uint8), doff)
        out = bytearray(data)
        wit = host_route.wit
        moff, tid, pos, doff = moff.tolist(), tid.tolist(), pos.tolist(), doff.tolist()
        for d in range(n):
            row = int.from_bytes(rows[d].tobytes(), "little")
            for k in range(moff[d], moff[d + 1]):
                if wit[tid[k]] & row:
                    s = doff[d] + pos[k]
                    out[s:s + host_route.lens[tid[k]]] = b"*" * host_route.lens[tid[k]]
        return bytes(out)
    # the host route's own tables: an engine over the finder's keywords, and per term the expressions it is a witness of (a walk
    # over the finder's trees: the keyword units outside every NOT) as one integer
    from gofindthem_amd.engine import Engine
    host_route.eng = Engine()
    host_route.eng.build(sorted(k if isinstance(k, bytes) else k.encode() for k in f.GetKeywords()))
    terms = host_route.eng.terms()
    host_route.lens = [len(k) for k in terms]
    tid_of = {k: i for i, k in enumerate(terms)}
    wit = [0] * len(terms)
    for i in range(E):
        stack = [f.expression(i)[2]]
        while stack:
            n = stack.pop()
            if n["Type"] == "UNIT":
                lit = n.get("Literal", "").encode()
                if lit in tid_of:
                    wit[tid_of[lit]] |= 1 << i
            elif n["Type"] != "NOT":
                stack += [n[k] for k in ("LExpr", "RExpr") if k in n]
    host_route.wit = wit

    def timed(fn, reps=3):
        best, r = None, None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        return best, r
    dev_ms, got = timed(lambda: f.RedactLines(data))
    host_ms, ref = timed(host_route)
    end_to_end = {"lines": data.count(b"\n"), "bytes": len(data), "RedactLines_ms": round(dev_ms, 2), "host_scan_python_join_bytearray_ms": round(host_ms, 2),
                  "same_bytes": bool(got[0] == ref), "lowered": bool(got[1]), "masked_bytes": got[0].count(b"*") - data.count(b"*")}
    out = {"tool": "bench_spans", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "lines": args.lines, "terms": args.terms, "exprs": args.exprs, "window_s": args.window},
           "shapes": shapes, "end_to_end": end_to_end}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
