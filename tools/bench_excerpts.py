#!/usr/bin/env python
"""What the excerpts round the hits cost: gft_excerpt_spans_device (gft_excerpt.hip and the select's copy kernel) against the two
routes to the same text that were there before -- gft_select_docs_device of the documents that hit (whole documents come down),
and the host route (Finder.SpansLines, then slicing the text on the host, which the caller must still hold) --, with the bytes
that cross the link on each route.

  (a) the calls, two shapes: the headline corpus of bench.py (--docs documents of about 4 KB), and the same text cut into lines of
      about 100 bytes.  before = after = 40.  The excerpt call and the select alternate in the same run (host clock round calls
      that end in a stream synchronise, the fill call into tensors of the counted sizes; medians over the repeats that fill a
      window of --window seconds), with the stages' own times from gft_profile_read per call.
  (b) the whole finder call over --lines lines from host memory: Finder.ExcerptLines against Finder.SpansLines(source=True) plus
      slicing and merging on the host in Python, and against Finder.SelectLines.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_excerpts.py [--docs 200000] [--lines 20000] [--out profiles/excerpts_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

EXC_STAGES = ("excerpt_window", "excerpt_smin", "excerpt_scan", "excerpt_place", "excerpt_copy")
SEL_STAGES = ("select_mark", "select_scan", "select_place", "select_copy")
REACH = 40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per shape")
    ap.add_argument("--out", default=os.path.join("profiles", "excerpts_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_excerpts.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(exprs)
    eh = f.engine_handle()
    W = (f.n_expressions + 31) // 32

    def read_total(cat):
        ms, cnt = C.c_double(), C.c_uint64()
        assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
        return ms.value

    def measure(text, off):
        n = int(off.numel()) - 1
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())
        so, st, ln, tm, lowered = f.SpansDevice(text, off, bm)
        assert not lowered
        ex = f.ExcerptsDevice(text, off, so, st, ln, False, False, REACH, REACH)
        out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off = ex[:7]
        m, nb = int(exc_doc.numel()), int(out.numel())
        sel, sel_off, sel_idx = f.SelectDevice(text, off, bm)
        sm, sb = int(sel_idx.numel()), int(sel.numel())
        cm, ct = C.c_uint64(0), C.c_uint64(0)

        def excerpt():
            assert L.gft_excerpt_spans_device(eh, text.data_ptr(), off.data_ptr(), n, so.data_ptr(), st.data_ptr(), ln.data_ptr(), REACH, REACH, 1,
                                              out.data_ptr(), nb, exc_off.data_ptr(), exc_doc.data_ptr(), exc_start.data_ptr(), exc_span_off.data_ptr(),
                                              m, span_rel.data_ptr(), doc_exc_off.data_ptr(), C.byref(cm), C.byref(ct)) == 0

        def select():
            assert L.gft_select_docs_device(eh, text.data_ptr(), off.data_ptr(), n, bm.data_ptr(), f.n_expressions, None, 0, None, sel.data_ptr(), sb,
                                            sel_off.data_ptr(), sel_idx.data_ptr(), sm, C.byref(cm), C.byref(ct)) == 0
        for _ in range(2):                                          # warm-up: buffers grown, clocks up
            excerpt()
            select()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        times = {"excerpt": [], "select": []}
        t0 = time.perf_counter()
        while len(times["excerpt"]) < 5 or time.perf_counter() - t0 < args.window:
            for name, fn in (("excerpt", excerpt), ("select", select)):
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - a) * 1e3)
        reps = len(times["excerpt"])
        n_spans = int(st.numel())
        res = {"documents": n, "text_bytes": int(off[-1].item() - off[0].item()), "documents_hit": sm, "spans": n_spans, "excerpts": m,
               "excerpt_bytes": nb, "repeats": reps}
        for name, v in times.items():
            res[name + "_call_ms"] = round(statistics.median(v), 4)
        for cat in EXC_STAGES + SEL_STAGES:
            res[cat + "_ms"] = round(read_total(cat) / reps, 4)
        L.gft_profile_enable(eh, 0)
        res["excerpt_over_select"] = round(res["excerpt_call_ms"] / res["select_call_ms"], 3)
        # what comes down on each route to the text round the hits
        res["link_bytes_excerpt_route"] = nb + (m + 1) * 8 * 2 + m * 12 + n_spans * 12       # blob; exc_off, exc_span_off; doc, start; rel, len, term
        res["link_bytes_select_route"] = sb + (sm + 1) * 8 + sm * 8 + (n + 1) * 8 + n_spans * 12   # documents; out_off; doc_idx; span_off; spans
        res["link_bytes_host_route"] = (n + 1) * 8 + n * W * 4 + n_spans * 12                # offsets, rows, spans -- and the text stays on the host
        return res

    shapes = {}
    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    shapes["a1: documents of 4 KB"] = measure(text, off)
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    shapes["a2: lines of 100 bytes"] = measure(lined, loff)
    del text, off, lined, loff
    torch.cuda.empty_cache()

    # (b): the numbers a user sees
    t, o = w.docs_host(0, max(args.lines // 40, 1))
    a = np.array(t[:int(o[-1])], dtype=np.uint8)
    a[a == 10] = 32
    a[99::100] = 10
    data = a[:args.lines * 100].tobytes()

    def host_route():
        idx, spans, _ = f.SpansLines(data, source=True)
        lines = data.split(b"\n")
        res = []
        for d, sp in zip(idx.tolist(), spans):
            line = lines[d] + b"\n"
            per = []
            for s, e, kw in sp:
                lo, hi = max(0, s - REACH), min(len(line), e + REACH)
                for _ in range(3):
                    if 0 < lo < len(line) and (line[lo] & 0xC0) == 0x80:
                        lo -= 1
                    if hi < len(line) and (line[hi] & 0xC0) == 0x80:
                        hi += 1
                per.append((lo, hi, s, e, kw))
            per.sort(key=lambda x: x[:2])
            merged = []
            for lo, hi, s, e, kw in per:
                if merged and lo <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], hi)
                    merged[-1][2].append((s, e, kw))
                else:
                    merged.append([lo, hi, [(s, e, kw)]])
            res.append([(lo, line[lo:hi], hits) for lo, hi, hits in merged])
        return idx, res

    def timed(fn, reps=5):
        v, r = [], None
        fn()                                                        # warm-up
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(v), r
    exc_ms, exc = timed(lambda: f.ExcerptLines(data, REACH, REACH))
    host_ms, host = timed(host_route)
    sel_ms, sel = timed(lambda: f.SelectLines(data))
    same = [[(s, t) for s, t, _ in per] for per in exc[1]] == [[(s, t) for s, t, _ in per] for per in host[1]]
    end_to_end = {"lines": data.count(b"\n"), "bytes": len(data), "lines_hit": int(len(exc[0])), "ExcerptLines_ms": round(exc_ms, 2),
                  "SpansLines_plus_host_slicing_ms": round(host_ms, 2), "SelectLines_ms": round(sel_ms, 2),
                  "excerpt_bytes": sum(len(t) for per in exc[1] for _, t, _ in per), "selected_bytes": len(sel[0]),
                  "same_excerpts_as_host_slicing": bool(same)}
    out = {"tool": "bench_excerpts", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "lines": args.lines, "terms": args.terms, "exprs": args.exprs, "window_s": args.window, "before": REACH,
                      "after": REACH},
           "shapes": shapes, "end_to_end": end_to_end}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
