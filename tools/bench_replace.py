#!/usr/bin/env python
"""What replacing the hits costs: gft_replace_spans_device (the excerpt's run passes, gft_replace.hip) against calls that were
there before and move the same text -- gft_mark_spans_device (the yardstick: <em> plus </em> per run is the same kind of work as a
5-byte replacement per run), gft_select_docs_device of the documents that hit and a plain device copy of the batch's bytes --, and
the finder call against the host route.

  (a) the calls, two shapes: the headline corpus of bench.py (--docs documents of about 4 KB), and the same text cut into lines of
      about 100 bytes.  One 5-byte replacement for every run.  The replace call, the mark call, the select and the copy alternate
      in the same run (host clock round calls that end in a stream synchronise, the fill call into tensors of the counted sizes;
      medians over the rounds that fill a window of --window seconds), with the stages' own times from gft_profile_read read
      after every call: the median per round and the quartiles, which are the run-to-run spread the copy kernels are compared
      within.
  (b) three replacement shapes on the 4 KB corpus: every run deleted, 5 bytes, 255 bytes.
  (c) the whole finder call over --lines lines from host memory: Finder.ReplaceLines against Finder.SpansLines(source=True) plus
      a splice in Python -- the route a caller had before.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_replace.py [--docs 200000] [--lines 20000] [--out profiles/replace_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

REP_STAGES = ("replace_runs", "replace_ids", "replace_scan", "replace_place", "replace_copy")
MARK_STAGES = ("mark_runs", "mark_scan", "mark_place", "mark_copy")
SEL_STAGES = ("select_mark", "select_scan", "select_place", "select_copy")
OPEN, CLOSE = b"<em>", b"</em>"
FIVE = b"[NAM]"


def quartiles(v):
    s = sorted(v)
    return [round(s[len(s) // 4], 4), round(statistics.median(s), 4), round(s[(3 * len(s)) // 4], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per shape")
    ap.add_argument("--out", default=os.path.join("profiles", "replace_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_replace.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import replace_table
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

    def replacer(text, off, n, so, st, ln, rep):
        """(the fill call as a function, bytes written, runs)"""
        out, out_off, dro, run_new, run_len, run_rep, _ = f.ReplaceDevice(text, off, so, st, ln, None, False, False, rep)
        nb, runs = int(out.numel()), int(run_new.numel())
        rep_bytes, rep_off = replace_table(rep)
        cm, ct = C.c_uint64(0), C.c_uint64(0)

        def call():
            assert L.gft_replace_spans_device(eh, text.data_ptr(), off.data_ptr(), n, so.data_ptr(), st.data_ptr(), ln.data_ptr(), None, None, 0,
                                              rep_bytes or None, rep_off.ctypes.data, 1, 0, out.data_ptr(), nb, out_off.data_ptr(), dro.data_ptr(),
                                              run_new.data_ptr(), run_len.data_ptr(), run_rep.data_ptr(), runs, C.byref(cm), C.byref(ct)) == 0
        call.keep = (out, out_off, dro, run_new, run_len, run_rep, rep_bytes, rep_off)
        return call, nb, runs

    def alternate(calls, stages):
        """the calls in turn until the window is full -> ({name: [ms]}, {stage: [ms per round]})"""
        for _ in range(2):                                          # warm-up: buffers grown, clocks up
            for _, fn in calls:
                fn()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        times = {name: [] for name, _ in calls}
        per = {s: [] for s in stages}
        last = {s: 0.0 for s in stages}
        t0 = time.perf_counter()
        while len(times[calls[0][0]]) < 5 or time.perf_counter() - t0 < args.window:
            for name, fn in calls:
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - a) * 1e3)
            for s in stages:
                v = read_total(s)
                per[s].append(v - last[s])
                last[s] = v
        L.gft_profile_enable(eh, 0)
        return times, per

    def spans_of(text, off):
        n = int(off.numel()) - 1
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())
        so, st, ln, tm, lowered = f.SpansDevice(text, off, bm)
        assert not lowered
        return n, bm, so, st, ln

    def measure(text, off):
        n, bm, so, st, ln = spans_of(text, off)
        rep, rb, runs = replacer(text, off, n, so, st, ln, FIVE)
        out, out_off, span_new, doc_run_off, _ = f.MarkDevice(text, off, so, st, ln, False, False, OPEN, CLOSE)
        nb = int(out.numel())
        sel, sel_off, sel_idx = f.SelectDevice(text, off, bm)
        sm, sb = int(sel_idx.numel()), int(sel.numel())
        n_text = int(off[-1].item() - off[0].item())
        plain = torch.empty(n_text, dtype=torch.uint8, device="cuda")
        src = text[int(off[0].item()):int(off[0].item()) + n_text]
        cm, ct = C.c_uint64(0), C.c_uint64(0)

        def mark():
            assert L.gft_mark_spans_device(eh, text.data_ptr(), off.data_ptr(), n, so.data_ptr(), st.data_ptr(), ln.data_ptr(), OPEN, len(OPEN), CLOSE,
                                           len(CLOSE), 0, out.data_ptr(), nb, out_off.data_ptr(), span_new.data_ptr(), doc_run_off.data_ptr(),
                                           C.byref(cm), C.byref(ct)) == 0

        def select():
            assert L.gft_select_docs_device(eh, text.data_ptr(), off.data_ptr(), n, bm.data_ptr(), f.n_expressions, None, 0, None, sel.data_ptr(), sb,
                                            sel_off.data_ptr(), sel_idx.data_ptr(), sm, C.byref(cm), C.byref(ct)) == 0

        def copy():
            plain.copy_(src)
            torch.cuda.synchronize()
        times, per = alternate((("replace", rep), ("mark", mark), ("select", select), ("copy", copy)), REP_STAGES + MARK_STAGES + SEL_STAGES)
        res = {"documents": n, "text_bytes": n_text, "documents_hit": sm, "selected_bytes": sb, "spans": int(st.numel()), "runs": runs,
               "replaced_bytes": rb, "marked_bytes": nb, "rounds": len(times["replace"])}
        for name, v in times.items():
            res[name + "_call_ms"] = round(statistics.median(v), 4)
        for cat, v in per.items():
            res[cat + "_ms"] = round(statistics.median(v), 4)
        res["replace_over_mark"] = round(res["replace_call_ms"] / res["mark_call_ms"], 3)
        res["replace_over_select"] = round(res["replace_call_ms"] / res["select_call_ms"], 3)
        res["replace_over_copy"] = round(res["replace_call_ms"] / res["copy_call_ms"], 3)
        # the three copy kernels per byte they write: quartiles over the rounds
        for cat, b in (("replace_copy", rb), ("mark_copy", nb), ("select_copy", sb)):
            res[cat + "_ns_per_KB_q1_median_q3"] = quartiles([x * 1e6 / max(b, 1) * 1024 for x in per[cat]])
        return res

    def shapes_of(text, off):
        n, bm, so, st, ln = spans_of(text, off)
        calls, meta = [], {}
        for name, rep in (("deleted", b""), ("5_bytes", FIVE), ("255_bytes", bytes(33 + i % 90 for i in range(255)))):
            fn, nb, runs = replacer(text, off, n, so, st, ln, rep)
            calls.append((name, fn))
            meta[name] = {"replaced_bytes": nb, "runs": runs}
        res = {}
        # (one call a round per shape: the stages' totals are read after each)
        for name, fn in calls:
            times, per = alternate(((name, fn),), REP_STAGES)
            res[name] = dict(meta[name], call_ms=round(statistics.median(times[name]), 4), rounds=len(times[name]),
                             **{s + "_ms": round(statistics.median(v), 4) for s, v in per.items()})
            res[name]["replace_copy_ns_per_KB_q1_median_q3"] = quartiles([x * 1e6 / max(meta[name]["replaced_bytes"], 1) * 1024
                                                                        for x in per["replace_copy"]])
        return res

    shapes = {}
    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    shapes["a1: documents of 4 KB"] = measure(text, off)
    rep_shapes = shapes_of(text, off)
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    shapes["a2: lines of 100 bytes"] = measure(lined, loff)
    del text, off, lined, loff
    torch.cuda.empty_cache()

    # (c): the numbers a user sees
    t, o = w.docs_host(0, max(args.lines // 40, 1))
    a = np.array(t[:int(o[-1])], dtype=np.uint8)
    a[a == 10] = 32
    a[99::100] = 10
    data = a[:args.lines * 100].tobytes()

    def host_route():
        idx, spans, _ = f.SpansLines(data, source=True)
        lines = data.split(b"\n")
        hit = dict(zip(idx.tolist(), spans))
        res = []
        for d, line in enumerate(lines[:-1] if data.endswith(b"\n") else lines):
            line += b"\n"
            sp = hit.get(d)
            if not sp:
                res.append(line)
                continue
            runs = []
            for s, e, _ in sorted((s, e, 0) for s, e, _ in sp):
                if runs and s <= runs[-1][1]:
                    runs[-1][1] = max(runs[-1][1], e)
                else:
                    runs.append([s, e])
            parts, pos = [], 0
            for s, e in runs:
                parts += [line[pos:s], FIVE]
                pos = e
            parts.append(line[pos:])
            res.append(b"".join(parts))
        return b"".join(res)

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
    rl_ms, rl = timed(lambda: f.ReplaceLines(data, FIVE))
    host_ms, host = timed(host_route)
    end_to_end = {"lines": data.count(b"\n"), "bytes": len(data), "replaced_bytes": len(rl[0]), "ReplaceLines_ms": round(rl_ms, 2),
                  "SpansLines_plus_host_splice_ms": round(host_ms, 2), "host_over_device": round(host_ms / rl_ms, 2),
                  "same_bytes_as_host_splice": bool(rl[0] == host)}
    out = {"tool": "bench_replace", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "lines": args.lines, "terms": args.terms, "exprs": args.exprs, "window_s": args.window,
                      "replacement": FIVE.decode(), "open": OPEN.decode(), "close": CLOSE.decode()},
           "shapes": shapes, "replacement_shapes_4KB": rep_shapes, "end_to_end": end_to_end}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
