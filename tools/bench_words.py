#!/usr/bin/env python
"""What whole-word matching costs: gft_filter_word_matches_device (gft_words.hip) over the scan's canonical match list against the
scan that makes the list, and the finder's ProcessDevice with the option on against the option off, on the two shapes of
tools/bench_term_stats.py:

  (a) bench.py's headline batch (--docs documents of about 4 KB);
  (b) the same text cut into lines of about 100 bytes;
and HighlightLines over --lines lines both ways.  Each pair alternates in the same run; host clock round calls that end in a stream
synchronise, medians, minimum and maximum over the repeats that fill --window seconds; the filter's stages from gft_profile_read.
The rows of the two finders are counted, not compared: the workload's expressions hold NOT, so a row may gain and lose bits.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_words.py [--docs 200000] [--lines 20000] [--out profiles/words_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per pair")
    ap.add_argument("--out", default=os.path.join("profiles", "words_bench.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_words.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import words_shape
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    finders = {}
    for name, whole in (("substrings", False), ("whole_words", True)):
        f = Finder(GpuEngine(), EmptyRgxEngine(), False, whole_words=whole)
        f.AddExpressions(exprs)
        finders[name] = f
    W = (finders["substrings"].n_expressions + 31) // 32

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "repeats": len(v)}

    def alternate(calls):
        """calls: [(name, fn)], each ending in a stream synchronise -> {name: summary}"""
        for _ in range(2):
            for _, fn in calls:
                fn()
        times = {k: [] for k, _ in calls}
        t0 = time.perf_counter()
        while len(times[calls[0][0]]) < 5 or time.perf_counter() - t0 < args.window * len(calls):
            for k, fn in calls:
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - a) * 1e3)
        return {k: summary(v) for k, v in times.items()}

    def batch(text, off):
        n = int(off.numel()) - 1
        res = {"documents": n, "bytes": int(off[-1].item())}
        rows = {k: torch.zeros((n, W), dtype=torch.int32, device="cuda") for k in finders}
        torch.cuda.synchronize()
        for k, f in finders.items():                                 # (builds the dictionary with the first batch)
            f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, rows[k].data_ptr())
        a, b = rows["substrings"], rows["whole_words"]
        res["rows_true_substrings"] = int((a != 0).any(dim=1).sum().item())
        res["rows_true_whole_words"] = int((b != 0).any(dim=1).sum().item())
        # the filter alone over the canonical list, against the scan that makes it
        f = finders["substrings"]
        eh = f.engine_handle()
        nt = int(L.gft_n_terms(eh))
        tp, ln = C.c_void_p(), C.c_uint32()
        lens = []
        for t in range(nt):
            assert L.gft_term(eh, t, C.byref(tp), C.byref(ln)) == 0
            lens.append(int(ln.value))
        tl = torch.tensor(lens, dtype=torch.int32, device="cuda")
        m = _lib.GftMatches()

        def scan():
            assert L.gft_scan_device(eh, text.data_ptr(), off.data_ptr(), n, _lib.GFT_FOLD_ASCII, C.byref(m)) == 0
        scan()
        nm = int(m.n_matches)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        out_pos, out_term = (torch.zeros(max(nm, 1), dtype=torch.int32, device="cuda") for _ in range(2))
        total = C.c_uint64(0)
        torch.cuda.synchronize()

        def scan_and_filter():
            scan()                                                   # (the list lives in the engine's buffers: every filter call follows its scan)
            assert L.gft_filter_word_matches_device(eh, text.data_ptr(), off.data_ptr(), n, m.match_off, m.pos, None, m.term_id, tl.data_ptr(), nt, 0,
                                                    out_off.data_ptr(), out_pos.data_ptr(), None, out_term.data_ptr(), nm, C.byref(total)) == 0
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        t = alternate([("scan_device", scan), ("scan_then_filter", scan_and_filter)])
        res.update(t)
        for cat in ("word_check", "word_mark", "word_scan", "word_place"):
            ms, cnt = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
            res[cat + "_ms"] = round(ms.value / max(int(cnt.value), 1), 4)
        L.gft_profile_enable(eh, 0)
        res["matches"], res["kept"] = nm, int(total.value)
        res["filter_ms"] = round(t["scan_then_filter"]["median_ms"] - t["scan_device"]["median_ms"], 4)
        res["filter_over_scan"] = round(res["filter_ms"] / t["scan_device"]["median_ms"], 4)
        res["filter_kernels_ms"] = round(sum(res[c + "_ms"] for c in ("word_check", "word_mark", "word_scan", "word_place")), 4)
        res["ns_per_match"] = round(res["filter_ms"] * 1e6 / max(nm, 1), 4)
        # the finder's ProcessDevice both ways
        t = alternate([(k, (lambda f=f, k=k: f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, rows[k].data_ptr()))) for k, f in finders.items()])
        res["process_device"] = t
        res["whole_words_over_substrings"] = round(t["whole_words"]["median_ms"] / t["substrings"]["median_ms"], 3)
        return res

    out = {"tool": "bench_words", "device": torch.cuda.get_device_name(0), "shape": words_shape(),
           "config": {"docs": args.docs, "terms": args.terms, "exprs": args.exprs, "lines": args.lines, "window_s": args.window}, "batches": {}}
    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    out["batches"]["a: documents of 4 KB"] = batch(text, off)
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    del text, off
    torch.cuda.empty_cache()
    loff = finders["substrings"].SplitLinesDevice(lined, n_bytes, 0)
    out["batches"]["b: lines of 100 bytes"] = batch(lined, loff)
    # HighlightLines over the first lines, both ways (upload, split, process, spans, marks, download)
    end = int(loff[min(args.lines, int(loff.numel()) - 1)].item())
    data = lined[:end].cpu().numpy().tobytes()
    marked = {}

    def highlight(k):
        marked[k] = finders[k].HighlightLines(data)[0]
    t = alternate([(k, (lambda k=k: highlight(k))) for k in finders])
    out["highlight_lines"] = {"lines": min(args.lines, int(loff.numel()) - 1), "bytes": end, **t,
                              "marked_bytes": {k: len(v) for k, v in marked.items()},
                              "whole_words_over_substrings": round(t["whole_words"]["median_ms"] / t["substrings"]["median_ms"], 3)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
