#!/usr/bin/env python
"""What mapping the spans of a lowered batch back to the caller's bytes costs: gft_map_spans_to_source_device (gft_lowermap.hip and
the table form of k_lower) against gft_to_lower_device of the SAME batch -- existing code: the map replaces the lowered clone that
Finder.RedactLines needed before --, and Finder.RedactLines(source=True) against Finder.RedactLines() and against the host route.

  (a) the map call, two shapes, one non-ASCII upper-case letter (É) at the head of every document so that the finder lowers the batch:
      the headline corpus of bench.py (--docs documents of about 4 KB), and the same text cut into lines of about 100 bytes.
      Both calls alternate in the same run (host clock round calls that end in a stream synchronise; medians over the repeats that
      fill a window of --window seconds; the span arrays are restored outside the clock, the map works in place), with the
      stages' own times from gft_profile_read per call: "lowermap_table" (count pass, prefix sum, table pass), "lowermap_spans"
      (check and write pass), and "lower_count" / "lower_scan" / "lower_write" of the lower call.
  (b) the whole finder call: RedactLines(source=True) against RedactLines() over --lines lines from host memory, one É in them;
  (c) the host route of tools/bench_spans.py on that log, for scale: gft_scan from host memory, the join of the match list with the
      rows and the witness sets in Python, the masking of a bytearray (it folds ASCII only: its bytes are not compared).
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_lowermap.py [--docs 200000] [--lines 20000] [--out profiles/lowermap_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MAP_STAGES = ("lowermap_table", "lowermap_spans")
LOWER_STAGES = ("lower_count", "lower_scan", "lower_write")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per shape")
    ap.add_argument("--out", default=os.path.join("profiles", "lowermap_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_lowermap.py measures on the GPU: no HIP device here")
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

    def with_capital(text, off):
        """É over the first two bytes of every document that has them"""
        n_bytes = int(off[-1].item())
        out = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
        out[:n_bytes] = text[:n_bytes]
        at = off[:-1][(off[1:] - off[:-1]) >= 2]
        out[at] = 0xC3
        out[at + 1] = 0x89
        return out

    def measure(text, off):
        n = int(off.numel()) - 1
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())
        so, st, ln, _, lowered = f.SpansDevice(text, off, bm)
        assert lowered, "the batch was not lowered: no span to map"
        st0, ln0 = st.clone(), ln.clone()
        low_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        tot = C.c_uint64(0)
        torch.cuda.synchronize()
        assert L.gft_to_lower_device(eh, text.data_ptr(), off.data_ptr(), n, None, 0, low_off.data_ptr(), C.byref(tot)) == 0
        low = torch.empty(int(tot.value) + 64, dtype=torch.uint8, device="cuda")

        def lower():
            assert L.gft_to_lower_device(eh, text.data_ptr(), off.data_ptr(), n, low.data_ptr(), int(tot.value), low_off.data_ptr(), C.byref(tot)) == 0

        def spans_map():
            assert L.gft_map_spans_to_source_device(eh, text.data_ptr(), off.data_ptr(), n, so.data_ptr(), st.data_ptr(), ln.data_ptr()) == 0

        def restore():
            st.copy_(st0)
            ln.copy_(ln0)
            torch.cuda.synchronize()
        for _ in range(2):                                          # warm-up: buffers grown, clocks up
            lower()
            restore()
            spans_map()
        moved = int((st != st0).sum().item())
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        times = {"lower": [], "map": []}
        t0 = time.perf_counter()
        while len(times["map"]) < 5 or time.perf_counter() - t0 < args.window:
            restore()
            for name, fn in (("lower", lower), ("map", spans_map)):
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - a) * 1e3)
        reps = len(times["map"])
        res = {"documents": n, "text_bytes": int(off[-1].item() - off[0].item()), "lowered_bytes": int(tot.value), "spans": int(st.numel()),
               "spans_moved": moved, "repeats": reps}
        for name, v in times.items():
            res[name + "_call_ms"] = round(statistics.median(v), 4)
        for cat in MAP_STAGES + LOWER_STAGES:
            res[cat + "_ms"] = round(read_total(cat) / reps, 4)
        L.gft_profile_enable(eh, 0)
        res["map_over_lower"] = round(res["map_call_ms"] / res["lower_call_ms"], 3)
        res["map_stages_over_lower_stages"] = round(sum(res[c + "_ms"] for c in MAP_STAGES) / max(sum(res[c + "_ms"] for c in LOWER_STAGES), 1e-9), 3)
        return res

    shapes = {}
    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    shapes["a1: documents of 4 KB"] = measure(with_capital(text, off), off)
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    shapes["a2: lines of 100 bytes"] = measure(with_capital(lined, loff), loff)
    del text, off, lined, loff
    torch.cuda.empty_cache()

    # (b), (c): the numbers a user sees -- the log of bench_spans.py with one É in it
    t, o = w.docs_host(0, max(args.lines // 40, 1))
    a = np.array(t[:int(o[-1])], dtype=np.uint8)
    a[a == 10] = 32
    a[99::100] = 10
    a = a[:args.lines * 100]
    a[50:52] = (0xC3, 0x89)
    data = a.tobytes()

    def host_route():
        from gofindthem_amd.engine import split_lines_host
        n, doff = split_lines_host(data, 0)
        doff = doff[:n + 1]
        rows = f.ProcessTexts(blob=np.frombuffer(data + b"\0" * 64, dtype=np.uint8), doc_off=doff)
        moff, tid, pos = host_route.eng.scan(np.frombuffer(data.lower() + b"\0" * 64, dtype=np.uint8), doff)
        out = bytearray(data)
        wit, lens = host_route.wit, host_route.lens
        moff, tid, pos, doff = moff.tolist(), tid.tolist(), pos.tolist(), doff.tolist()
        for d in range(n):
            row = int.from_bytes(rows[d].tobytes(), "little")
            for k in range(moff[d], moff[d + 1]):
                if wit[tid[k]] & row:
                    s = doff[d] + pos[k]
                    out[s:s + lens[tid[k]]] = b"*" * lens[tid[k]]
        return bytes(out)
    from gofindthem_amd.engine import Engine
    host_route.eng = Engine()
    host_route.eng.build(sorted(k if isinstance(k, bytes) else k.encode() for k in f.GetKeywords()))
    terms = host_route.eng.terms()
    host_route.lens = [len(k) for k in terms]
    tid_of = {k: i for i, k in enumerate(terms)}
    wit = [0] * len(terms)
    for i in range(f.n_expressions):
        stack = [f.expression(i)[2]]
        while stack:
            nd = stack.pop()
            if nd["Type"] == "UNIT":
                lit = nd.get("Literal", "").encode()
                if lit in tid_of:
                    wit[tid_of[lit]] |= 1 << i
            elif nd["Type"] != "NOT":
                stack += [nd[k] for k in ("LExpr", "RExpr") if k in nd]
    host_route.wit = wit

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
    src_ms, src = timed(lambda: f.RedactLines(data, source=True))
    low_ms, low = timed(lambda: f.RedactLines(data))
    host_ms, _ = timed(host_route, reps=2)
    diff = np.frombuffer(src[0], np.uint8) != np.frombuffer(data, np.uint8)
    end_to_end = {"lines": data.count(b"\n"), "bytes": len(data), "RedactLines_source_ms": round(src_ms, 2), "RedactLines_ms": round(low_ms, 2),
                  "source_over_lowered": round(src_ms / low_ms, 3), "host_scan_python_join_bytearray_ms": round(host_ms, 2),
                  "lowered": bool(src[1] and low[1]), "same_length_as_input": len(src[0]) == len(data),
                  "bytes_changed_by_source": int(diff.sum()), "all_changed_are_masks": bool((np.frombuffer(src[0], np.uint8)[diff] == ord("*")).all()),
                  "bytes_changed_by_lowered": int((np.frombuffer(low[0], np.uint8) != np.frombuffer(data, np.uint8)).sum()) if len(low[0]) == len(data) else None}
    out = {"tool": "bench_lowermap", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "lines": args.lines, "terms": args.terms, "exprs": args.exprs, "window_s": args.window},
           "shapes": shapes, "end_to_end": end_to_end}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
