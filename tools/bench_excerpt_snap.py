#!/usr/bin/env python
"""What snapping the excerpts' windows to word or line borders costs: gft_excerpt_spans_snap_device against
gft_excerpt_spans_device -- which this feature leaves as it was -- on the same resident batch and the same spans, corpus and rule
set of tools/bench_excerpts.py, before = after = 40.

  shapes   the headline corpus of bench.py (--docs documents of about 4 KB), and the same text cut into lines of about 100 bytes
  runs     per shape: the snapped entry point with NO snap bit (a condition, not a measurement: it launches the same kernels, so
           its time must lie within the plain call's spread), snap = words at reach 64, and -- on the 4 KB documents -- snap =
           lines at reach 4096
Each run alternates with the plain call in the same loop (host clock round calls that end in a stream synchronise, the fill call
into tensors of the counted sizes; median and [min, max] over the repeats that fill a window of --window seconds), with the
"excerpt_window" stage time of each side from gft_profile_read round every call.  No threshold in here; prints one JSON line and
writes it to --out.

    python tools/bench_excerpt_snap.py [--docs 200000] [--out profiles/excerpt_snap_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

REACH = 40
RUNES, WORDS, LINES = 1, 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per run")
    ap.add_argument("--out", default=os.path.join("profiles", "excerpt_snap_bench.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_excerpt_snap.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import excerpt_spans_tensor
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(exprs)
    eh = f.engine_handle()
    W = (f.n_expressions + 31) // 32

    def window_ms():
        ms, cnt = C.c_double(), C.c_uint64()
        assert L.gft_profile_read(eh, b"excerpt_window", C.byref(ms), C.byref(cnt)) == 0
        return ms.value

    def ok(rc):
        assert rc == 0, L.gft_last_error(eh)

    def spread(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def measure(text, off, runs):
        n = int(off.numel()) - 1
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())
        so, st, ln, tm, lowered = f.SpansDevice(text, off, bm)
        assert not lowered
        cm, ct = C.c_uint64(0), C.c_uint64(0)
        head = (eh, text.data_ptr(), off.data_ptr(), n, so.data_ptr(), st.data_ptr(), ln.data_ptr(), REACH, REACH)

        def prepared(flags, reach):
            """the outputs of one side, sized by a counting call, and the fill call into them"""
            snap = {0: None, WORDS: "words", LINES: "lines"}[flags & 6]
            if snap is None:                                        # (no snap bit: the plain call's sizes, which the fill call confirms)
                ex = excerpt_spans_tensor(lambda *a: ok(L.gft_excerpt_spans_device(eh, *a)), text, off, so, st, ln, REACH, REACH, True)
            else:
                ex = excerpt_spans_tensor(lambda *a: ok(L.gft_excerpt_spans_snap_device(eh, *a)), text, off, so, st, ln, REACH, REACH, True, snap, reach)
            out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off = ex
            m, nb = int(exc_doc.numel()), int(out.numel())
            tail = (out.data_ptr(), nb, exc_off.data_ptr(), exc_doc.data_ptr(), exc_start.data_ptr(), exc_span_off.data_ptr(), m, span_rel.data_ptr(),
                    doc_exc_off.data_ptr(), C.byref(cm), C.byref(ct))

            def call():
                if reach is None:
                    assert L.gft_excerpt_spans_device(*head, flags, *tail) == 0
                else:
                    assert L.gft_excerpt_spans_snap_device(*head, flags, reach, *tail) == 0
                assert cm.value == m and ct.value == nb
            return call, m, nb, ex

        plain, m0, nb0, keep0 = prepared(RUNES, None)
        res = {"documents": n, "text_bytes": int(off[-1].item() - off[0].item()), "spans": int(st.numel()), "excerpts": m0, "excerpt_bytes": nb0,
               "runs": {}}
        for name, flags, reach in runs:
            snapped, m, nb, keep = prepared(flags, reach)
            for _ in range(2):                                      # warm-up: buffers grown, clocks up
                plain()
                snapped()
            assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
            times = {"plain": [], "snapped": []}
            stage = {"plain": [], "snapped": []}
            t0 = time.perf_counter()
            while len(times["plain"]) < 5 or time.perf_counter() - t0 < args.window:
                for side, fn in (("plain", plain), ("snapped", snapped)):
                    torch.cuda.synchronize()
                    s0 = window_ms()
                    a = time.perf_counter()
                    fn()
                    times[side].append((time.perf_counter() - a) * 1e3)
                    stage[side].append(window_ms() - s0)
            L.gft_profile_enable(eh, 0)
            r = {"flags": flags, "reach": reach, "excerpts": m, "excerpt_bytes": nb, "repeats": len(times["plain"]),
                 "plain_call_ms": spread(times["plain"]), "snapped_call_ms": spread(times["snapped"]),
                 "plain_excerpt_window_ms": spread(stage["plain"]), "snapped_excerpt_window_ms": spread(stage["snapped"])}
            r["snapped_over_plain"] = round(r["snapped_call_ms"]["median"] / r["plain_call_ms"]["median"], 3)
            r["within_plain_spread"] = bool(r["plain_call_ms"]["min"] <= r["snapped_call_ms"]["median"] <= r["plain_call_ms"]["max"])
            if not flags & 6:                                       # the condition: the same excerpts, byte for byte
                r["same_bytes_as_plain"] = bool(m == m0 and nb == nb0 and torch.equal(keep[0], keep0[0]))
            res["runs"][name] = r
            del snapped, keep
        return res

    shapes = {}
    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    shapes["a1: documents of 4 KB"] = measure(text, off, (("no snap bit", RUNES, 64), ("words, reach 64", RUNES | WORDS, 64),
                                                         ("lines, reach 4096", RUNES | LINES, 4096)))
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    shapes["a2: lines of 100 bytes"] = measure(lined, loff, (("no snap bit", RUNES, 64), ("words, reach 64", RUNES | WORDS, 64)))
    out = {"tool": "bench_excerpt_snap", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "terms": args.terms, "exprs": args.exprs, "window_s": args.window, "before": REACH, "after": REACH},
           "shapes": shapes}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
