#!/usr/bin/env python
"""What the lines round the hits cost: gft_context_docs_device (gft_context.hip) against gft_select_docs_device of the same batch
given as `also` the keep flags the context call decided -- it copies the same bytes, so the difference is the reach, carry and
decide passes (and the third prefix sum) alone --, and the finder call against the host route.

  (a) the calls, two shapes: the headline corpus of bench.py (--docs documents of about 4 KB), and the same text cut into lines of
      about 100 bytes.  Synthetic rows of one column, 1 % and 10 % of the documents hit; before = after = 2.  The two calls alternate
      in the same run (host clock round calls that end in a stream synchronise, the fill call into tensors of the counted sizes;
      medians over the repeats that fill a window of --window seconds), with the stages' own times from gft_profile_read per call.
      --baseline-lib PATH: the select is timed in a library built from another commit (the parent's), loaded beside the tree's,
      on a handle of its own.
  (b) the whole finder call over --lines lines from host memory: Finder.ContextLines against Finder.ProcessLines, a dilation of the
      hit flags in numpy and slicing on the host -- the route a caller had before.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_context.py [--docs 200000] [--lines 20000] [--baseline-lib PATH] [--out profiles/context_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CTX_STAGES = ("context_mark", "context_reach", "context_carry", "context_decide", "context_scan", "context_place", "context_copy")
SEL_STAGES = ("select_mark", "select_scan", "select_place", "select_copy")
BEFORE = AFTER = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per shape")
    ap.add_argument("--baseline-lib", default=None, help="a libgft.so of another commit for the select's times")
    ap.add_argument("--out", default=os.path.join("profiles", "context_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_context.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    eng = Engine()
    eh = eng._h
    # the select's library and handle: the tree's own, or another commit's
    BL, bh = L, eh
    if args.baseline_lib:
        BL = C.CDLL(os.path.abspath(args.baseline_lib))
        for name in ("gft_engine_create", "gft_engine_destroy", "gft_select_docs_device", "gft_profile_enable", "gft_profile_reset", "gft_profile_read"):
            fn = getattr(BL, name)
            fn.restype, fn.argtypes = _lib.SYMBOLS[name]
        bh = C.c_void_p()
        assert BL.gft_engine_create(C.byref(bh), 0) == 0

    def read_total(lib, h, cat):
        ms, cnt = C.c_double(), C.c_uint64()
        assert lib.gft_profile_read(h, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
        return ms.value

    def measure(text, off, fraction, seed):
        n = int(off.numel()) - 1
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        rows = (torch.rand(n, generator=g, device="cuda") < fraction).to(torch.int32).reshape(n, 1).contiguous()
        out, out_off, doc_idx, kind, group_off = eng.context_docs_device(text, off, rows, 1, None, "any", None, BEFORE, AFTER)
        m, nb, ng = int(doc_idx.numel()), int(out.numel()), int(group_off.numel()) - 1
        keep = torch.zeros(n, dtype=torch.uint8, device="cuda")
        keep[doc_idx] = 1
        sel = torch.empty(nb + 64, dtype=torch.uint8, device="cuda")
        sel_off = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        sel_idx = torch.empty(max(m, 1), dtype=torch.int64, device="cuda")
        cnt = [C.c_uint64(0) for _ in range(4)]
        refs = [C.byref(x) for x in cnt]

        def context():
            assert L.gft_context_docs_device(eh, text.data_ptr(), off.data_ptr(), n, rows.data_ptr(), 1, None, 0, None, BEFORE, AFTER, None, out.data_ptr(),
                                             nb, out_off.data_ptr(), doc_idx.data_ptr(), kind.data_ptr(), m, group_off.data_ptr(), ng, *refs) == 0

        def select():
            assert BL.gft_select_docs_device(bh, text.data_ptr(), off.data_ptr(), n, rows.data_ptr(), 1, None, 0, keep.data_ptr(), sel.data_ptr(), nb,
                                             sel_off.data_ptr(), sel_idx.data_ptr(), m, refs[0], refs[3]) == 0
        calls = (("context", context), ("select", select))
        for _ in range(2):                                          # warm-up: buffers grown, clocks up
            for _, fn in calls:
                fn()
        assert (cnt[0].value, cnt[3].value) == (m, nb) and torch.equal(sel[:nb], out) and torch.equal(sel_off, out_off), "the two calls copy other bytes"
        for lib, h in ((L, eh), (BL, bh)):
            assert lib.gft_profile_enable(h, 1) == 0 and lib.gft_profile_reset(h) == 0
        times = {name: [] for name, _ in calls}
        t0 = time.perf_counter()
        while len(times["context"]) < 5 or time.perf_counter() - t0 < args.window:
            for name, fn in calls:
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - a) * 1e3)
        reps = len(times["context"])
        res = {"documents": n, "hit": int(kind.sum().item()), "kept": m, "groups": ng, "bytes_copied": nb, "repeats": reps}
        for name, v in times.items():
            res[name + "_call_ms"] = round(statistics.median(v), 4)
        for cat in CTX_STAGES:
            res[cat + "_ms"] = round(read_total(L, eh, cat) / reps, 4)
        for cat in SEL_STAGES:
            res[cat + "_ms"] = round(read_total(BL, bh, cat) / reps, 4)
        L.gft_profile_enable(eh, 0)
        BL.gft_profile_enable(bh, 0)
        res["context_over_select"] = round(res["context_call_ms"] / res["select_call_ms"], 3)
        res["passes_ms"] = round(res["context_reach_ms"] + res["context_carry_ms"] + res["context_decide_ms"], 4)
        res["passes_over_copy"] = round(res["passes_ms"] / max(res["context_copy_ms"], 1e-9), 3)
        return res

    w = Workload(args.terms)
    shapes = {}
    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    loff = eng.split_lines_device(lined, n_bytes, 0)
    for pct in (1, 10):
        shapes["a1: documents of 4 KB, %d %% hit" % pct] = measure(text, off, pct / 100.0, pct)
        shapes["a2: lines of 100 bytes, %d %% hit" % pct] = measure(lined, loff, pct / 100.0, 100 + pct)
    del text, off, lined, loff
    torch.cuda.empty_cache()
    if args.baseline_lib:
        BL.gft_engine_destroy(bh)
    eng.close()

    # (b): the numbers a user sees
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(exprs)
    E = f.n_expressions
    t, o = w.docs_host(0, max(args.lines // 40, 1))
    a = np.array(t[:int(o[-1])], dtype=np.uint8)
    a[a == 10] = 32
    a[99::100] = 10
    data = a[:args.lines * 100].tobytes()
    off_h, rows_h = f.ProcessLines(data)
    hits = np.array([(rows_h[:, i >> 5] >> np.uint32(i & 31) & 1).mean() for i in range(E)])
    picked, hit = [], np.zeros(rows_h.shape[0], dtype=bool)
    for i in np.argsort(hits):                                      # rare expressions first, until about a twentieth of the lines hit
        if hits[i] == 0:
            continue
        picked.append(int(i))
        hit |= (rows_h[:, i >> 5] >> np.uint32(i & 31) & 1).astype(bool)
        if hit.mean() >= 0.05:
            break
    want = f.want_mask(indices=picked)

    def host_route():
        o, r = f.ProcessLines(data)
        h = (r & want).any(axis=1)
        keep = h.copy()
        for k in range(1, AFTER + 1):
            keep[k:] |= h[:-k]
        for k in range(1, BEFORE + 1):
            keep[:-k] |= h[k:]
        idx = np.flatnonzero(keep)
        b = np.frombuffer(data, dtype=np.uint8)
        return b"".join(b[int(o[d]):int(o[d + 1])].tobytes() for d in idx), idx

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
    ctx_ms, got = timed(lambda: f.ContextLines(data, BEFORE, AFTER, want, "any"))
    host_ms, ref = timed(host_route)
    end_to_end = {"lines": data.count(b"\n"), "bytes": len(data), "lines_hit": int(hit.sum()), "lines_kept": int(got[2].size), "groups": int(got[4].size) - 1,
                  "ContextLines_ms": round(ctx_ms, 2), "ProcessLines_numpy_dilation_host_slicing_ms": round(host_ms, 2),
                  "host_over_device": round(host_ms / ctx_ms, 2), "same_bytes_as_host_route": bool(got[0] == ref[0] and got[2].tolist() == ref[1].tolist())}
    f.close()
    out = {"tool": "bench_context", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "lines": args.lines, "terms": args.terms, "exprs": args.exprs, "window_s": args.window, "before": BEFORE,
                      "after": AFTER, "select_from": "another build: " + os.path.basename(args.baseline_lib) if args.baseline_lib else "the tree's library"},
           "shapes": shapes, "end_to_end": end_to_end}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
