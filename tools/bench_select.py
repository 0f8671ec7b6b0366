#!/usr/bin/env python
"""What keeping the documents that hit costs: gft_select_docs_device (gft_select.hip) per launch, and its copy kernel against a plain
device-to-device copy of the same number of bytes (torch.Tensor.copy_ between two resident tensors), alternating in the same run.

  (a) the headline corpus of bench.py (--docs documents of about 4 KB, 10 000 terms, 1 000 expressions), rows from the real finder:
      ANY over 1 expression, over 10 (those whose own hit rates lie nearest to 5 %: a middle selectivity) and over all, and
      want = NULL under NONE;
  (b) the same corpus with synthetic rows: 1 %, 10 %, 50 % and 100 % of the documents selected;
  (c) the JSON Lines corpus of tools/bench_split_lines.py (--json-docs documents), cut with GFT_SPLIT_JSON_LINES, synthetic rows at
      10 % and 100 %.

Per shape: the four launches' times from gft_profile_read (means over the repeats that fill a window of --window seconds), GB/s of
select_copy as 2 x bytes copied / time, the same for the plain copy, and their ratio.  The whole series runs --runs times: the
spread of the copy's own figure from run to run is what a ratio has to be read against.  Then the number a user sees: Finder.SelectLines
over --lines text lines from host memory against "ProcessLines, download offsets and rows, gather in numpy" at about 10 %
selectivity.  No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_select.py [--docs 1000000] [--json-docs 200000] [--lines 200000] [--runs 3] [--out profiles/select_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LAUNCHES = ("select_mark", "select_scan", "select_place", "select_copy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--json-docs", type=int, default=200_000)
    ap.add_argument("--lines", type=int, default=200_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of select calls per shape (well over a tenth)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "select_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_select.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    for i, e in enumerate(exprs):
        f.AddExpressionWithTag(e, "tag%d" % (i % 50))
    eh = f.engine_handle()
    E = f.n_expressions
    W = (E + 31) // 32

    def measure(text, off, rows, n_cols, want, mode):
        """one shape -> its figures: the fill call with exact caps, alternating with a copy_ of the same bytes"""
        n = int(off.numel()) - 1
        m, total = C.c_uint64(0), C.c_uint64(0)
        wp = want.ctypes.data if want is not None else None
        head = (eh, text.data_ptr(), off.data_ptr(), n, rows.data_ptr() if n_cols else None, n_cols, wp, mode, None)
        torch.cuda.synchronize()
        assert L.gft_select_docs_device(*head, None, 0, None, None, 0, C.byref(m), C.byref(total)) == 0
        nm, nb = int(m.value), int(total.value)
        out = torch.empty(nb + 64, dtype=torch.uint8, device="cuda")
        src = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda").random_(0, 256)
        dst = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
        oo = torch.empty(nm + 1, dtype=torch.int64, device="cuda")
        di = torch.empty(max(nm, 1), dtype=torch.int64, device="cuda")

        def call():
            assert L.gft_select_docs_device(*head, out.data_ptr(), nb, oo.data_ptr(), di.data_ptr(), nm, C.byref(m), C.byref(total)) == 0
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(2):                                   # warm-up: buffers grown, clocks up
            call()
            dst.copy_(src)
        torch.cuda.synchronize()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        copy_ms, reps, t0 = 0.0, 0, time.perf_counter()
        while reps < 5 or time.perf_counter() - t0 < args.window:
            call()
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            copy_ms += ev[0].elapsed_time(ev[1])
            reps += 1
        res = {"documents": n, "selected": nm, "bytes_copied": nb, "repeats": reps}
        for cat in LAUNCHES:
            ms, cnt = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
            res[cat + "_ms"] = round(ms.value / max(cnt.value, 1), 4)
        L.gft_profile_enable(eh, 0)
        copy_ms /= reps
        res["plain_copy_ms"] = round(copy_ms, 4)
        if nb and res["select_copy_ms"] > 0:
            res["select_copy_GBps"] = round(2 * nb / (res["select_copy_ms"] * 1e-3) / 1e9, 1)
            res["plain_copy_GBps"] = round(2 * nb / (copy_ms * 1e-3) / 1e9, 1)
            res["ratio_to_plain_copy"] = round(copy_ms / res["select_copy_ms"], 3)
        del out, src, dst
        return res

    def synthetic(n, fraction, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return (torch.rand(n, generator=g, device="cuda") < fraction).to(torch.int32).reshape(n, 1).contiguous()

    runs = []
    # (a), (b): the headline corpus
    text, off = w.docs_device(0, args.docs)
    bm = torch.zeros((args.docs, W), dtype=torch.int32, device="cuda")
    f.ProcessDevice(text.data_ptr(), off.data_ptr(), args.docs, bm.data_ptr())
    # (c): JSON Lines
    def lines_of(n):
        t, o = w.docs_host(0, n)
        return [bytes(t[int(o[d]):int(o[d + 1])]).replace(b"\n", b" ") for d in range(n)]
    raws = []
    for d, t in enumerate(lines_of(args.json_docs)):
        t = t.decode("ascii")
        k = len(t) // 8
        p = [t[i * k:(i + 1) * k] for i in range(8)]
        raws.append(json.dumps({"Id": d, "Title": p[0], "Body": [p[1], p[2], p[3]], "Meta": {"Author": p[4], "Notes": [p[5]]},
                                "Comments": [{"Text": p[6], "Score": 3}, {"Text": p[7], "Score": 5}]}).encode())
    jblob = b"\n".join(raws) + b"\n"
    jtext = torch.from_numpy(np.frombuffer(jblob + b"\0" * 64, dtype=np.uint8).copy()).cuda()
    joff = f.SplitLinesDevice(jtext, len(jblob), 1)
    del raws
    # ten expressions for a middle selectivity: the generator's expressions cover the corpus, so the first ten already hit every
    # document; these are the ten whose own hit rates lie nearest to 5 %
    counts = torch.stack([((bm[:, i >> 5] >> (i & 31)) & 1).sum() for i in range(E)]).cpu().numpy() / float(args.docs)
    middle = [int(i) for i in np.argsort(np.abs(counts - 0.05))[:10]]
    for run in range(args.runs):
        shapes = {}
        for name, want, mode in (("a: ANY over 1 expression", f.want_mask(indices=[0]), 0), ("a: ANY over 10 expressions", f.want_mask(indices=middle), 0),
                                 ("a: ANY over all expressions", f.want_mask(), 0), ("a: NONE, want NULL", None, 2)):
            shapes[name] = measure(text, off, bm, E, want, mode)
        for pct in (1, 10, 50, 100):
            shapes["b: %d %% selected" % pct] = measure(text, off, synthetic(args.docs, pct / 100.0, pct), 1, None, 0)
        for pct in (10, 100):
            shapes["c: JSON lines, %d %% selected" % pct] = measure(jtext, joff, synthetic(int(joff.numel()) - 1, pct / 100.0, pct), 1, None, 0)
        runs.append(shapes)
    full = [r["b: 100 % selected"] for r in runs]
    spread = {"plain_copy_GBps": [r.get("plain_copy_GBps") for r in full], "select_copy_GBps": [r.get("select_copy_GBps") for r in full],
              "ratio_to_plain_copy": [r.get("ratio_to_plain_copy") for r in full]}
    del text, off, bm, jtext, joff
    torch.cuda.empty_cache()

    # the number a user sees: lines in host memory, the selected lines back in host memory
    data = b"\n".join(lines_of(args.lines)) + b"\n"
    off_h, rows_h = f.ProcessLines(data)
    hits = np.array([(rows_h[:, i >> 5] >> np.uint32(i & 31) & 1).mean() for i in range(E)])
    order = np.argsort(-hits)
    picked, frac, hit = [], 0.0, np.zeros(rows_h.shape[0], dtype=bool)
    for i in order[::-1]:                                    # rare expressions first, until about a tenth of the lines hit
        if hits[i] == 0:
            continue
        picked.append(int(i))
        hit |= (rows_h[:, i >> 5] >> np.uint32(i & 31) & 1).astype(bool)
        frac = float(hit.mean())
        if frac >= 0.1:
            break
    want = f.want_mask(indices=picked)

    def numpy_route():
        o, r = f.ProcessLines(data)
        keep = np.flatnonzero((r & want).any(axis=1))
        a = np.frombuffer(data, dtype=np.uint8)
        return b"".join(a[int(o[d]):int(o[d + 1])].tobytes() for d in keep), keep

    def timed(fn, reps=3):
        best = None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None or dt < best else best
        return best, r
    sel_ms, got = timed(lambda: f.SelectLines(data, want, "any"))
    np_ms, ref = timed(numpy_route)
    assert got[0] == ref[0] and got[2].tolist() == ref[1].tolist(), "SelectLines and the numpy gather differ"
    end_to_end = {"lines": args.lines, "bytes": len(data), "selectivity": round(frac, 4), "expressions_in_mask": len(picked),
                  "SelectLines_ms": round(sel_ms, 2), "ProcessLines_download_numpy_gather_ms": round(np_ms, 2)}
    out = {"tool": "bench_select", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "json_docs": args.json_docs, "lines": args.lines, "terms": args.terms, "exprs": args.exprs,
                      "window_s": args.window, "runs": args.runs},
           "runs": runs, "spread_at_100_percent": spread, "end_to_end": end_to_end}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
