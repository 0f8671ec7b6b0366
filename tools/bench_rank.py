#!/usr/bin/env python
"""What the ranking costs: gft_score_docs_device, gft_top_docs_device (gft_rank.hip) and Finder.TopLines against their yardsticks.

  (a) the canonical match list of bench.py's headline batch (--docs documents of about 4 KB);
  (b) the same text cut into lines of about 100 bytes.
Each: the score call (plain and distinct) against gft_term_stats_device on the same list -- the same walk with another sink; with
--parent LIB that call comes from the parent commit's library --, the top call at k = 10 and k = 4096 against a plain device read of
the score array (its maximum), alternating in the same run; host clock round calls that end in a stream synchronise, medians,
minimum and maximum over the repeats that fill --window seconds; the stages' own times from gft_profile_read.
  (c) Finder.TopLines over --lines lines against the host route: SpansLines, then reduceat and argpartition in numpy.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_rank.py [--docs 200000] [--parent /path/to/parent/libgft.so] [--out profiles/rank_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STAGES = ("score_check", "score_docs", "top_max", "top_select", "top_place", "top_sort")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--lines", type=int, default=20_000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per measurement")
    ap.add_argument("--parent", default=None, help="the parent commit's libgft.so: its gft_term_stats_device is the score call's yardstick")
    ap.add_argument("--out", default=os.path.join("profiles", "rank_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rank.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import rank_shape
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    L = _lib.load()
    w = Workload(args.terms)
    exprs = make_expressions(w.terms(), args.exprs, inord_fraction=0.0, cover=True)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(exprs)
    eh = f.engine_handle()
    W = (f.n_expressions + 31) // 32
    PL, ph = L, eh
    if args.parent:
        PL, ph = C.CDLL(os.path.abspath(args.parent)), C.c_void_p()
        PL.gft_engine_create.argtypes, PL.gft_engine_create.restype = [C.c_void_p, C.c_int], C.c_int
        PL.gft_term_stats_device.argtypes = _lib.SYMBOLS["gft_term_stats_device"][1]
        PL.gft_engine_destroy.argtypes = [C.c_void_p]
        assert PL.gft_engine_create(C.byref(ph), -1) == 0

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "repeats": len(v)}

    def measure(calls):
        """{name: summary} of the calls, alternating, and the stages' times per round"""
        for _ in range(2):
            for _, fn in calls:
                fn()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        times = {k: [] for k, _ in calls}
        t0 = time.perf_counter()
        while len(times[calls[0][0]]) < 5 or time.perf_counter() - t0 < args.window:
            for k, fn in calls:
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - a) * 1e3)
        res = {k: summary(v) for k, v in times.items()}
        reps = len(times[calls[0][0]])
        res["stages_ms_per_round"] = {}
        for cat in STAGES:
            ms, cnt = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
            if cnt.value:
                res["stages_ms_per_round"][cat] = round(ms.value / reps, 4)
        L.gft_profile_enable(eh, 0)
        return res

    def rank_of(off_ptr, term_ptr, n, nt, weights):
        occ, docs, first = (torch.zeros(nt, dtype=torch.int64, device="cuda") for _ in range(3))
        score = torch.zeros(n, dtype=torch.int64, device="cuda")
        ti, ts = (torch.zeros(4096, dtype=torch.int64, device="cuda") for _ in range(2))
        mx, n_top = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize()

        def stats():
            assert PL.gft_term_stats_device(ph, off_ptr, term_ptr, n, nt, 0, 0, occ.data_ptr(), docs.data_ptr(), first.data_ptr()) == 0

        def score_call(flags):
            assert L.gft_score_docs_device(eh, off_ptr, term_ptr, n, nt, weights.ctypes.data, flags, score.data_ptr(), C.byref(mx)) == 0

        def top(k):
            assert L.gft_top_docs_device(eh, score.data_ptr(), n, k, 0, ti.data_ptr(), ts.data_ptr(), C.byref(n_top)) == 0
        res = measure([("term_stats", stats), ("score", lambda: score_call(0)), ("score_distinct", lambda: score_call(_lib.GFT_SCORE_DISTINCT))])
        res["term_stats_from"] = "parent" if args.parent else "this library"
        res["score_over_term_stats"] = round(res["score"]["median_ms"] / res["term_stats"]["median_ms"], 3)
        res["score_distinct_over_term_stats"] = round(res["score_distinct"]["median_ms"] / res["term_stats"]["median_ms"], 3)
        score_call(0)
        res.update(documents=n, n_terms=nt, entries=int(occ.sum().item()), max_score=int(mx.value), nonzero_scores=int((score != 0).sum().item()))
        t = measure([("read_scores", lambda: score.max().item()), ("top_10", lambda: top(10)), ("top_4096", lambda: top(4096))])
        t["select_passes"] = max(1, (int(mx.value).bit_length() + rank_shape()["digit_bits"] - 1) // rank_shape()["digit_bits"])
        t["top_10_over_read"] = round(t["top_10"]["median_ms"] / t["read_scores"]["median_ms"], 2)
        t["top_4096_over_read"] = round(t["top_4096"]["median_ms"] / t["read_scores"]["median_ms"], 2)
        sc = score.cpu().numpy()
        order = np.lexsort((np.arange(n), -sc))[:4096]
        order = order[sc[order] > 0]
        t["same_as_host"] = bool(int(n_top.value) == order.size and (ti[:order.size].cpu().numpy() == order).all())
        res["top"] = t
        return res

    class Raw:
        """library-owned device memory as an array-interface object"""

        def __init__(self, ptr, count, typestr):
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    def as_tensor(ptr, count, dtype):
        if not count:
            return torch.zeros(0, dtype=dtype, device="cuda")
        return torch.as_tensor(Raw(ptr, count, "<i8" if dtype == torch.int64 else "<i4"), device="cuda").clone()

    lists = {}

    def batch(label, text, off):
        n = int(off.numel()) - 1
        m = _lib.GftMatches()
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())           # (builds the dictionary with the first batch)
        nt = int(L.gft_n_terms(eh))
        assert L.gft_scan_device(eh, text.data_ptr(), off.data_ptr(), n, _lib.GFT_FOLD_ASCII, C.byref(m)) == 0
        d_off, d_term = as_tensor(m.match_off, n + 1, torch.int64), as_tensor(m.term_id, int(m.n_matches), torch.int32)
        weights = (np.arange(nt, dtype=np.uint32) % 7 + 1).astype(np.uint32)
        lists[label] = rank_of(d_off.data_ptr(), d_term.data_ptr(), n, nt, weights)

    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    batch("a: documents of 4 KB, canonical match list", text, off)
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    del text, off
    torch.cuda.empty_cache()
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    batch("b: lines of 100 bytes, canonical match list", lined, loff)

    # (c) the finder's call against the host route
    data = lined[:int(loff[args.lines].item())].cpu().numpy().tobytes()
    del lined
    res = {}
    for k in (10, 4096):
        f.TopLines(data, k=k)
        v, h = [], []
        for _ in range(5):
            a = time.perf_counter()
            got, _ = f.TopLines(data, k=k)
            b = time.perf_counter()
            idx, spans, _ = f.SpansLines(data)
            cnt = np.zeros(args.lines, dtype=np.int64)
            cnt[idx.astype(np.int64)] = [len(s) for s in spans]
            kk = min(k, int(np.count_nonzero(cnt)))
            part = np.argpartition(-cnt, kk - 1)[:kk] if kk else np.zeros(0, np.int64)
            c = time.perf_counter()
            v.append((b - a) * 1e3)
            h.append((c - b) * 1e3)
        thr = int(cnt[part].min()) if kk else 0
        res["k_%d" % k] = {"top_lines": summary(v), "host_route": summary(h), "host_over_top_lines": round(statistics.median(h) / statistics.median(v), 1),
                           "same_scores_above_threshold": sorted(d for d, s, _ in got if s > thr) == sorted(int(d) for d in part if cnt[d] > thr)}
    out = {"tool": "bench_rank", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "terms": args.terms, "exprs": args.exprs, "lines": args.lines, "window_s": args.window, "parent": bool(args.parent)},
           "shape": rank_shape(), "lists": lists, "top_lines": res}
    if args.parent:
        PL.gft_engine_destroy(ph)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
