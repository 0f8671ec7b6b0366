#!/usr/bin/env python
"""What the term statistics cost: gft_term_stats_device (gft_stats.hip) over the lists the calls before it make, against the scan
that makes the list and against the only route there was to these numbers -- the term and offset arrays downloaded, numpy.bincount
and a unique over (document, term) on the host.

  (a) the canonical match list of bench.py's headline batch (--docs documents of about 4 KB);
  (b) the same text cut into lines of about 100 bytes;
  (c) the span list of (a) (the kept matches), and apart from it a list of the same shape with ONE term in every entry: the hot term.
Each: the statistics call, gft_scan_device alone and (once) the host route, alternating in the same run; host clock round calls that
end in a stream synchronise, medians, minimum and maximum over the repeats that fill --window seconds; the stages' own times from
gft_profile_read.  With --variant LIB (tools/build_variant.sh with GFT_VARIANT_SRC=gft_stats.hip -DGFT_STATS_NO_COMBINE) the same
lists also go through the kernel without the LDS combining: one global atomic per entry.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_term_stats.py [--docs 200000] [--variant gofindthem_amd/libgft_nocombine.so] [--out profiles/term_stats_bench.json]
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
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per list")
    ap.add_argument("--variant", default=None, help="a library built with -DGFT_STATS_NO_COMBINE")
    ap.add_argument("--out", default=os.path.join("profiles", "term_stats_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_term_stats.py measures on the GPU: no HIP device here")
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
    V, vh = None, C.c_void_p()
    if args.variant:
        V = C.CDLL(os.path.abspath(args.variant))
        V.gft_engine_create.argtypes, V.gft_engine_create.restype = [C.c_void_p, C.c_int], C.c_int
        V.gft_term_stats_device.argtypes = _lib.SYMBOLS["gft_term_stats_device"][1]
        V.gft_engine_destroy.argtypes = [C.c_void_p]
        assert V.gft_engine_create(C.byref(vh), -1) == 0

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "repeats": len(v)}

    def stats_of(name, off_ptr, term_ptr, n, nt, scan=None, host_arrays=None):
        occ, docs, first = (torch.zeros(nt, dtype=torch.int64, device="cuda") for _ in range(3))
        torch.cuda.synchronize()

        def stats(lib=L, h=eh):
            assert lib.gft_term_stats_device(h, off_ptr, term_ptr, n, nt, 0, 0, occ.data_ptr(), docs.data_ptr(), first.data_ptr()) == 0
        calls = [("stats", stats)]
        if V is not None:
            calls.append(("stats_no_combine", lambda: stats(V, vh)))
        for _ in range(2):
            for _, fn in calls:
                fn()
        ref = occ.clone(), docs.clone(), first.clone()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        times = {k: [] for k, _ in calls}
        t0 = time.perf_counter()
        while len(times["stats"]) < 5 or time.perf_counter() - t0 < args.window:
            for k, fn in calls:
                torch.cuda.synchronize()
                a = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - a) * 1e3)
        reps = len(times["stats"])
        res = {"documents": n, "n_terms": nt, "entries": int(occ.sum().item()), "distinct_terms": int((occ != 0).sum().item())}
        for k, v in times.items():
            res[k] = summary(v)
        for cat in ("stats_check", "stats_count"):
            ms, cnt = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
            res[cat + "_ms"] = round(ms.value / reps, 4)
        L.gft_profile_enable(eh, 0)
        if V is not None:
            stats(V, vh)
            res["no_combine_same_counts"] = all(bool(torch.equal(a, b)) for a, b in zip(ref, (occ, docs, first)))
            res["no_combine_over_stats"] = round(res["stats_no_combine"]["median_ms"] / res["stats"]["median_ms"], 2)
        res["ns_per_entry"] = round(res["stats"]["median_ms"] * 1e6 / max(res["entries"], 1), 4)
        if scan is not None:
            v = []
            for _ in range(5):
                torch.cuda.synchronize()
                a = time.perf_counter()
                scan()
                v.append((time.perf_counter() - a) * 1e3)
            res["scan_device"] = summary(v)
            res["stats_over_scan"] = round(res["stats"]["median_ms"] / res["scan_device"]["median_ms"], 4)
        if host_arrays is not None:
            d_off, d_term = host_arrays()
            torch.cuda.synchronize()
            a = time.perf_counter()
            off = d_off.cpu().numpy()
            term = d_term.cpu().numpy()
            b = time.perf_counter()
            h_occ = np.bincount(term, minlength=nt)
            doc = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
            pairs = np.unique(doc * nt + term)
            h_docs = np.bincount(pairs % nt, minlength=nt)
            c = time.perf_counter()
            res["host_route"] = {"download_ms": round((b - a) * 1e3, 1), "numpy_ms": round((c - b) * 1e3, 1), "bytes_down": int(off.nbytes + term.nbytes)}
            res["host_over_stats"] = round((c - a) * 1e3 / res["stats"]["median_ms"], 1)
            res["same_counts_as_host"] = bool((h_occ == ref[0].cpu().numpy()).all() and (h_docs == ref[1].cpu().numpy()).all())
        return res

    class Raw:
        """library-owned device memory as an array-interface object"""

        def __init__(self, ptr, count, typestr):
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    def as_tensor(ptr, count, dtype):
        """a copy of library-owned device memory as a tensor (the next scan reuses the buffers)"""
        if not count:
            return torch.zeros(0, dtype=dtype, device="cuda")
        return torch.as_tensor(Raw(ptr, count, "<i8" if dtype == torch.int64 else "<i4"), device="cuda").clone()

    nt = int(L.gft_n_terms(eh)) if L.gft_n_terms(eh) else None
    lists = {}

    def batch(label, text, off, with_spans):
        nonlocal nt
        n = int(off.numel()) - 1
        m = _lib.GftMatches()

        def scan():
            assert L.gft_scan_device(eh, text.data_ptr(), off.data_ptr(), n, _lib.GFT_FOLD_ASCII, C.byref(m)) == 0
        bm = torch.zeros((n, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f.ProcessDevice(text.data_ptr(), off.data_ptr(), n, bm.data_ptr())           # (builds the dictionary with the first batch)
        nt = int(L.gft_n_terms(eh))
        scan()
        nm = int(m.n_matches)
        d_off, d_term = as_tensor(m.match_off, n + 1, torch.int64), as_tensor(m.term_id, nm, torch.int32)
        lists[label + ": canonical match list"] = stats_of(label, d_off.data_ptr(), d_term.data_ptr(), n, nt, scan, lambda: (d_off, d_term))
        if with_spans:
            so, st, ln, tm, lowered = f.SpansDevice(text, off, bm)
            lists[label + ": span list (kept matches)"] = stats_of(label, so.data_ptr(), tm.data_ptr(), n, nt, None, lambda: (so, tm))
            hot = torch.full_like(tm, 7)
            lists[label + ": span list, one hot term"] = stats_of(label, so.data_ptr(), hot.data_ptr(), n, nt)

    text, off = w.docs_device(0, args.docs)
    n_bytes = int(off[-1].item())
    batch("a: documents of 4 KB", text, off, True)
    lined = torch.zeros(n_bytes + 64, dtype=torch.uint8, device="cuda")
    lined[:n_bytes] = text[:n_bytes]
    lined[99:n_bytes:100] = 10
    del text, off
    torch.cuda.empty_cache()
    loff = f.SplitLinesDevice(lined, n_bytes, 0)
    batch("b: lines of 100 bytes", lined, loff, False)
    out = {"tool": "bench_term_stats", "device": torch.cuda.get_device_name(0),
           "config": {"docs": args.docs, "terms": args.terms, "exprs": args.exprs, "window_s": args.window, "variant": args.variant},
           "shape": {k: int(v) for k, v in __import__("gofindthem_amd.engine", fromlist=["stats_shape"]).stats_shape().items()}, "lists": lists}
    if V is not None:
        V.gft_engine_destroy(vh)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
