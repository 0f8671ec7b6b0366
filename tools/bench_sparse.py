#!/usr/bin/env python
"""What a host consumer of a batch pays for its results: the dense bitmap against the sparse lists ("Sparse
batch results").  The headline workload of bench.py (same generator arguments; --docs shrinks it), device-resident corpus,
per step, the three legs in turn inside one run so that they see the same machine:

  1. ProcessDevice alone (the existing path);
  2. ProcessDevice + download of the dense bitmap into pinned host memory: what a host consumer pays today;
  3. ProcessDevice + CompactDevice + download of row_off, expr_idx and tag_id into pinned host memory (the caller's
     protocol: the call hands the total back, the two lists are downloaded at that length);
  4. the three compaction launches from gft_profile_read in a pass of their own (profiling brackets every launch with
     events), the bytes each moves and the rate that makes.

HIP events on the engine's stream, median over --steps steps after --warmup.  Prints one JSON line and writes it to --out.

    python tools/bench_sparse.py [--docs 1000000] [--steps 20] [--warmup 3] [--out profiles/sparse_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--inord", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tags", type=int, default=8, help="the expressions are registered under this many tags in turn")
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 (the figures are medians)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sparse.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    dev = torch.device("cuda", 0)
    wl = Workload(args.terms)
    exprs = make_expressions(wl.terms(), args.exprs, inord_fraction=args.inord, cover=True)
    finder = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), caseSensitive=False, device=0)
    per_tag = (len(exprs) + args.tags - 1) // args.tags
    for k in range(0, len(exprs), per_tag):
        finder.AddExpressionsWithTag(exprs[k:k + per_tag], "tag%d" % (k // per_tag))
    finder.ForceBuild()
    L = _lib.load()
    eh = finder.engine_handle()
    assert L.gft_set_stream(eh, torch.cuda.current_stream().cuda_stream) == 0
    n = args.docs
    text, doc_off = wl.docs_device(0, n, device=dev)
    words = (args.exprs + 31) // 32
    bitmap = torch.zeros((n, words), dtype=torch.int32, device=dev)
    row_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def process():
        finder.ProcessDevice(text.data_ptr(), doc_off.data_ptr(), n, bitmap.data_ptr())

    for _ in range(4):                     # sizes learnt (unit table, match pool)
        process()
    total = finder.CompactDevice(bitmap.data_ptr(), n, row_off.data_ptr(), None, None, 0)
    cap = total + total // 8 + 1024        # (one corpus: every step has this total; a caller sizes from the batches before)
    expr_idx = torch.zeros(cap, dtype=torch.int32, device=dev)
    tag_id = torch.zeros(cap, dtype=torch.int32, device=dev)
    h_bitmap = torch.empty((n, words), dtype=torch.int32).pin_memory()
    h_row_off = torch.empty(n + 1, dtype=torch.int64).pin_memory()
    h_expr_idx = torch.empty(cap, dtype=torch.int32).pin_memory()
    h_tag_id = torch.empty(cap, dtype=torch.int32).pin_memory()

    def leg1():
        process()

    def leg2():
        process()
        h_bitmap.copy_(bitmap, non_blocking=True)

    def leg3():
        process()
        t = finder.CompactDevice(bitmap.data_ptr(), n, row_off.data_ptr(), expr_idx.data_ptr(), tag_id.data_ptr(), cap)
        assert t <= cap
        h_row_off.copy_(row_off, non_blocking=True)
        h_expr_idx[:t].copy_(expr_idx[:t], non_blocking=True)
        h_tag_id[:t].copy_(tag_id[:t], non_blocking=True)

    legs = [leg1, leg2, leg3]
    times = [[] for _ in legs]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for step in range(args.warmup + args.steps):
        for k, leg in enumerate(legs):     # the legs alternate inside every step
            a.record()
            leg()
            b.record()
            b.synchronize()
            if step >= args.warmup:
                times[k].append(a.elapsed_time(b))
    # the two downloads carry the same answer
    ro = h_row_off.numpy().astype(np.uint64)
    assert int(ro[n]) == total
    counts = np.diff(ro)
    bits = np.unpackbits(h_bitmap.numpy().view(np.uint8).reshape(n, words * 4)[:4096], axis=1, bitorder="little")[:, :args.exprs]
    assert np.array_equal(bits.sum(axis=1), counts[:bits.shape[0]]), "sparse and dense results differ"
    assert np.array_equal(np.nonzero(bits)[1], h_expr_idx.numpy()[:int(ro[bits.shape[0]])]), "sparse and dense results differ"

    # leg 4: the launches alone, profiled (a pass of its own: an event pair around every launch costs host time)
    assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
    for _ in range(args.steps):
        process()                          # (the solver kernel of the same run: the yardstick for the three launches)
        finder.CompactDevice(bitmap.data_ptr(), n, row_off.data_ptr(), expr_idx.data_ptr(), tag_id.data_ptr(), cap)
    bm_bytes = n * words * 4
    moved = {"compact_count": bm_bytes + 4 * n,
             "compact_scan": 2 * 4 * n + 8 * (n + 1),
             "compact_fill": bm_bytes + 8 * n + 2 * 4 * total}
    kernels = {}
    for name, nbytes in moved.items():
        ms, cnt = C.c_double(), C.c_uint64()
        assert L.gft_profile_read(eh, name.encode(), C.byref(ms), C.byref(cnt)) == 0
        per = ms.value / max(cnt.value, 1)
        kernels[name] = {"ms": round(per, 4), "launches": int(cnt.value), "bytes": nbytes,
                         "GBps": round(nbytes / (per * 1e-3) / 1e9, 1) if per > 0 else None}
    for name in ("scan", "solve"):
        ms, cnt = C.c_double(), C.c_uint64()
        assert L.gft_profile_read(eh, name.encode(), C.byref(ms), C.byref(cnt)) == 0
        kernels[name] = {"ms": round(ms.value / max(cnt.value, 1), 4), "launches": int(cnt.value)}
    L.gft_profile_enable(eh, 0)

    med = [statistics.median(t) for t in times]
    out = {
        "tool": "bench_sparse", "device": torch.cuda.get_device_name(0),
        "config": {"docs": n, "terms": args.terms, "exprs": args.exprs, "inord": args.inord, "tags": len(finder.tags()),
                   "steps": args.steps, "warmup": args.warmup},
        "hits_per_doc": {"mean": round(float(counts.mean()), 3), "max": int(counts.max()), "total": total},
        "bytes": {"dense_bitmap": bm_bytes, "sparse": 8 * (n + 1) + 2 * 4 * total},
        "ms_median": {"process_device": round(med[0], 4), "process_device_dense_download": round(med[1], 4),
                      "process_device_compact_sparse_download": round(med[2], 4)},
        "ms_min_max": [[round(min(t), 4), round(max(t), 4)] for t in times],
        "sparse_over_dense": round(med[2] / med[1], 4),
        "dense_download_ms": round(med[1] - med[0], 4), "compact_and_sparse_download_ms": round(med[2] - med[0], 4),
        "profiled_launches": kernels,
        "compaction_launches_ms": round(sum(kernels[k]["ms"] for k in moved), 4),
    }
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    finder.close()


if __name__ == "__main__":
    main()
