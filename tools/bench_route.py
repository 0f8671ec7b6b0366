#!/usr/bin/env python
"""What routing a batch to K buckets in one call costs against K calls of the select: gft_route_docs_device (gft_route.hip) in EVERY
mode over the corpus shape of tools/bench_select.py (--docs documents of about 4 KB) with 8 tags that each hit about an eighth of
the documents (synthetic rows of 8 columns, one per tag), timed in ONE process against

  (a) route_docs_device: one fill call with exact caps -- one read of the rows, one host synchronisation in the middle;
  (b) the eight select_docs_device fill calls that produce the same eight blobs (asserted equal, byte for byte and index for
      index, before anything is timed);
  (c) a plain device-to-device copy of the same number of bytes (torch.Tensor.copy_).

Wall time per call from the host's clock with the device drained before and after (the calls wait for the stream themselves), the
three alternating in every repetition after --warmup rounds; median, minimum and maximum over --reps repetitions.  Then, in a pass
of its own with the profile on, the per-kernel times of (a) from gft_profile_read and the share of route_count + route_place.  A
second figure: the count-only form (a tag histogram, 2 x 9 numbers come down) against downloading the rows and counting with numpy.
No threshold in here; prints one JSON line and writes it to --out.

    python tools/bench_route.py [--docs 200000] [--reps 9] [--warmup 2] [--out profiles/route_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LAUNCHES = ("route_mark", "route_count", "route_scan", "route_place", "route_copy")
K = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--terms", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "route_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_route.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.engine import Engine
    from gofindthem_amd.workload import Workload

    L = _lib.load()
    eng = Engine()
    eh = eng._h
    text, off = Workload(args.terms).docs_device(0, args.docs)
    n = args.docs
    g = torch.Generator(device="cuda")
    g.manual_seed(8)
    bits = (torch.rand((n, K), generator=g, device="cuda") < 1.0 / K).to(torch.int32)
    rows = (bits << torch.arange(K, device="cuda", dtype=torch.int32)).sum(dim=1, dtype=torch.int32).reshape(n, 1).contiguous()
    masks = np.array([[1 << k] for k in range(K)], dtype=np.uint32)
    flat = np.ascontiguousarray(masks.reshape(-1))

    # the sizes, and the outputs of every contender, allocated once
    bd, bb = np.zeros(K + 1, np.uint64), np.zeros(K + 1, np.uint64)
    head = (eh, text.data_ptr(), off.data_ptr(), n, rows.data_ptr(), K, flat.ctypes.data, K, 1, 0, None)
    torch.cuda.synchronize()
    assert L.gft_route_docs_device(*head, None, 0, None, None, 0, bd.ctypes.data, bb.ctypes.data) == 0
    m, total = int(bd[K]), int(bb[K])
    out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    oo = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    di = torch.empty(max(m, 1), dtype=torch.int64, device="cuda")
    sel = []
    for k in range(K):
        mk, tk = int(bd[k + 1] - bd[k]), int(bb[k + 1] - bb[k])
        sel.append((torch.empty(tk + 64, dtype=torch.uint8, device="cuda"), torch.empty(mk + 1, dtype=torch.int64, device="cuda"),
                    torch.empty(max(mk, 1), dtype=torch.int64, device="cuda"), mk, tk))
    src = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
    sm, st = C.c_uint64(0), C.c_uint64(0)

    def route():
        assert L.gft_route_docs_device(*head, out.data_ptr(), total, oo.data_ptr(), di.data_ptr(), m, bd.ctypes.data, bb.ctypes.data) == 0

    def selects():
        for k in range(K):
            o, so, si, mk, tk = sel[k]
            assert L.gft_select_docs_device(eh, text.data_ptr(), off.data_ptr(), n, rows.data_ptr(), K, masks[k].ctypes.data, 0, None, o.data_ptr(), tk,
                                            so.data_ptr(), si.data_ptr(), mk, C.byref(sm), C.byref(st)) == 0

    def copy():
        dst.copy_(src)

    # the same eight blobs
    route()
    selects()
    torch.cuda.synchronize()
    for k in range(K):
        o, so, si, mk, tk = sel[k]
        a, b = int(bd[k]), int(bd[k + 1])
        assert torch.equal(out[int(bb[k]):int(bb[k + 1])], o[:tk]), "bucket %d: bytes differ" % k
        assert torch.equal(di[a:b], si[:mk]) and torch.equal(oo[a:b + 1] - oo[a], so), "bucket %d: entries differ" % k

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    times = {"route": [], "selects": [], "copy": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("route", route), ("selects", selects), ("copy", copy)):
            t = timed(fn)
            if rep >= args.warmup:
                times[name].append(t)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    res = {"a_route": stats(times["route"]), "b_eight_selects": stats(times["selects"]), "c_plain_copy": stats(times["copy"])}
    res["a_over_b"] = round(res["a_route"]["median_ms"] / res["b_eight_selects"]["median_ms"], 3)
    res["a_over_c"] = round(res["a_route"]["median_ms"] / res["c_plain_copy"]["median_ms"], 3)

    # the kernels of (a), in a pass of their own
    assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
    for _ in range(args.reps):
        route()
    kernels = {}
    for cat in LAUNCHES:
        ms, cnt = C.c_double(), C.c_uint64()
        assert L.gft_profile_read(eh, cat.encode(), C.byref(ms), C.byref(cnt)) == 0
        kernels[cat + "_ms"] = round(ms.value / args.reps, 4)               # per call (route_scan: its two scopes together)
    L.gft_profile_enable(eh, 0)
    on_device = sum(kernels.values())
    res["kernels_of_a"] = kernels
    res["count_and_place_share_of_kernels"] = round((kernels["route_count_ms"] + kernels["route_place_ms"]) / on_device, 4) if on_device else None

    # a tag histogram: count only, against rows down and numpy
    def count_only():
        assert L.gft_route_docs_device(*head, None, 0, None, None, 0, bd.ctypes.data, None) == 0
        return bd.copy()

    def numpy_count():
        r = rows.cpu().numpy().view(np.uint32).reshape(-1)
        return np.array([int(((r >> np.uint32(k)) & 1).sum()) for k in range(K)], dtype=np.uint64)
    hist = {"count_only": [], "rows_down_numpy": []}
    for rep in range(args.warmup + args.reps):
        for name, fn in (("count_only", count_only), ("rows_down_numpy", numpy_count)):
            t = timed(fn)
            if rep >= args.warmup:
                hist[name].append(t)
    assert np.diff(count_only()).tolist() == numpy_count().tolist()
    res["histogram"] = {"count_only": stats(hist["count_only"]), "rows_down_numpy": stats(hist["rows_down_numpy"])}

    out_j = {"tool": "bench_route", "device": torch.cuda.get_device_name(0),
             "config": {"docs": n, "text_bytes": int(off[n].item()), "buckets": K, "entries": m, "bytes_routed": total, "reps": args.reps,
                        "warmup": args.warmup}, "result": res}
    line = json.dumps(out_j)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
