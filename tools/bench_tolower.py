#!/usr/bin/env python
"""What a batch that leaves ASCII costs: the finder's repeat through the device's ToLower kernels (gft_tolower.hip) against
the host repeat it replaces (GFT_DEVICE_TOLOWER=0: text down, ToLower per document on one thread, scan, bitmap up), in the
same run on the same box.  The mixed-alphabet workload of bench.py (--docs shrinks it), device-resident, with an upper-case
E-acute planted (a) in one document, (b) in every document.  Per planting:

  * Finder.ProcessDevice per batch on both finders, the two settings interleaved batch by batch, median of --steps batches
    after --warmup (HIP events around the call: it is synchronous);
  * the three lowering launches from gft_profile_read in a pass of their own, and their share of the bound of
    3 x text bytes (two reads, one write) at 8 TB/s.

Prints one JSON line and writes it to --out.

    python tools/bench_tolower.py [--docs 1000000] [--steps 10] [--warmup 2] [--out profiles/tolower_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=10_000)
    ap.add_argument("--exprs", type=int, default=1_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "tolower_bench.json"))
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10 (the figures are medians)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tolower.py measures on the GPU: no HIP device here")
    from gofindthem_amd import _lib
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    from gofindthem_amd.workload import Workload, make_expressions

    dev = torch.device("cuda", 0)
    wl = Workload(args.terms, alphabet="mixed")
    exprs = make_expressions(wl.terms(), args.exprs, inord_fraction=0.0, cover=True)
    L = _lib.load()

    def make_finder(device_tolower):
        if device_tolower:
            os.environ.pop("GFT_DEVICE_TOLOWER", None)
        else:
            os.environ["GFT_DEVICE_TOLOWER"] = "0"       # (read when the finder is created)
        f = Finder(GpuEngine.__new__(GpuEngine), EmptyRgxEngine(), caseSensitive=False, device=0)
        f.AddExpressions(exprs)
        f.ForceBuild()
        assert L.gft_set_stream(f.engine_handle(), torch.cuda.current_stream().cuda_stream) == 0
        return f

    finders = {"host": make_finder(False), "device": make_finder(True)}
    os.environ.pop("GFT_DEVICE_TOLOWER", None)
    n = args.docs
    text, doc_off = wl.docs_device(0, n, device=dev)
    text_bytes = int(doc_off[n].item() - doc_off[0].item())
    words = (args.exprs + 31) // 32
    bitmaps = {k: torch.zeros((n, words), dtype=torch.int32, device=dev) for k in finders}

    def plant(docs):
        """C3 89 over the first three ASCII bytes in a row among a document's first 18"""
        start = doc_off[:-1][docs]
        assert bool(((doc_off[1:][docs] - start) >= 18).all()), "documents shorter than 18 bytes"
        win = text[(start[:, None] + torch.arange(18, device=dev)[None, :])]
        ok = (win[:, :-2] < 128) & (win[:, 1:-1] < 128) & (win[:, 2:] < 128)
        assert bool(ok.any(dim=1).all()), "a document without three ASCII bytes in a row at its start"
        at = start + ok.to(torch.int8).argmax(dim=1)
        text[at] = 0xC3
        text[at + 1] = 0x89

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    results = {}
    for planting, docs in (("one_document", torch.tensor([n // 2], device=dev)), ("every_document", torch.arange(n, device=dev))):
        plant(docs)
        times = {k: [] for k in finders}
        before = {k: f.lowered_batches() for k, f in finders.items()}
        for step in range(args.warmup + args.steps):
            for k, f in finders.items():                 # the two settings alternate inside every step
                a.record()
                f.ProcessDevice(text.data_ptr(), doc_off.data_ptr(), n, bitmaps[k].data_ptr())
                b.record()
                b.synchronize()
                if step >= args.warmup:
                    times[k].append(a.elapsed_time(b))
        steps = args.warmup + args.steps
        after = {k: f.lowered_batches() for k, f in finders.items()}
        assert (after["device"][0] - before["device"][0], after["device"][1] - before["device"][1]) == (steps, 0)
        assert (after["host"][0] - before["host"][0], after["host"][1] - before["host"][1]) == (0, steps)
        assert torch.equal(bitmaps["host"], bitmaps["device"]), "the two paths give different bitmaps"
        # the launches alone, profiled (a pass of its own: an event pair around every launch costs host time)
        eh = finders["device"].engine_handle()
        assert L.gft_profile_enable(eh, 1) == 0 and L.gft_profile_reset(eh) == 0
        for _ in range(args.steps):
            finders["device"].ProcessDevice(text.data_ptr(), doc_off.data_ptr(), n, bitmaps["device"].data_ptr())
        kernels = {}
        for name in ("lower_count", "lower_scan", "lower_write", "scan", "solve"):
            ms, cnt = C.c_double(), C.c_uint64()
            assert L.gft_profile_read(eh, name.encode(), C.byref(ms), C.byref(cnt)) == 0
            kernels[name] = {"ms": round(ms.value / max(cnt.value, 1), 4), "launches": int(cnt.value)}
        L.gft_profile_enable(eh, 0)
        lower_ms = sum(kernels[k]["ms"] for k in ("lower_count", "lower_scan", "lower_write"))
        bound_ms = 3 * text_bytes / HBM_BYTES_PER_S * 1e3
        med = {k: statistics.median(t) for k, t in times.items()}
        results[planting] = {
            "ms_median": {"host_repeat_GFT_DEVICE_TOLOWER_0": round(med["host"], 3), "device_repeat": round(med["device"], 3)},
            "ms_min_max": {k: [round(min(t), 3), round(max(t), 3)] for k, t in times.items()},
            "device_over_host": round(med["device"] / med["host"], 5),
            "profiled_launches": kernels,
            "lowering_launches_ms": round(lower_ms, 4), "bound_ms_3x_text_at_8TBps": round(bound_ms, 4),
            "fraction_of_bound": round(bound_ms / lower_ms, 4) if lower_ms > 0 else None,
        }
    out = {"tool": "bench_tolower", "device": torch.cuda.get_device_name(0),
           "config": {"docs": n, "terms": args.terms, "exprs": args.exprs, "alphabet": "mixed", "text_bytes": text_bytes,
                      "steps": args.steps, "warmup": args.warmup},
           "plantings": results}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    for f in finders.values():
        f.close()


if __name__ == "__main__":
    main()
