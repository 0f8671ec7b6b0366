#!/usr/bin/env python3
"""Snippets that read well: a few multi-line log records go up once, and the same hits come back three ways -- as raw windows of
bytes round every hit, as windows grown to the borders of the words their edges cut, and as the lines the hits stand in (no
window at all, every edge walked to its newline: grep's output inside every record).  All three are cut where the records lie;
only the excerpts come down.  Needs a HIP device, no files.

    python examples/snippet_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXPRESSIONS = ['"authenticate" or "password"', '"timeout" and "upstream"']

RECORDS = [
    b"2026-10-21T09:00:07Z auth-7f\nlevel=warn\nfailed to authenticate user administrator from 10.0.0.7\nretrying in 5 s",
    b"2026-10-21T09:00:09Z web-12\nlevel=info\nrequest served in 12 ms",
    b"2026-10-21T09:01:12Z gateway-3\nlevel=error\nupstream timeout after 30 s\nbad password for root\nconnection closed",
    "2026-10-21T09:03:02Z café-1\nlevel=error\nCAFÉ gateway: PASSWORD expired for josé".encode(),
]


def snippets(f, records, **how):
    """the excerpts of the records' hits, per record: [(start_in_record, bytes)]; how: before, after, snap, reach"""
    import torch
    blob = b"".join(records)
    buf = torch.zeros(len(blob) + 64, dtype=torch.uint8, device="cuda")
    buf[:len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    ends = [0]
    for r in records:
        ends.append(ends[-1] + len(r))
    off = torch.tensor(ends, dtype=torch.int64, device="cuda")
    rows = torch.zeros((len(records), (f.n_expressions + 31) // 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    f.ProcessDevice(buf.data_ptr(), off.data_ptr(), len(records), rows.data_ptr())
    span_off, start, length, _, lowered = f.SpansDevice(buf, off, rows, source=True)
    out, exc_off, exc_doc, exc_start = f.ExcerptsDevice(buf, off, span_off, start, length, lowered, True, **how)[:4]
    text, eo = out.cpu().numpy().tobytes(), exc_off.cpu().tolist()
    per_record = [[] for _ in records]
    for k, (d, s) in enumerate(zip(exc_doc.cpu().tolist(), exc_start.cpu().tolist())):
        per_record[d].append((s, text[eo[k]:eo[k + 1]]))
    return per_record


def main():
    from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(EXPRESSIONS)
    for title, how in (("raw windows, 12 bytes either side", dict(before=12, after=12)),
                       ("the same windows, grown to word borders", dict(before=12, after=12, snap="words", reach=64)),
                       ("the lines the hits stand in", dict(before=0, after=0, snap="lines", reach=4096))):
        print(title + ":")
        for d, found in enumerate(snippets(f, RECORDS, **how)):
            for start, text in found:
                print("    record %d, byte %3d: %s" % (d, start, text.decode(errors="replace").replace("\n", "\\n")))
    f.close()


if __name__ == "__main__":
    main()
