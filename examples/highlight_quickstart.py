#!/usr/bin/env python3
"""Showing the hits in the text: a blob of text lines goes up once, the finder's rows and the spans of the keyword occurrences that
made an expression true are computed where the blob lies, the markers are written round the hits there too, and the marked text
comes back -- hits that overlap or touch share one pair of markers.  Then the excerpts round the hits, marked the same way.
Needs a HIP device, no files.

    python examples/highlight_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402

f = Finder(GpuEngine(), EmptyRgxEngine(), False)
f.AddExpressionWithTag('"error" and not "retry"', "alerts")
f.AddExpressionWithTag('"timeout" or "refused"', "network")

log = """09:00:01 service started
09:00:07 ERROR disk full on /var
09:00:09 error sending mail, will retry
09:01:12 connection refused by 10.0.0.7
09:01:15 request served in 12 ms
09:02:40 Timeout after 30 s, ERROR reported
09:03:02 CAFÉ gateway in İstanbul: ERROR reported
""".encode()

marked, lowered = f.HighlightLines(log, open=b"**", close=b"**")
print("the lines that hit, ** round the hits%s:" % (" (the batch was lowered for the scan; the caller's bytes are marked)" if lowered else ""))
for line in marked.decode(errors="replace").splitlines():
    if "**" in line:
        print("    " + line)

print('only the tag "network", in ANSI bold:')
marked, _ = f.HighlightLines(log, open=b"\x1b[1m", close=b"\x1b[0m", want=f.want_mask(tags=["network"]))
for line in marked.decode(errors="replace").splitlines():
    if "\x1b[1m" in line:
        print("    " + line)

print("the excerpts, 8 bytes on either side of a hit, with <em> round the hits:")
idx, excerpts, _ = f.ExcerptLines(log, before=8, after=8, mark=(b"<em>", b"</em>"))
for k, d in enumerate(idx.tolist()):
    for start, text, hits in excerpts[k]:
        print("    line %d, byte %3d: ...%s...   %s" % (d, start, text.decode(errors="replace").rstrip("\n"),
                                                      [text[a:b].decode(errors="replace") for a, b, _ in hits]))
