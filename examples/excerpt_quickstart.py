#!/usr/bin/env python3
"""Showing what hit: a blob of text lines goes up once, the finder's rows, the spans of the keyword occurrences that made an
expression true and the excerpts round them are computed where the blob lies, and only the excerpts come back -- a few bytes of
context on either side of every hit, neighbouring hits in one excerpt, cut on rune borders.  Needs a HIP device, no files.

    python examples/excerpt_quickstart.py
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


def bracketed(text, hits):
    """the excerpt with every hit in brackets (hits may nest or repeat: the brackets go in from the back)"""
    marks = sorted({(e, "]") for _, e, _ in hits} | {(s, "[") for s, _, _ in hits}, key=lambda m: (-m[0], m[1] == "]"))
    for at, mark in marks:
        text = text[:at] + mark.encode() + text[at:]
    return text.decode(errors="replace")


for before, after in ((8, 8), (12, 3)):
    idx, excerpts, lowered = f.ExcerptLines(log, before=before, after=after)
    print("%d bytes in front of a hit, %d behind it%s:" % (before, after, " (the batch was lowered for the scan)" if lowered else ""))
    for k, d in enumerate(idx.tolist()):
        for start, text, hits in excerpts[k]:
            print("    line %d, byte %3d: ...%s..." % (d, start, bracketed(text, hits)))

print('only the tag "network", the whole line as the window:')
idx, excerpts, _ = f.ExcerptLines(log, before=0xFFFFFFFF, after=0xFFFFFFFF, want=f.want_mask(tags=["network"]))
for k, d in enumerate(idx.tolist()):
    for start, text, hits in excerpts[k]:
        print("    line %d: %s" % (d, bracketed(text, hits).rstrip("\n")))
