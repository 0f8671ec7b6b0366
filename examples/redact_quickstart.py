#!/usr/bin/env python3
"""Marking and masking what hit: a blob of text lines goes up once, the finder's rows and the spans of the keyword occurrences that
made an expression true are computed where it lies, and the lines that hit come back with those bytes masked.  Needs a HIP device,
no files.

    python examples/redact_quickstart.py
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

idx, spans, lowered = f.SpansLines(log)
masked, _ = f.RedactLines(log, mask=b"#")
lines = masked.split(b"\n")
print("lines that hit: %s%s" % (idx.tolist(), " (positions index the lower-cased text)" if lowered else ""))
for k, d in enumerate(idx.tolist()):
    print("    " + lines[d].decode())
    for start, end, keyword in spans[k]:
        print("        bytes %d..%d: %s" % (start, end, keyword.decode()))

# The É and the İ make the finder lower the whole batch before it scans it (strings.ToLower; "İ" shrinks from two bytes to one): the
# calls above answer in the lower-cased text.  source=True maps the spans back: the caller's own bytes, lengths and upper case
idx, spans, lowered = f.SpansLines(log, source=True)
masked, _ = f.RedactLines(log, mask=b"#", source=True)
lines = masked.split(b"\n")
print("the same with source=True (positions index the caller's text, lowered = %s):" % lowered)
for k, d in enumerate(idx.tolist()):
    print("    " + lines[d].decode())
    for start, end, keyword in spans[k]:
        print("        bytes %d..%d: %s" % (start, end, keyword.decode()))

print('only the tag "network":')
masked, _ = f.RedactLines(log, f.want_mask(tags=["network"]))
for d in f.SpansLines(log, f.want_mask(tags=["network"]))[0].tolist():
    print("    " + masked.split(b"\n")[d].decode())
