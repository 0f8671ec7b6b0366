#!/usr/bin/env python3
"""Which lines matched most: a blob of text lines goes up once, the scan, the rows, a score per line and the selection of the best
lines are computed where the blob lies, and three lines come back -- their numbers, their scores and their bytes.  Two keywords
weigh more than the rest.  Needs a HIP device, no files.

    python examples/top_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402

f = Finder(GpuEngine(), EmptyRgxEngine(), False)
f.AddExpressionWithTag('"error" and not "retry"', "alerts")
f.AddExpressionWithTag('"timeout" or "refused"', "network")
f.AddExpressionWithTag('"segfault" or "panic"', "alerts")

log = """09:00:01 service started
09:00:07 ERROR disk full on /var
09:00:09 error sending mail, will retry
09:01:12 connection refused by 10.0.0.7
09:01:15 request served in 12 ms
09:02:40 Timeout after 30 s, ERROR reported
09:03:02 CAFÉ gateway in İstanbul: ERROR reported, error logged
""".encode()


def table(top):
    for line, score, text in top:
        print("    line %d, score %3d: %s" % (line, score, text.decode(errors="replace").rstrip("\n")))


top, lowered = f.TopLines(log, k=3, weights={"timeout": 10, "refused": 5})
print("the three worst lines, a timeout weighing 10 and a refusal 5%s:" % (" (the batch was lowered for the scan)" if lowered else ""))
table(top)

top, _ = f.TopLines(log, k=3, distinct=True)
print("every keyword of a line once, all of them weighing 1:")
table(top)

top, _ = f.TopLines(log, k=3, kept=False)
print("every occurrence of every keyword, whatever the expressions say:")
table(top)
