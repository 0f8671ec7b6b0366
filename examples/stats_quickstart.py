#!/usr/bin/env python3
"""Which keywords ever fire: a blob of text lines goes up once, the scan, the rows and the histogram of the keyword occurrences are
computed where the blob lies, and two counters and a line number per keyword come back -- how often it occurred, on how many
lines, and on which line first.  Then how many lines every expression is true on.  Needs a HIP device, no files.

    python examples/stats_quickstart.py
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
lines = log.decode(errors="replace").splitlines()


def table(stats):
    for kw, (occ, docs, first) in sorted(stats.items(), key=lambda kv: -kv[1][0]):
        print("    %-10s %3d times on %2d lines, first on line %d: %s" % (kw.decode(errors="replace"), occ, docs, first, lines[first]))


stats, lowered = f.TermStatsLines(log)
print("the keywords that made an expression true%s:" % (" (the batch was lowered for the scan)" if lowered else ""))
table(stats)

stats, _ = f.TermStatsLines(log, kept=False)
print("every occurrence of every keyword, whatever the expressions say:")
table(stats)
silent = sorted(set(k.encode() for k in f.GetKeywords()) - set(stats))
print("keywords that never fired: %s" % ", ".join(k.decode() for k in silent))

print("lines every expression is true on:")
for i, n in enumerate(f.CountExpressions(log).tolist()):
    src, tag, _ = f.expression(i, tree=False)
    print("    %2d lines  [%s] %s" % (n, tag, src))
