#!/usr/bin/env python3
"""Whole-word matching: short keywords such as "err", "out" or "served" fire inside other words when keywords are substrings.  With
Finder(whole_words=True) an occurrence counts only where it stands at word borders -- letters, marks, digits and `_` on both sides
of an edge make it part of a longer word --, and everything built on the rows and the spans follows: what is selected, what is
highlighted, what is counted.  The log of the other quickstarts, with the option off and on.  Needs a HIP device, no files.

    python examples/words_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402

log = """09:00:01 service started
09:00:07 ERROR disk full on /var
09:00:09 error sending mail, will retry
09:01:12 connection refused by 10.0.0.7
09:01:15 request served in 12 ms
09:02:40 Timeout after 30 s, ERROR reported
09:03:02 CAFÉ gateway in İstanbul: ERROR reported
""".encode()

for whole in (False, True):
    f = Finder(GpuEngine(), EmptyRgxEngine(), False, whole_words=whole)
    f.AddExpressionWithTag('"err" or "error"', "alerts")
    f.AddExpressionWithTag('"out" or "in" or "port"', "short words")
    f.AddExpressionWithTag('"serve" or "fuse"', "stems")
    print("whole_words=%s" % whole)
    picked, off, idx = f.SelectLines(log)
    print("  selects lines %s" % idx.tolist())
    marked, lowered = f.HighlightLines(log, open=b"[", close=b"]")
    for line in marked.decode(errors="replace").splitlines():
        if "[" in line:
            print("    " + line)
    stats, _ = f.TermStatsLines(log)
    print("  keyword: (occurrences, lines, first line)  %s" % {k.decode(): v for k, v in sorted(stats.items())})
    f.close()
