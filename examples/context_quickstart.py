#!/usr/bin/env python3
"""grep -n -C1 on the device: the log of select_quickstart.py goes up once, the finder's rows are made where it lies, and only the
lines that hit and the lines round them come back -- with their line numbers, which of them are hits (grep's `:`) and which are
context (`-`), and where one group of consecutive lines ends and the next begins (`--`).  Needs a HIP device, no files.

    python examples/context_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402

f = Finder(GpuEngine(), EmptyRgxEngine(), False)
f.AddExpressionWithTag('"error" and not "retry"', "alerts")
f.AddExpressionWithTag('"timeout" or "refused"', "network")

log = b"""09:00:01 service started
09:00:07 ERROR disk full on /var
09:00:09 error sending mail, will retry
09:01:12 connection refused by 10.0.0.7
09:01:15 request served in 12 ms
09:02:40 Timeout after 30 s, ERROR reported
"""


def grep_n(data, out_off, doc_idx, kind, group_off):
    """the kept lines as grep -n prints them"""
    starts = set(group_off[1:-1].tolist())
    for k in range(len(doc_idx)):
        if k in starts:
            print("--")
        line = data[int(out_off[k]):int(out_off[k + 1])].decode().rstrip("\n")
        print("%d%s%s" % (doc_idx[k] + 1, ":" if kind[k] else "-", line))


for title, want, mode, before, after in (('grep -n -C1, tag "alerts"', f.want_mask(tags=["alerts"]), "any", 1, 1),
                                         ('grep -n -A1, tag "network"', f.want_mask(tags=["network"]), "any", 0, 1),
                                         ("grep -n -v -B1, any expression", None, "none", 1, 0)):
    print("# " + title)
    grep_n(*f.ContextLines(log, before, after, want, mode))
