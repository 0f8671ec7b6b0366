#!/usr/bin/env python3
"""Keeping the lines that hit: a blob of text lines goes up once, the finder's rows are made where it lies, and only the lines
whose rows hit the mask -- with their offsets and their line numbers -- come back.  Needs a HIP device, no files.

    python examples/select_quickstart.py
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

for title, want, mode in (("any expression", None, "any"), ('tag "alerts"', f.want_mask(tags=["alerts"]), "any"),
                          ("both expressions", f.want_mask(indices=[0, 1]), "all"), ("no expression", None, "none")):
    data, out_off, doc_idx = f.SelectLines(log, want, mode)
    print("%s: lines %s" % (title, doc_idx.tolist()))
    for k in range(len(doc_idx)):
        print("    " + data[int(out_off[k]):int(out_off[k + 1])].decode().rstrip("\n"))
