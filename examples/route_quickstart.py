#!/usr/bin/env python3
"""Routing lines to their tags: a blob of log lines goes up once, the finder's rows are made where it lies, and one call sorts the
lines into one run per tag -- a line under every tag it carries, the untagged ones in a rest bucket of their own.  One blob, its
offsets and the line numbers come back.  Needs a HIP device, no files.

    python examples/route_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402

f = Finder(GpuEngine(), EmptyRgxEngine(), False)
f.AddExpressionWithTag('"error" and not "retry"', "alerts")
f.AddExpressionWithTag('"timeout" or "refused"', "network")
f.AddExpressionWithTag('"disk" or "/var"', "storage")

log = b"""09:00:01 service started
09:00:07 ERROR disk full on /var
09:00:09 error sending mail, will retry
09:01:12 connection refused by 10.0.0.7
09:01:15 request served in 12 ms
09:02:40 Timeout after 30 s, ERROR reported
"""

parts, idx = f.RouteLines(log, rest=True)
for name, part, lines in zip(f.tags() + ["(no tag)"], parts, idx):
    print("%s: lines %s" % (name, lines.tolist()))
    for line in part.decode().splitlines():
        print("    " + line)

docs, nbytes = f.CountLines(log)
print("histogram:", dict(zip(f.tags(), zip(docs.tolist(), nbytes.tolist()))))
