#!/usr/bin/env python3
"""Placeholders for the hits: a blob of text lines goes up once, the finder's rows and the spans of the keyword occurrences that
made an expression true are computed where the blob lies, every run of hits is rewritten by its replacement there too -- names
become [NAME], hosts become <host>, a keyword can be deleted --, and the replaced text comes back.  Hits that overlap or touch are
replaced together, once, by the replacement that comes first in the dict.  Needs a HIP device, no files.

    python examples/replace_quickstart.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine  # noqa: E402

f = Finder(GpuEngine(), EmptyRgxEngine(), False)
f.AddExpressionWithTag('"alice" or "bob" or "émile"', "names")
f.AddExpressionWithTag('"10.0.0.7" or "mail.example.org" or "gateway"', "hosts")
f.AddExpressionWithTag('"error" and not "retry"', "alerts")

log = """09:00:01 service started by Alice
09:00:07 ERROR disk full on /var, bob notified
09:00:09 error sending mail to mail.example.org, will retry
09:01:12 connection refused by 10.0.0.7
09:01:15 request served in 12 ms
09:02:40 Timeout after 30 s at the gateway, ERROR reported to ÉMILE
""".encode()

names = {k: b"[NAME]" for k in ("alice", "bob", "émile")}
hosts = {k: b"<host>" for k in ("10.0.0.7", "mail.example.org", "gateway")}
replaced, lowered = f.ReplaceLines(log, {**names, **hosts, "error": b"error"}, want=f.want_mask(tags=["names", "hosts"]))
print("names and hosts replaced%s:" % (" (the batch was lowered for the scan; the caller's bytes are replaced)" if lowered else ""))
for line in replaced.decode(errors="replace").splitlines():
    print("    " + line)

print("every hit of every tag deleted:")
replaced, _ = f.ReplaceLines(log, b"")
for line in replaced.decode(errors="replace").splitlines():
    print("    " + line)
