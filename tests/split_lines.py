"""Blobs of lines for the split's tests (test_split_lines_host.py: the kernels' walk on the host; test_gpu_split_lines.py: the
kernels): a reference written from the contract in include/gft.h that does not call the library, the fixed cases built from the
walk's own borders (gft_debug_split_shape), and seeded random blobs.  No tests in here."""
import functools

import numpy as np

from gofindthem_amd.engine import split_shape

AFTER_NL, JSON_LINES = 0, 1
WS = b" \t\n\r"


def reference(data, mode):
    """the offsets [n + 1] of data's documents ([0] for none): bytes.split with running positions, plus the blank-line rule"""
    pieces = data.split(b"\n")
    starts, pos = [], 0
    for i, p in enumerate(pieces):
        if i == len(pieces) - 1 and not p:           # the final empty piece is dropped
            break
        if mode == AFTER_NL:
            starts.append(pos)
        elif p.strip(WS):                            # a non-blank line; document 0 starts at 0 whatever lies in front
            starts.append(pos if starts else 0)
        pos += len(p) + 1
    return starts + [len(data)] if starts else [0]


def documents(data, mode):
    off = reference(data, mode)
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def sparse_reference(length, planted, mode):
    """the same for a blob of `length` spaces with the bytes of `planted` {position: byte} in it, from the planted bytes alone"""
    starts, line, blank = [], 0, True
    if mode == AFTER_NL:
        starts = [0] + [p + 1 for p in sorted(planted) if planted[p] == 10 and p + 1 < length]
        return starts + [length] if length else [0]
    for p in sorted(planted):
        b = planted[p]
        if blank and b not in WS:
            starts.append(line if starts else 0)
            blank = False
        if b == 10:
            line, blank = p + 1, True
    return starts + [length] if starts else [0]


def _fill(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def short_lines(n, seed):
    rng = np.random.default_rng(seed)
    parts, size = [], 0
    while size < n:
        k = int(rng.integers(0, 1000))
        p = b'{"k":%d}' % k + (b"\r\n" if k % 4 == 0 else b"\n") + (b" \n" if k % 8 == 0 else b"")
        parts.append(p)
        size += len(p)
    return b"".join(parts)[:n]


@functools.lru_cache(maxsize=None)
def fixed_cases():
    """[(name, blob)]: every length and form the contract and the tile / carry-trip borders make special"""
    T, K = split_shape()
    c = [("empty", b""), ("one newline", b"\n"), ("one byte", b"x"), ("one space", b" ")]
    for n in (15, 16, 17, T - 1, T, T + 1):
        body = _fill(b'{"a":1}\n', n)
        c += [("%d bytes" % n, body), ("%d bytes, final newline" % n, body[:-1] + b"\n"), ("%d bytes, no final newline" % n, body[:-1] + b"x"),
              ("%d newlines" % n, b"\n" * n), ("%d spaces" % n, b" " * n), ("%d bytes of whitespace" % n, _fill(b" \t\r\n", n)),
              ("%d bytes, crlf" % n, _fill(b'{"a":1}\r\n', n)), ("%d bytes, indented" % n, _fill(b'  \t{"a":1}\n', n))]
    for at in (T - 1, T, T + 1):
        s = bytearray(b"a" * (2 * T))
        s[at] = 10
        c.append(("newline at %d" % at, bytes(s)))
        s[at + 1] = 32
        c.append(("newline at %d, a space behind it" % at, bytes(s)))
    s = bytearray(b"a" * (2 * T))
    s[T - 1] = 10
    c.append(("a line starts on the tile border", bytes(s)))
    s[T:T + 40] = b" " * 40
    s[T + 40] = 10
    c.append(("a blank line starts on the tile border", bytes(s)))
    c += [("a line of 3 T + 5 bytes in front of a short one", b"a" * (3 * T + 5) + b"\n{}\n"),
          ("a line of 3 T + 5 bytes without a newline", b"{}\n" + b"a" * (3 * T + 5)),
          ("not blank, carried across tiles", b"ab\nx" + b" " * (2 * T + 3) + b"\n{}\n"),
          ("blank so far, carried across tiles", b"ab\n" + b" " * (2 * T + 3) + b'{"a":1}\n{}\n'),
          ("blank from the blob's start", b"\t" * (2 * T + 3) + b"{}\n"),
          ("a second carry trip", short_lines((K + 1) * T + 7, 1))]
    s = bytearray(short_lines((K + 1) * T + 7, 2))
    lo, hi = K * T - 3 * T // 2, K * T + 3 * T // 2
    s[lo:hi] = _fill(b" aaaaaaa", hi - lo)
    c.append(("a line over the carry trip's border", bytes(s)))
    s[lo:hi] = b" " * (hi - lo)
    c.append(("a blank stretch over the carry trip's border", bytes(s)))
    return c


ALPHABET = np.frombuffer(b"\r \ta{", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def random_cases(n=200, seed=20240611):
    """n seeded blobs over the alphabet \\n \\r space \\t a {: lengths up to 1 MB, a newline every 2 to every 5000 bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        length = int(10 ** rng.uniform(0, 6))
        every = 10 ** rng.uniform(np.log10(2), np.log10(5000))
        blob = ALPHABET[rng.integers(0, len(ALPHABET), length)]
        blob = np.where(rng.random(length) < 1.0 / every, np.uint8(10), blob).astype(np.uint8)
        out.append(("random %d" % i, blob.tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def expected(which):
    """{(name, mode): offsets} of fixed_cases() or random_cases(), computed once"""
    cases = fixed_cases() if which == "fixed" else random_cases()
    return {(name, mode): reference(blob, mode) for name, blob in cases for mode in (AFTER_NL, JSON_LINES)}
