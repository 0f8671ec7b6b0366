"""Inputs and references shared by tests/test_tolower_host.py (the host walk through the kernels' piece logic) and
tests/test_gpu_tolower.py (the kernels): batches of byte strings for gft_to_lower_device, and what strings.ToLower makes of
them -- the host's gft_to_lower, document by document."""
import ctypes as C
import random

import numpy as np

from gofindthem_amd import _lib

PIECE, CHUNK, UNIT_MAX = 16, 1024, 8192        # bytes per lane, per wave trip, per work unit (csrc/gft_tolower_piece.hpp)

# the code points whose lower-case form has another UTF-8 length (tests/test_tolower_host.py checks the list against
# gft_to_lower over every code point)
SHRINK_2_1 = [0x0130]
SHRINK_3_1 = [0x212A]
SHRINK_3_2 = [0x1E9E, 0x2126, 0x212B, 0x2C62, 0x2C64, 0x2C6D, 0x2C6E, 0x2C6F, 0x2C70, 0x2C7E, 0x2C7F, 0xA78D, 0xA7AA, 0xA7AB,
              0xA7AC, 0xA7AD, 0xA7AE, 0xA7B0, 0xA7B1, 0xA7B2, 0xA7C5]
GROW_2_3 = [0x023A, 0x023E]
LENGTH_CHANGERS = SHRINK_2_1 + SHRINK_3_1 + SHRINK_3_2 + GROW_2_3

RUNES = {2: "É", 3: "ẞ", 4: "\U00010400"}      # upper-case letters of 2, 3 and 4 bytes (the 3-byte one shrinks)
INVALID = [b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xc1\xbf", b"\xf0\x80\x80\x80", b"\x80", b"\xbf",
           b"\xe2\x82", b"\xf0\x9f\x98", b"\xc3"] + [bytes([b]) for b in range(0xF5, 0x100)]


def ref_lower(doc):
    """gft_to_lower: the host's strings.ToLower of one document"""
    L = _lib.load()
    doc = bytes(doc)
    out = C.create_string_buffer(3 * len(doc) + 1)
    need = C.c_uint64()
    assert L.gft_to_lower(doc, len(doc), out, 3 * len(doc) + 1, C.byref(need)) == 0
    return out.raw[:need.value]


def reference(docs):
    """-> (lowered bytes of the batch, offsets u64 [n + 1])"""
    low = [ref_lower(d) for d in docs]
    off = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        off[1:] = np.cumsum([len(x) for x in low], dtype=np.uint64)
    return b"".join(low), off


def py_lower(s):
    """strings.ToLower of valid text, restated rune by rune (no final-sigma rule, no multi-character forms)"""
    return "".join("i" if ch == "İ" else (ch.lower() if len(ch.lower()) == 1 else ch) for ch in s)


def pack(docs, lead=0):
    """blob (lead bytes of filler in front, 64 bytes of readable slack behind) and offsets, doc_off[0] = lead"""
    off = np.zeros(len(docs) + 1, np.uint64)
    off[0] = lead
    if docs:
        off[1:] = lead + np.cumsum([len(d) for d in docs], dtype=np.uint64)
    blob = np.frombuffer(b"\xc3" * lead + b"".join(docs) + b"\x89" * 64, np.uint8).copy()   # (filler that would complete a rune)
    return blob, off


def _ascii(n, seed=0):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ABCDEFXYZ abcdexyz,.09@[`{") for _ in range(n))


def edge_batches():
    """name -> documents (bytes)"""
    out = {}
    sizes = [0, 1, 2, 3, 4, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193, 20000]
    out["sizes_ascii"] = [_ascii(n, n) for n in sizes]
    # the same sizes filled with 2-byte upper-case letters (and one odd byte in front so that runes straddle every piece)
    out["sizes_runes"] = [(b"Z" * (n & 1) + "É".encode() * (n // 2))[:n] for n in sizes] + \
                         [(b"z" + "ẞK\U00010400A".encode() * (n // 11 + 1))[:n] for n in sizes]
    out["empty_run"] = [b""] * 300 + [b"\xc3"] + [b""] * 200 + [b"\x89AB"] + [b""] * 77
    out["only_empty"] = [b""] * 5
    # a 2-, 3- and 4-byte rune starting at each of the offsets 12..16 of a piece, around a 1 KiB boundary and around a unit
    # boundary (a document of UNIT_MAX + 2 bytes is cut into two units of UNIT_MAX / 2 + 1 bytes)
    placed = []
    for L, ch in RUNES.items():
        r = ch.encode()
        for at in list(range(12, 17)) + list(range(CHUNK - 4, CHUNK + 2)) + list(range(3 * CHUNK - 4, 3 * CHUNK + 2)):
            placed.append(_ascii(at, at) + r + _ascii(40, L))
        for at in range(UNIT_MAX // 2 + 1 - 4, UNIT_MAX // 2 + 1 + 2):
            d = _ascii(at, at) + r
            placed.append(d + _ascii(UNIT_MAX + 2 - len(d), L))
        for at in range(7000 - 4, 7000 + 2):         # three units of 7 000 bytes
            d = _ascii(at, at) + r + _ascii(100, 5) + r
            placed.append(d + _ascii(21000 - len(d), L))
    out["rune_placement"] = placed
    # document boundaries that cut a rune after each of its bytes; the neighbour's first bytes would complete it
    cut = []
    for L, ch in RUNES.items():
        r = ch.encode()
        for k in range(1, L):
            for pre in (b"", b"ab", _ascii(15, k), _ascii(1023, k)):
                cut += [pre + r[:k], r[k:] + b"Q"]
    out["cut_runes"] = cut
    lc = []
    for cp in LENGTH_CHANGERS:
        e = chr(cp).encode()
        lc += [e, e * 1000, b"AB" + e + b"CD" + e + e + b"Z"]
    out["length_changers"] = lc
    out["invalid"] = [b"\xff" * 1000] + INVALID + [b"A" + x + b"Z" for x in INVALID] + [b"".join(INVALID) * 20] + \
                     [bytes(range(0x80, 0x100)) * 3, b"\xe2\x82\xac\xe2\x82", b"\xf0\x9f\x98\x80\xf0\x9f\x98", b"\xc3\xc3\x89\x89"]
    return out


def random_docs(n=2000, seed=20260117, max_len=300):
    """documents of 0..max_len bytes drawn from ASCII, Latin-1, Greek / Cyrillic capitals, the length-changers and raw bytes"""
    rng = random.Random(seed)
    greek_cyr = [chr(c) for c in range(0x391, 0x3AA) if c != 0x3A2] + [chr(c) for c in range(0x410, 0x430)]
    latin1 = [chr(c) for c in range(0xC0, 0x100)]
    docs = []
    for _ in range(n):
        want = rng.randint(0, max_len)
        kind = rng.random()
        d = bytearray()
        while len(d) < want:
            x = rng.random()
            if kind < 0.25 or x < 0.5:
                d += bytes([rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ abcdefghijklmnopqrstuvwxyz0123456789.,")])
            elif x < 0.65:
                d += rng.choice(latin1).encode()
            elif x < 0.8:
                d += rng.choice(greek_cyr).encode()
            elif x < 0.9:
                d += chr(rng.choice(LENGTH_CHANGERS)).encode()
            else:
                d += bytes([rng.randrange(0x80, 0x100)])
        docs.append(bytes(d[:want]))
    return docs
