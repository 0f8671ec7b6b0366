"""strings.ToLower for the device, on the host: the two-level mapping table the kernels read (gft_debug_lower_rune) against
gft_to_lower over every code point, and gft_to_lower_device's count / prefix / write walk through the kernels' own piece
logic (gft_debug_emulate_to_lower, csrc/gft_tolower_piece.hpp) against gft_to_lower document by document -- on the inputs of
tests/test_gpu_tolower.py, so that what the GPU module runs is known to be a test here."""
import ctypes as C
import random

import numpy as np
import pytest

from gofindthem_amd import _lib
from tolower_cases import (GROW_2_3, LENGTH_CHANGERS, SHRINK_2_1, SHRINK_3_1, SHRINK_3_2, edge_batches, pack, py_lower, random_docs,
                           ref_lower, reference)

GFT_E_INVALID = -1


def emulate(docs, lead=0, cap=None, guard=0):
    """gft_debug_emulate_to_lower -> (rc, out bytes [cap + guard], out_off, total)"""
    L = _lib.load()
    blob, off = pack(docs, lead)
    blob = blob[:len(blob) - 64].copy() if len(blob) > 64 else blob        # (the hook asks for no slack)
    out_off = np.full(len(docs) + 1, 0xDEAD, np.uint64)
    total = C.c_uint64(0)
    if cap is None:
        rc = L.gft_debug_emulate_to_lower(blob.ctypes.data, off.ctypes.data, len(docs), None, 0, out_off.ctypes.data, C.byref(total))
        if rc:
            return rc, b"", out_off, total.value
        cap = total.value
    out = np.full(cap + guard + 1, 0xA5, np.uint8)
    rc = L.gft_debug_emulate_to_lower(blob.ctypes.data, off.ctypes.data, len(docs), out.ctypes.data, cap, out_off.ctypes.data, C.byref(total))
    return rc, out[:cap + guard].tobytes(), out_off, total.value


def test_symbols_present():
    L = _lib.load()
    for name in ("gft_to_lower_device", "gft_debug_lower_rune", "gft_debug_emulate_to_lower", "gft_finder_lowered_batches"):
        assert hasattr(L, name) and name in _lib.SYMBOLS


def test_table_lookup_equals_to_lower_for_every_code_point():
    L = _lib.load()
    cps = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]
    low = ref_lower("".join(map(chr, cps)).encode("utf-8")).decode("utf-8")
    assert len(low) == len(cps)
    f = L.gft_debug_lower_rune
    bad = [cp for cp, ch in zip(cps, low) if f(cp) != ord(ch)]
    assert not bad, "first differences: %s" % [hex(c) for c in bad[:8]]
    # the second reference, and the list of length-changers the GPU module places
    changers = {}
    for cp, ch in zip(cps, low):
        assert ch == py_lower(chr(cp)), hex(cp)
        a, b = len(chr(cp).encode()), len(ch.encode())
        if a != b:
            changers.setdefault((a, b), []).append(cp)
    assert changers == {(2, 1): SHRINK_2_1, (3, 1): SHRINK_3_1, (3, 2): sorted(SHRINK_3_2), (2, 3): GROW_2_3}
    assert len(SHRINK_3_2) == 3 + 18 and len(LENGTH_CHANGERS) == 25      # (unicode_lower.inc, Unicode 13: 25 code points in all)


@pytest.mark.parametrize("name", sorted(edge_batches()))
def test_emulation_equals_to_lower_on_the_gpu_modules_edge_inputs(name):
    docs = edge_batches()[name]
    want, want_off = reference(docs)
    for lead in (0, 5):
        rc, out, off, total = emulate(docs, lead)
        assert rc == 0 and total == len(want)
        assert np.array_equal(off, want_off)
        assert out == want, "first difference at byte %d" % next(i for i in range(len(want)) if out[i] != want[i])


def test_no_documents():
    rc, out, off, total = emulate([])
    assert rc == 0 and total == 0 and off.tolist() == [0]


@pytest.fixture(scope="module")
def random_family():
    docs = random_docs()
    return docs, reference(docs)


def test_random_family_is_not_vacuous(random_family):
    """asserted on the reference alone: what keeps the GPU module's random case from passing with an A-Z fold"""
    docs, _ = random_family
    assert len(docs) == 2000 and max(map(len, docs)) <= 300 and min(map(len, docs)) == 0
    changing = invalid = differ = 0
    for d in docs:
        low = ref_lower(d)
        text = d.decode("utf-8", "replace")
        changing += any(ord(ch) in LENGTH_CHANGERS for ch in text)
        try:
            d.decode("utf-8")
        except UnicodeDecodeError:
            invalid += 1
        differ += low != bytes(b + 32 if 65 <= b <= 90 else b for b in d)
    assert changing * 3 >= len(docs), changing
    assert invalid * 3 >= len(docs), invalid
    assert differ * 2 >= len(docs), differ


def test_emulation_equals_to_lower_on_the_random_family(random_family):
    docs, (want, want_off) = random_family
    rc, out, off, total = emulate(docs)
    assert rc == 0 and total == len(want) and np.array_equal(off, want_off) and out == want
    for d in docs[:300]:                     # valid documents: the restatement in Python agrees
        try:
            s = d.decode("utf-8")
        except UnicodeDecodeError:
            continue
        assert ref_lower(d) == py_lower(s).encode("utf-8")


def test_emulation_on_seeded_random_byte_strings():
    rng = random.Random(99)
    docs = [bytes(rng.choice(b"\x00AZaz\x7f\x80\xbf\xc0\xc2\xc3\xdf\xe0\xe2\xed\xef\xf0\xf4\xf5\xff\x9f\xa0\x90\x8f\x89\xb0") for _ in range(rng.randint(0, 200)))
            for _ in range(400)]
    docs += [bytes(rng.randrange(256) for _ in range(rng.choice([1, 17, 1025, 9000])))for _ in range(12)]
    want, want_off = reference(docs)
    rc, out, off, total = emulate(docs, lead=3)
    assert rc == 0 and total == len(want) and np.array_equal(off, want_off) and out == want


def test_cap_below_the_total_writes_nothing_past_cap():
    docs = edge_batches()["length_changers"] + edge_batches()["invalid"] + [b"plain ASCII " * 40]
    want, want_off = reference(docs)
    for cap in (len(want) - 1, len(want) - 17, len(want) // 2, 1):
        rc, out, off, total = emulate(docs, cap=cap, guard=64)
        assert rc == 0 and total == len(want) and np.array_equal(off, want_off)
        assert out[:cap] == want[:cap]
        assert out[cap:] == b"\xa5" * 64, "cap %d: bytes stored past cap" % cap


def test_refusals():
    L = _lib.load()
    blob, off = pack([b"abc", b"DEF"])
    out = np.zeros(64, np.uint8)
    out_off = np.zeros(3, np.uint64)
    total = C.c_uint64()
    call = lambda b, o, n, dst, cap, oo: L.gft_debug_emulate_to_lower(b, o, n, dst, cap, oo, C.byref(total))   # noqa: E731
    assert call(blob.ctypes.data, off.ctypes.data, 2, out.ctypes.data, 64, out_off.ctypes.data) == 0
    assert out[:6].tobytes() == b"abcdef"
    desc = np.array([0, 5, 3], np.uint64)
    assert call(blob.ctypes.data, desc.ctypes.data, 2, out.ctypes.data, 64, out_off.ctypes.data) == GFT_E_INVALID
    # the output inside the input, and the offsets on top of the input's
    assert call(blob.ctypes.data, off.ctypes.data, 2, blob.ctypes.data + 2, 16, out_off.ctypes.data) == GFT_E_INVALID
    assert call(blob.ctypes.data, off.ctypes.data, 2, out.ctypes.data, 64, off.ctypes.data) == GFT_E_INVALID
    assert blob[:6].tobytes() == b"abcDEF" and off.tolist() == [0, 3, 6]
    assert call(blob.ctypes.data, off.ctypes.data, 2, None, 8, out_off.ctypes.data) == GFT_E_INVALID      # cap without a buffer
