"""The table set on the host (no GPU): csrc/table_set.cpp through gft_debug_tables.

The hook compiles a dictionary with the function gft_build calls -- or reads a blob with the function gft_import_tables
calls --, chooses the scan kernel the way both do for a device with a given LDS size, and writes the set with the function
gft_export_tables calls.  So the blob format, its validation and the decision table of DESIGN.md 4.7 are checked here; the
GPU suite keeps the checks that the installed tables scan like the oracle (tests/test_gpu_parity.py).
"""
import random
import struct

import pytest

from gofindthem_amd import _lib
from gofindthem_amd.workload import Workload
from helpers import Refused, tables


def lower_terms():
    return Workload(2000).terms()


def no_short_terms():
    """few byte classes, every term at least 4 bytes long: scan2's tables are supported and their short3 is EMPTY"""
    rng = random.Random(11)
    return sorted({bytes(rng.choice(b"abcde") for _ in range(rng.randint(4, 12))) for _ in range(300)})


def mixed_terms():
    return sorted({t.decode("utf-8").lower().encode("utf-8") for t in Workload(3000, alphabet="mixed").terms()})


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("GFT_SCAN_KERNEL", "GFT_SCAN5_LARGE", "GFT_SCAN5_GROUPS", "GFT_SCAN5_BLOOM_KB", "GFT_SCAN5_FIFO"):
        monkeypatch.delenv(name, raising=False)


def skip_to_scan2(b):
    """offset of Scan2Tables::supported in a blob (gft_export_tables' layout)"""
    at = 20
    n_terms = struct.unpack_from("<Q", b, at)[0]; at += 8
    for _ in range(n_terms):
        at += 8 + struct.unpack_from("<Q", b, at)[0]
    at += 4 + 256 + 4 + 4                          # n_classes, byte_class, n_states, max_term_len
    for width in (4, 4, 4, 4, 4, 4, 4, 1):         # delta, out_term, out_link, term_len, depth, fail, child_begin, in_class
        at += 8 + width * struct.unpack_from("<Q", b, at)[0]
    return at


def resealed(b):
    h = 1469598103934665603
    for c in b[:-8]:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return b[:-8] + struct.pack("<Q", h)


@pytest.mark.parametrize("make", [lower_terms, no_short_terms, mixed_terms])
def test_written_blob_reads_back_to_the_same_bytes(make):
    """compile -> write -> read -> write: identical bytes, and the same kernel chosen from the set that was read.  The
    dictionary without a term shorter than 4 bytes has an empty short3 over kp >= 3 classes: a set whose short3 was
    replaced by the 16-byte upload placeholder before it was written is refused by the reader ("scan2 short3 size")"""
    terms = make()
    kernel, blob = tables(terms)
    kernel2, blob2 = tables(blob=blob)
    assert blob2 == blob and kernel2 == kernel
    if make is no_short_terms:
        at = skip_to_scan2(blob)
        supported, kp = struct.unpack_from("<II", blob, at)
        at += 24
        at += 8 + 4 * struct.unpack_from("<Q", blob, at)[0]                # filter
        assert supported == 1 and kp ** 3 > 16 and struct.unpack_from("<Q", blob, at)[0] == 0, "short3 is not empty"
        # the blob that the placeholder edit used to produce is one the reader refuses
        with pytest.raises(Refused, match="scan2 short3 size"):
            tables(blob=resealed(blob[:at] + struct.pack("<Q", 16) + bytes(16) + blob[at + 8:]))


def test_damaged_and_foreign_blobs_are_refused():
    _, blob = tables(lower_terms())
    assert len(blob) > 100_000
    for bad in (blob[:-1], blob[:1000], b"GFTT" + blob[4:200], blob[:500] + bytes([blob[500] ^ 1]) + blob[501:], b""):
        with pytest.raises(Refused):
            tables(blob=bad)
    # a blob that is internally consistent as far as the checksum goes, but whose tables point outside themselves
    # (stale or crafted): every index-bearing table is validated
    n_bad = 0
    for frac in (0.2, 0.35, 0.5, 0.65, 0.8, 0.9, 0.97):
        at = int(len(blob) * frac) & ~3
        try:
            tables(blob=resealed(blob[:at] + b"\xff\xff\xff\x7f" + blob[at + 4:]))
        except Refused:
            n_bad += 1
    assert n_bad >= 2
    # relations BETWEEN the tables: the suffix-window set's class count and class map must be the automaton's, a bucket key
    # must be four classes, and a key must sit in its own pair of the bucket table
    at = skip_to_scan2(blob) + 4
    kp = struct.unpack_from("<I", blob, at)[0]
    assert 2 <= kp <= 64 and struct.unpack_from("<I", blob, at - 4)[0] == 1, "blob layout changed: adapt skip_to_scan2"
    for forged_kp in (kp - 1, kp + 1, 2):
        with pytest.raises(Refused, match="inconsistent"):
            tables(blob=resealed(blob[:at] + struct.pack("<I", forged_kp) + blob[at + 4:]))


def test_scan_kernel_decision_table(monkeypatch):
    """DESIGN.md 4.7, the rows that a library without the extra kernels reaches, at gfx950's LDS size"""
    extra = b"extra_kernels=1" in _lib.load().gft_build_info()
    lower, mixed = lower_terms(), mixed_terms()
    assert len({b for t in mixed for b in t}) >= 48 and min(len(t) for t in mixed) <= 3
    # row 4: scan5 by default wherever it applies -- also over more than 32 byte classes (the large-alphabet route)
    assert tables(lower)[0] == "scan5" and tables(lower, forced="scan5")[0] == "scan5" and tables(lower, forced="")[0] == "scan5"
    assert tables(mixed)[0] == "scan5" and tables(no_short_terms())[0] == "scan5"
    # row 2: a forced scan3 is obeyed; it is also what is left when scan5 does not apply
    assert tables(lower, forced="scan3")[0] == "scan3" and tables(mixed, forced="scan3")[0] == "scan3"
    monkeypatch.setenv("GFT_SCAN5_LARGE", "0")
    assert tables(mixed)[0] == "scan3" and tables(mixed, forced="scan5")[0] == "scan3"
    assert tables(lower)[0] == "scan5"                                     # (at most 32 byte classes: not its business)
    monkeypatch.delenv("GFT_SCAN5_LARGE")
    # last row: a forced dfa is obeyed
    assert tables(lower, forced="dfa")[0] == "dfa" and tables(mixed, forced="dfa")[0] == "dfa"
    # a value that names no kernel leaves only the rows that do not ask for one: scan5 needs f unset or scan5, scan3 is
    # chosen when neither scan5 nor scan2 applies -- scan2 never does in a product library
    assert tables(lower, forced="nonsense")[0] == ("scan2" if extra else "scan3")
    # forced=None: the environment's own value
    monkeypatch.setenv("GFT_SCAN_KERNEL", "dfa")
    assert tables(lower, forced=None)[0] == "dfa"
    monkeypatch.delenv("GFT_SCAN_KERNEL")
    # row 1: the cross-check kernels in a library that does not carry them
    for name in ("scan2", "scan4"):
        if extra:
            assert tables(lower, forced=name)[0] == name and tables(mixed, forced=name)[0] == "dfa"
        else:
            with pytest.raises(Refused, match="built without the cross-check kernels") as ei:
                tables(lower, forced=name)
            assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    # the limits that come before the choice
    with pytest.raises(Refused, match="keyword longer than 7424 bytes") as ei:
        tables([b"x" * 7425, b"abc"])
    assert ei.value.code == _lib.GFT_E_UNSUPPORTED
    with pytest.raises(Refused, match="LDS too small"):
        tables(lower, lds_max=64 * 1024)
