"""What the four batch calls over a term list (gft_batch_term_stats_device, gft_batch_top_docs_device and their whole-word twins)
refuse in their shared front end, and what the two calls that take such a list (gft_term_stats_device, gft_score_docs_device)
refuse before they need the device: one table per call of (arguments, status code, the exact gft_last_error text), in the order the
refusals are tested -- null arguments, flag bits (the caller's, then scan_flags), k and the top arrays, the device, the sizes --
shown by calls that commit two faults at once, where the earlier test must win.  The pointers are addresses of host arrays: nothing
refused here is ever read.  On a machine without a device gft_engine_create hands out its handle together with GFT_E_HIP, and
every table ends with the calls that pass the argument tests and meet "no HIP device available"; on a machine with a device those
rows are left out, since the call would go on to read the host addresses from the device, and the rows of SIZES run in their place:
an n_docs beyond the source's limit, refused in front of every allocation and every read.

The rows were recorded on the commit before the front end (batch_term_list) and again behind it.  The rows marked "was:" are the
ones that answer differently, with what that commit answered; every other row answered the same.  ("single-device handles only"
needs a handle over several devices and is in the GPU tests.)"""
import ctypes as C

import numpy as np
import pytest

from gofindthem_amd import _lib

INVALID, HIP = _lib.GFT_E_INVALID, _lib.GFT_E_HIP
NO_DEVICE = "no HIP device available"
NULL = "null argument"
_mem = np.zeros(4096, dtype=np.uint64)
PTR = _mem.ctypes.data                       # a non-null address for every array argument
FOLD = _lib.GFT_FOLD_ASCII


@pytest.fixture(scope="module")
def handle():
    L = _lib.load()
    h = C.c_void_p()
    rc = L.gft_engine_create(C.byref(h), -1)
    assert h and rc in (0, HIP)
    if rc == HIP:
        assert L.gft_last_error(h).decode().startswith(NO_DEVICE + ": ")
    yield L, h, rc == HIP
    L.gft_engine_destroy(h)


def stats_args(text=PTR, doc_off=PTR, n_docs=3, scan_flags=FOLD, bitmap=None, want=None, flags=0, doc_base=0, occ=PTR, docs=PTR, first=PTR):
    return (text, doc_off, n_docs, scan_flags, bitmap, want, flags, doc_base, occ, docs, first)


def top_args(text=PTR, doc_off=PTR, n_docs=3, scan_flags=FOLD, bitmap=None, want=None, weights=None, flags=0, k=2, doc_base=0, score=PTR,
             top_idx=PTR, top_score=PTR):
    return (text, doc_off, n_docs, scan_flags, bitmap, want, weights, flags, k, doc_base, score, top_idx, top_score)


def list_stats_args(off=PTR, term=PTR, n_docs=3, n_terms=5, flags=0, doc_base=0, occ=PTR, docs=PTR, first=PTR):
    return (off, term, n_docs, n_terms, flags, doc_base, occ, docs, first)


def list_score_args(off=PTR, term=PTR, n_docs=3, n_terms=5, weights=None, flags=0, score=PTR):
    return (off, term, n_docs, n_terms, weights, flags, score)


# What the commit before answered with a bitmap and no device, in the rows' comments:
#   "was: alloc"  the plain calls allocated in front of every test of the handle: GFT_E_HIP "stats alloc: no ROCm-capable device is
#                 detected" ("rank alloc: ..." from the top call); the whole-word twins tested the device first and answered as now
#   "was: size"   the plain calls the same allocation failure; the twins GFT_E_INVALID "gft_hit_spans_words_device: a size beyond the
#                 address space", the name of a call the caller never made
def batch_stats_table(who):
    """the rows of one statistics call"""
    W = who + ": "
    return [
        (stats_args(text=None), INVALID, NULL),
        (stats_args(doc_off=None, bitmap=PTR), INVALID, NULL),                           # was: alloc
        (stats_args(text=None, flags=2), INVALID, NULL),                                 # null argument before the flags (was: unknown flag bits)
        (stats_args(doc_off=None, scan_flags=4), INVALID, NULL),                         # ... and before scan_flags (was: scan_flags is ...)
        (stats_args(flags=2), INVALID, W + "unknown flag bits"),
        (stats_args(flags=2, scan_flags=4), INVALID, W + "unknown flag bits"),           # the caller's flags before scan_flags
        (stats_args(flags=6, bitmap=PTR, n_docs=1 << 60), INVALID, W + "unknown flag bits"),
        (stats_args(scan_flags=4), INVALID, W + "scan_flags is GFT_FOLD_ASCII or 0"),
        (stats_args(scan_flags=3, bitmap=PTR), INVALID, W + "scan_flags is GFT_FOLD_ASCII or 0"),
        (stats_args(scan_flags=2, n_docs=1 << 60), INVALID, W + "scan_flags is GFT_FOLD_ASCII or 0"),   # the flags before the sizes
        (stats_args(), HIP, NO_DEVICE),
        (stats_args(flags=1, scan_flags=0, want=PTR), HIP, NO_DEVICE),
        (stats_args(bitmap=PTR), HIP, NO_DEVICE),                                        # was: alloc
        (stats_args(bitmap=PTR, want=PTR, occ=None, docs=None, first=None), HIP, NO_DEVICE),   # was: alloc
        (stats_args(n_docs=1 << 60), HIP, NO_DEVICE),                                    # the device before the sizes
        (stats_args(bitmap=PTR, n_docs=1 << 60), HIP, NO_DEVICE),                        # was: size
        (stats_args(text=None, doc_off=None, n_docs=0), HIP, NO_DEVICE),                 # no documents: no arrays needed
        (stats_args(text=None, doc_off=None, n_docs=0, bitmap=PTR), HIP, NO_DEVICE),     # was: alloc
    ]


def batch_top_table(who):
    """the rows of one top call"""
    W = who + ": "
    return [
        (top_args(text=None), INVALID, NULL),
        (top_args(doc_off=None, bitmap=PTR), INVALID, NULL),                             # was: alloc
        (top_args(text=None, flags=2), INVALID, NULL),                                   # null argument before the flags (was: unknown flag bits)
        (top_args(doc_off=None, k=5000), INVALID, NULL),                                 # ... and before k
        (top_args(flags=2), INVALID, W + "unknown flag bits"),
        (top_args(flags=2, scan_flags=4), INVALID, W + "unknown flag bits"),             # the caller's flags before scan_flags
        (top_args(flags=2, k=5000), INVALID, W + "unknown flag bits"),                   # ... and before k
        (top_args(scan_flags=4), INVALID, W + "scan_flags is GFT_FOLD_ASCII or 0"),
        (top_args(scan_flags=2, k=5000, bitmap=PTR), INVALID, W + "scan_flags is GFT_FOLD_ASCII or 0"),   # scan_flags before k
        (top_args(k=4097), INVALID, W + "k above 4096"),                                 # was: no HIP device available
        (top_args(k=4097, bitmap=PTR), INVALID, W + "k above 4096"),                     # was: alloc
        (top_args(k=5000, top_idx=None), INVALID, W + "k above 4096"),                   # k before the top arrays (was: no HIP device available)
        (top_args(k=1 << 31, n_docs=1 << 60), INVALID, W + "k above 4096"),              # k before the sizes (was: no HIP device available)
        (top_args(top_idx=None), INVALID, NULL),                                         # was: no HIP device available
        (top_args(top_score=None, bitmap=PTR), INVALID, NULL),                           # was: alloc
        (top_args(k=4096, top_score=None, n_docs=1 << 60, bitmap=PTR), INVALID, NULL),   # the top arrays before the sizes (was: size)
        (top_args(), HIP, NO_DEVICE),
        (top_args(k=4096, flags=1, scan_flags=0, want=PTR, weights=PTR), HIP, NO_DEVICE),
        (top_args(k=0, top_idx=None, top_score=None, score=None), HIP, NO_DEVICE),       # no list asked for: no top arrays needed
        (top_args(bitmap=PTR), HIP, NO_DEVICE),                                          # was: alloc
        (top_args(n_docs=1 << 60), HIP, NO_DEVICE),                                      # the device before the sizes
        (top_args(bitmap=PTR, n_docs=1 << 60), HIP, NO_DEVICE),                          # was: size
        (top_args(text=None, doc_off=None, n_docs=0), HIP, NO_DEVICE),                   # no documents: no arrays needed
        (top_args(text=None, doc_off=None, n_docs=0, bitmap=PTR), HIP, NO_DEVICE),       # was: alloc
    ]


SIZE = "a size beyond the address space"
PLAIN_STATS, WORDS_STATS = batch_stats_table("gft_batch_term_stats_device"), batch_stats_table("gft_batch_term_stats_words_device")
PLAIN_TOP, WORDS_TOP = batch_top_table("gft_batch_top_docs_device"), batch_top_table("gft_batch_top_docs_words_device")

# with a device: an n_docs beyond the source's limit (plain: 2^60 entries of 16 bytes leave the address space; whole words: 2^38,
# the filter's) names the entry point that was called, with and without a bitmap.  (was, with a bitmap: an allocation of
# (n_docs + 1) * 8 bytes for the plain calls, "gft_hit_spans_words_device: ..." for the twins)
SIZES = {
    "gft_batch_term_stats_device": [stats_args(n_docs=1 << 60), stats_args(n_docs=1 << 60, bitmap=PTR)],
    "gft_batch_term_stats_words_device": [stats_args(n_docs=(1 << 38) + 1), stats_args(n_docs=1 << 60, bitmap=PTR)],
    "gft_batch_top_docs_device": [top_args(n_docs=1 << 60), top_args(n_docs=1 << 60, bitmap=PTR, score=None)],
    "gft_batch_top_docs_words_device": [top_args(n_docs=(1 << 38) + 1), top_args(n_docs=1 << 60, bitmap=PTR)],
}

T, S = "gft_term_stats_device: ", "gft_score_docs_device: "
LIST_STATS = [
    (list_stats_args(flags=2), INVALID, T + "unknown flag bits"),
    (list_stats_args(flags=2, off=None), INVALID, T + "unknown flag bits"),              # the flags before null argument
    (list_stats_args(off=None), INVALID, NULL),
    (list_stats_args(off=None, n_docs=1 << 60), INVALID, NULL),                          # null argument before the device and the sizes
    (list_stats_args(), HIP, NO_DEVICE),
    (list_stats_args(flags=1, occ=None, docs=None, first=None), HIP, NO_DEVICE),
    (list_stats_args(n_docs=1 << 60), HIP, NO_DEVICE),                                   # the device before the sizes
    (list_stats_args(term=None, n_terms=0), HIP, NO_DEVICE),                             # (the list's ends are read on the device)
    (list_stats_args(off=None, term=None, n_docs=0), HIP, NO_DEVICE),                    # no documents: no arrays needed
]
LIST_SCORE = [
    (list_score_args(flags=2), INVALID, S + "unknown flag bits"),
    (list_score_args(flags=2, off=None), INVALID, S + "unknown flag bits"),              # the flags before null argument
    (list_score_args(off=None), INVALID, NULL),
    (list_score_args(score=None), INVALID, NULL),
    (list_score_args(score=None, n_docs=1 << 60), INVALID, NULL),                        # null argument before the device and the sizes
    (list_score_args(), HIP, NO_DEVICE),
    (list_score_args(flags=1, weights=PTR), HIP, NO_DEVICE),
    (list_score_args(n_docs=1 << 60), HIP, NO_DEVICE),                                   # the device before the sizes
    (list_score_args(term=None, n_terms=0), HIP, NO_DEVICE),                             # (the list's ends are read on the device)
    (list_score_args(off=None, term=None, score=None, n_docs=0), HIP, NO_DEVICE),        # no documents: no arrays needed
]


def run(handle, table, call, least=2):
    L, h, no_device = handle
    ran = 0
    for i, (args, code, text) in enumerate(table):
        if code == HIP and not no_device:
            continue
        assert call(L, h, args) == code, (i, args)
        assert L.gft_last_error(h).decode() == text, (i, args)
        ran += 1
    assert ran >= sum(1 for _, code, _ in table if code != HIP) > least


def stats_call(name):
    na = C.c_int(7)

    def call(L, h, args):
        na.value = 7
        rc = getattr(L, name)(h, *args, C.byref(na))
        assert na.value == 0                                             # (cleared in front of every refusal)
        return rc
    return call


def top_call(name):
    na, n_top = C.c_int(7), C.c_uint64(7)

    def call(L, h, args):
        na.value = n_top.value = 7
        rc = getattr(L, name)(h, *args, C.byref(n_top), C.byref(na))
        assert (na.value, n_top.value) == (0, 0)
        return rc
    return call


def sizes(handle, name, call):
    L, h, no_device = handle
    if no_device:
        return
    for args in SIZES[name]:
        assert call(L, h, args) == INVALID, args
        assert L.gft_last_error(h).decode() == name + ": " + SIZE, args


@pytest.mark.parametrize("name,table", [("gft_batch_term_stats_device", PLAIN_STATS), ("gft_batch_term_stats_words_device", WORDS_STATS)])
def test_batch_stats_refusals_in_order(handle, name, table):
    run(handle, table, stats_call(name), 8)
    sizes(handle, name, stats_call(name))
    assert getattr(_lib.load(), name)(None, *stats_args(), None) == INVALID
    # nonascii may be NULL in a refusal too
    L, h, _ = handle
    assert getattr(L, name)(h, *stats_args(flags=2), None) == INVALID


@pytest.mark.parametrize("name,table", [("gft_batch_top_docs_device", PLAIN_TOP), ("gft_batch_top_docs_words_device", WORDS_TOP)])
def test_batch_top_refusals_in_order(handle, name, table):
    run(handle, table, top_call(name), 8)
    sizes(handle, name, top_call(name))
    assert getattr(_lib.load(), name)(None, *top_args(), None, None) == INVALID
    L, h, _ = handle
    assert getattr(L, name)(h, *top_args(k=4097), None, None) == INVALID


def test_list_head_refusals_in_order(handle):
    run(handle, LIST_STATS, lambda L, h, args: L.gft_term_stats_device(h, *args))
    mx = C.c_uint64(0)
    run(handle, LIST_SCORE, lambda L, h, args: L.gft_score_docs_device(h, *args, C.byref(mx)))
    assert _lib.load().gft_term_stats_device(None, *list_stats_args()) == INVALID
    assert _lib.load().gft_score_docs_device(None, *list_score_args(), None) == INVALID
