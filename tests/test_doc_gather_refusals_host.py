"""What the three document-gather calls (gft_select_docs_device, gft_context_docs_device, gft_route_docs_device) refuse before they
need the device: one table per call of (arguments, status code, the exact gft_last_error text), in the order the refusals are tested
-- shown by calls that commit two faults at once, where the earlier test must win.  The pointers are addresses of host arrays:
nothing refused here is ever read.  On a machine without a device gft_engine_create hands out its handle together with GFT_E_HIP,
and every table ends with the calls that pass the argument tests and meet "no HIP device available"; on a machine with a device
those last rows are left out, since the call would go on to read the host addresses from the device.  (The refusals behind the
device check are in test_refusals_leave_the_handle_usable of the three GPU test files; "single-device handles only" needs a handle
over several devices and is there too.)"""
import ctypes as C

import numpy as np
import pytest

from gofindthem_amd import _lib

INVALID, HIP, UNSUPPORTED = _lib.GFT_E_INVALID, _lib.GFT_E_HIP, _lib.GFT_E_UNSUPPORTED
NO_DEVICE = "no HIP device available"
_mem = np.zeros(4096, dtype=np.uint64)
PTR = _mem.ctypes.data                       # a non-null address for every array argument


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


def select_args(text=PTR, doc_off=PTR, n_docs=3, bitmap=PTR, n_cols=40, want=PTR, mode=0, also=None, out=PTR, cap_bytes=8, out_off=PTR, doc_idx=PTR,
                cap_docs=2):
    return (text, doc_off, n_docs, bitmap, n_cols, want, mode, also, out, cap_bytes, out_off, doc_idx, cap_docs)


def context_args(text=PTR, doc_off=PTR, n_docs=3, bitmap=PTR, n_cols=40, want=PTR, mode=0, also=None, before=1, after=1, fence=None, out=PTR,
                 cap_bytes=8, out_off=PTR, doc_idx=PTR, kind=PTR, cap_docs=2, group_off=PTR, cap_groups=2):
    return (text, doc_off, n_docs, bitmap, n_cols, want, mode, also, before, after, fence, out, cap_bytes, out_off, doc_idx, kind, cap_docs, group_off,
            cap_groups)


def route_args(text=PTR, doc_off=PTR, n_docs=3, bitmap=PTR, n_cols=40, masks=PTR, n_buckets=2, mode=1, flags=0, also=None, out=PTR, cap_bytes=8,
               out_off=PTR, doc_idx=PTR, cap_docs=2, bucket_doc=None, bucket_byte=None):
    return (text, doc_off, n_docs, bitmap, n_cols, masks, n_buckets, mode, flags, also, out, cap_bytes, out_off, doc_idx, cap_docs, bucket_doc,
            bucket_byte)


NULL = "null argument"
S, X, R = "gft_select_docs_device: ", "gft_context_docs_device: ", "gft_route_docs_device: "
CAP_BYTES = "cap_bytes but no output buffer"

# (arguments, code, text); the rows with NO_DEVICE pass every argument test
SELECT = [
    (select_args(doc_off=None), INVALID, NULL),
    (select_args(text=None), INVALID, NULL),
    (select_args(bitmap=None), INVALID, NULL),
    (select_args(text=None, out=None), INVALID, NULL),                                   # null argument before cap_bytes
    (select_args(out=None), INVALID, S + CAP_BYTES),
    (select_args(out=None, out_off=None), INVALID, S + CAP_BYTES),                       # cap_bytes before cap_docs
    (select_args(out_off=None), INVALID, S + "cap_docs but no offset or index array"),
    (select_args(doc_idx=None), INVALID, S + "cap_docs but no offset or index array"),
    (select_args(doc_idx=None, mode=3), INVALID, S + "cap_docs but no offset or index array"),   # cap_docs before the device and the mode
    (select_args(), HIP, NO_DEVICE),
    (select_args(mode=3), HIP, NO_DEVICE),                                               # the device before the mode ...
    (select_args(cap_docs=1 << 62, n_docs=1 << 62), HIP, NO_DEVICE),                     # ... and before the sizes
    (select_args(bitmap=None, n_cols=0, want=None), HIP, NO_DEVICE),                     # no columns: no rows needed
    (select_args(text=None, doc_off=None, bitmap=None, n_docs=0), HIP, NO_DEVICE),       # no documents: no arrays needed
    (select_args(out=None, cap_bytes=0, out_off=None, doc_idx=None, cap_docs=0), HIP, NO_DEVICE),
]
CONTEXT = [
    (context_args(doc_off=None), INVALID, NULL),
    (context_args(text=None), INVALID, NULL),
    (context_args(bitmap=None), INVALID, NULL),
    (context_args(bitmap=None, out=None), INVALID, NULL),
    (context_args(out=None), INVALID, X + CAP_BYTES),
    (context_args(out=None, kind=None), INVALID, X + CAP_BYTES),
    (context_args(out_off=None), INVALID, X + "cap_docs but no offset, index or kind array"),
    (context_args(doc_idx=None), INVALID, X + "cap_docs but no offset, index or kind array"),
    (context_args(kind=None), INVALID, X + "cap_docs but no offset, index or kind array"),
    (context_args(kind=None, group_off=None), INVALID, X + "cap_docs but no offset, index or kind array"),    # cap_docs before cap_groups
    (context_args(group_off=None), INVALID, X + "cap_groups but no group array"),
    (context_args(group_off=None, mode=7), INVALID, X + "cap_groups but no group array"),
    (context_args(), HIP, NO_DEVICE),
    (context_args(mode=7), HIP, NO_DEVICE),
    (context_args(cap_groups=1 << 62), HIP, NO_DEVICE),
    (context_args(text=None, doc_off=None, bitmap=None, n_docs=0), HIP, NO_DEVICE),
    (context_args(out=None, cap_bytes=0, out_off=None, doc_idx=None, kind=None, cap_docs=0, group_off=None, cap_groups=0), HIP, NO_DEVICE),
]
BUCKETS = "more than 64 buckets (GFT_ROUTE_MAX_BUCKETS), the rest bucket included"
ROUTE = [
    (route_args(flags=2), INVALID, R + "unknown flag bits"),
    (route_args(flags=3, n_buckets=65), INVALID, R + "unknown flag bits"),               # the flags before the buckets
    (route_args(n_buckets=65), UNSUPPORTED, R + BUCKETS),
    (route_args(n_buckets=64, flags=1), UNSUPPORTED, R + BUCKETS),
    (route_args(n_buckets=65, text=None), UNSUPPORTED, R + BUCKETS),                     # the buckets before null argument
    (route_args(doc_off=None), INVALID, NULL),
    (route_args(text=None), INVALID, NULL),
    (route_args(bitmap=None), INVALID, NULL),
    (route_args(bitmap=None, masks=None), INVALID, NULL),                                # null argument before the masks
    (route_args(masks=None), INVALID, R + "buckets but no masks"),
    (route_args(masks=None, out=None), INVALID, R + "buckets but no masks"),             # the masks before cap_bytes
    (route_args(out=None), INVALID, R + CAP_BYTES),
    (route_args(out=None, doc_idx=None), INVALID, R + CAP_BYTES),
    (route_args(out_off=None), INVALID, R + "cap_docs but no offset or index array"),
    (route_args(doc_idx=None), INVALID, R + "cap_docs but no offset or index array"),
    (route_args(doc_idx=None, mode=2, also=PTR), INVALID, R + "cap_docs but no offset or index array"),
    (route_args(), HIP, NO_DEVICE),
    (route_args(n_buckets=64), HIP, NO_DEVICE),
    (route_args(n_buckets=63, flags=1), HIP, NO_DEVICE),
    (route_args(mode=2), HIP, NO_DEVICE),                                                # the device before the mode ...
    (route_args(also=PTR), HIP, NO_DEVICE),                                              # ... before d_also without the rest flag ...
    (route_args(cap_docs=1 << 62), HIP, NO_DEVICE),                                      # ... and before the sizes
    (route_args(masks=None, n_buckets=0), HIP, NO_DEVICE),
    (route_args(masks=None, bitmap=None, n_cols=0), HIP, NO_DEVICE),
    (route_args(text=None, doc_off=None, bitmap=None, n_docs=0), HIP, NO_DEVICE),
]


def run(handle, table, call):
    L, h, no_device = handle
    ran = 0
    for i, (args, code, text) in enumerate(table):
        if code == HIP and not no_device:
            continue
        assert call(L, h, args) == code, (i, args)
        assert L.gft_last_error(h).decode() == text, (i, args)
        ran += 1
    assert ran >= sum(1 for _, code, _ in table if code != HIP) > 8


def test_select_refusals_in_order(handle):
    m, t = C.c_uint64(9), C.c_uint64(9)

    def call(L, h, args):
        m.value = t.value = 9
        rc = L.gft_select_docs_device(h, *args, C.byref(m), C.byref(t))
        assert (m.value, t.value) == (0, 0)                              # (the counts are cleared in front of every refusal)
        return rc
    run(handle, SELECT, call)
    assert _lib.load().gft_select_docs_device(None, *select_args(), C.byref(m), C.byref(t)) == INVALID


def test_context_refusals_in_order(handle):
    counts = [C.c_uint64(9) for _ in range(4)]

    def call(L, h, args):
        for c in counts:
            c.value = 9
        rc = L.gft_context_docs_device(h, *args, *[C.byref(c) for c in counts])
        assert [c.value for c in counts] == [0, 0, 0, 0]
        return rc
    run(handle, CONTEXT, call)
    assert _lib.load().gft_context_docs_device(None, *context_args(), *[C.byref(c) for c in counts]) == INVALID


def test_route_refusals_in_order(handle):
    run(handle, ROUTE, lambda L, h, args: L.gft_route_docs_device(h, *args))
    assert _lib.load().gft_route_docs_device(None, *route_args()) == INVALID
    # behind the flag and bucket tests the B + 1 borders are cleared, whatever is refused then
    L, h, _ = handle
    bd, bb = np.full(4, 7, dtype=np.uint64), np.full(4, 7, dtype=np.uint64)
    assert L.gft_route_docs_device(h, *route_args(text=None, bucket_doc=bd.ctypes.data, bucket_byte=bb.ctypes.data)) == INVALID
    assert bd.tolist() == [0, 0, 0, 7] and bb.tolist() == [0, 0, 0, 7]
    bd[:] = 7
    assert L.gft_route_docs_device(h, *route_args(flags=2, bucket_doc=bd.ctypes.data, bucket_byte=bb.ctypes.data)) == INVALID
    assert bd.tolist() == [7, 7, 7, 7]                                   # (refused in front of the clearing: untouched)
