"""GpuEngine: the batch-capable SubstringEngine (finder/substringEngine.go:11-18) over libgft.so."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GftExtra, GftMatches, GftSparse


class GftError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gft error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


def pack(strs):
    bs = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strs]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy()
    return blob, off


SPLIT_AFTER_NL, SPLIT_JSON_LINES = 0, 1      # gft_split_mode


def split_lines_tensor(call, buf, length, mode):
    """what Engine.split_lines_device and the finders' line calls share: `call(d_blob, len, mode, d_doc_off, cap, byref(n))` is
    gft_split_lines_device on some handle and raises on an error.  Two calls: count only, then into a tensor of n + 1 entries"""
    import torch
    length = int(length)
    if not buf.is_cuda or buf.dtype != torch.uint8 or not buf.is_contiguous() or length < 0 or buf.numel() < length + 64:
        raise ValueError("split_lines_device takes a contiguous torch.uint8 device tensor of at least length + 64 bytes")
    torch.cuda.current_stream(buf.device).synchronize()
    n = C.c_uint64(0)
    call(buf.data_ptr(), length, mode, None, 0, C.byref(n))
    off = torch.empty(int(n.value) + 1, dtype=torch.int64, device=buf.device)
    torch.cuda.current_stream(buf.device).synchronize()
    call(buf.data_ptr(), length, mode, off.data_ptr(), off.numel(), C.byref(n))
    return off


def split_lines_host(data, mode, cap=None, guard=0):
    """gft_debug_split_lines over a bytes object -> (n, doc_off uint64 [cap + guard]); no device needed.  cap=None: count first,
    then n + 1 entries; the guard entries behind cap hold 0xA5.. and must come back untouched"""
    L = _lib.load()
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = C.c_uint64(0)

    def call(off, cap):
        rc = L.gft_debug_split_lines(a.ctypes.data if a.size else None, a.size, mode, off.ctypes.data if off is not None else None, cap, C.byref(n))
        if rc != 0:
            raise GftError(rc, "gft_debug_split_lines")
    if cap is None:
        call(None, 0)
        cap = int(n.value) + 1
    off = np.full(cap + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    call(off, cap)
    return int(n.value), off


def split_shape():
    """(tile bytes, tiles per trip of the carry pass) of the split kernels (gft_debug_split_shape)"""
    t, k = C.c_uint32(0), C.c_uint32(0)
    _lib.load().gft_debug_split_shape(C.byref(t), C.byref(k))
    return int(t.value), int(k.value)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


SELECT_MODES = {"any": 0, "all": 1, "none": 2}      # gft_select_mode


def _select_mode(mode):
    return SELECT_MODES[mode] if isinstance(mode, str) else int(mode)


def _want_words(want, n_cols):
    """the host mask of a select call: None, or ceil(n_cols / 32) uint32 words"""
    if want is None:
        return None
    w = np.ascontiguousarray(want, dtype=np.uint32).reshape(-1)
    if w.size != (n_cols + 31) // 32:
        raise ValueError("want must have ceil(n_cols / 32) words")
    return w if w.size else np.zeros(1, dtype=np.uint32)


def _docs_tensor_args(who, text, doc_off, bitmap, n_cols, also, *fence):
    """the checks the *_docs_tensor functions make on their device tensors (fence: only for the call that has one) -> (n_docs, the
    five arguments every such C call begins with, also's address or None)"""
    n_docs = int(doc_off.numel()) - 1
    W = (n_cols + 31) // 32
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off")) + (((bitmap, 4, "bitmap"),) if W and n_docs > 0 else ()) + \
            (((also, 1, "also"),) if also is not None else ()) + (((fence[0], 1, "fence"),) if fence and fence[0] is not None else ()):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("%s: %s must be a contiguous device tensor of %d-byte integers" % (who, what, size))
    if n_docs < 0 or (W and n_docs > 0 and bitmap.numel() != n_docs * W) or (also is not None and also.numel() != n_docs) or \
            (fence and fence[0] is not None and fence[0].numel() != n_docs):
        raise ValueError("%s: doc_off, bitmap%s do not describe the same batch" % (who, ", also and fence" if fence else " and also"))
    return n_docs, (text.data_ptr(), doc_off.data_ptr(), n_docs, bitmap.data_ptr() if W and n_docs > 0 else None, n_cols), \
        also.data_ptr() if also is not None else None


def _docs_out_tensors(text, nm, nb):
    import torch                                                           # (the blob, out_off and doc_idx of exactly nm documents, nb bytes)
    buf = torch.zeros(nb + 64, dtype=torch.uint8, device=text.device)      # (64 bytes of slack: the result is a blob for the next call)
    return buf, torch.empty(nm + 1, dtype=torch.int64, device=text.device), torch.empty(nm, dtype=torch.int64, device=text.device)


def _docs_host_args(blob, doc_off, rows, n_cols, also):
    """the arrays of a *_docs_host call as the library reads them -> (the arrays, to be kept alive; n_docs; the five arguments every
    such C call begins with; also's address or None)"""
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
    off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    n_docs = off.size - 1
    bm = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1) if (n_cols + 31) // 32 and n_docs > 0 else None
    al = np.ascontiguousarray(also, dtype=np.uint8) if also is not None else None
    return (a, off, bm, al), n_docs, (a.ctypes.data if a.size else None, off.ctypes.data, n_docs, _p(bm), n_cols), _p(al)


def _docs_host_outputs(cap_bytes, cap_docs, guard, out_shift):
    """out (out_shift bytes into its allocation's 16-byte grid), out_off and doc_idx, filled with 0xA5 up to and including the guard"""
    raw = np.full(cap_bytes + guard + 32, 0xA5, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16 + out_shift
    return raw[at:at + cap_bytes + guard], np.full(cap_docs + 1 + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), \
        np.full(cap_docs + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)


def select_docs_tensor(call, text, doc_off, bitmap, n_cols, want, mode, also):
    """what Engine.select_docs_device and the finders' select calls share: `call(d_text, d_doc_off, n_docs, d_bitmap, n_cols, want,
    mode, d_also, d_out, cap_bytes, d_out_off, d_doc_idx, cap_docs, byref(m), byref(total))` is gft_select_docs_device on some
    handle and raises on an error.  Two calls: count only, then into tensors of exactly the sizes counted"""
    import torch
    n_docs, head, d_also = _docs_tensor_args("select_docs_device", text, doc_off, bitmap, n_cols, also)
    w = _want_words(want, n_cols)
    args = head + (_p(w), _select_mode(mode), d_also)
    m, total = C.c_uint64(0), C.c_uint64(0)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, None, 0, None, None, 0, C.byref(m), C.byref(total))
    nm, nb = int(m.value), int(total.value)
    buf, out_off, doc_idx = _docs_out_tensors(text, nm, nb)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, buf.data_ptr(), nb, out_off.data_ptr(), doc_idx.data_ptr() if nm else None, nm, C.byref(m), C.byref(total))
    return buf[:nb], out_off, doc_idx


def select_docs_host(blob, doc_off, rows, n_cols, want=None, mode="any", also=None, cap_bytes=None, cap_docs=None, guard=0, out_shift=0,
                     count_only=False):
    """gft_debug_select_docs over host arrays -> (m, total, out uint8 [cap_bytes + guard], out_off uint64 [cap_docs + 1 + guard],
    doc_idx uint64 [cap_docs + guard]); no device needed.  Caps None: count first, then exactly what the result needs; the guard
    entries behind the caps hold 0xA5 and must come back untouched.  out_shift: the output starts that many bytes into its
    allocation's 16-byte grid.  out_off, with its cap_docs + 1 entries, is always passed; count_only: no array at all"""
    L = _lib.load()
    keep, n_docs, head, p_also = _docs_host_args(blob, doc_off, rows, n_cols, also)
    w = _want_words(want, n_cols)
    m, total = C.c_uint64(0), C.c_uint64(0)

    def call(out, cb, oo, di, cd):
        rc = L.gft_debug_select_docs(*head, _p(w), _select_mode(mode), p_also, out, cb, oo, di, cd, C.byref(m), C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_select_docs")
    if cap_bytes is None or cap_docs is None:
        call(None, 0, None, None, 0)
        cap_bytes = int(total.value) if cap_bytes is None else cap_bytes
        cap_docs = int(m.value) if cap_docs is None else cap_docs
    out, out_off, doc_idx = _docs_host_outputs(cap_bytes, cap_docs, guard, out_shift)
    if count_only:
        call(None, 0, None, None, 0)
    else:
        call(out.ctypes.data if cap_bytes or guard else None, cap_bytes, out_off.ctypes.data, doc_idx.ctypes.data if cap_docs or guard else None, cap_docs)
    return int(m.value), int(total.value), out, out_off, doc_idx


def select_shape():
    """(chunk, trip, tile) bytes of the select's copy kernel (gft_debug_select_shape)"""
    c, t, k = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _lib.load().gft_debug_select_shape(C.byref(c), C.byref(t), C.byref(k))
    return int(c.value), int(t.value), int(k.value)


CONTEXT_MAX = (1 << 64) - 1                         # before / after: every document up to the next fence


def context_docs_tensor(call, text, doc_off, bitmap, n_cols, want, mode, also, before, after, fence):
    """what Engine.context_docs_device and the finder's context call share: `call(d_text, d_doc_off, n_docs, d_bitmap, n_cols, want,
    mode, d_also, before, after, d_fence, d_out, cap_bytes, d_out_off, d_doc_idx, d_kind, cap_docs, d_group_off, cap_groups, byref(m),
    byref(hits), byref(groups), byref(total))` is gft_context_docs_device on some handle and raises on an error.  Two calls: count
    only, then into tensors of exactly the sizes counted"""
    import torch
    n_docs, head, d_also = _docs_tensor_args("context_docs_device", text, doc_off, bitmap, n_cols, also, fence)
    if not (0 <= int(before) <= CONTEXT_MAX and 0 <= int(after) <= CONTEXT_MAX):
        raise ValueError("context_docs_device: before and after are counts of documents, 0 .. 2^64 - 1")
    w = _want_words(want, n_cols)
    args = head + (_p(w), _select_mode(mode), d_also, int(before), int(after), fence.data_ptr() if fence is not None else None)
    m, hits, groups, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    counts = (C.byref(m), C.byref(hits), C.byref(groups), C.byref(total))
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, None, 0, None, None, None, 0, None, 0, *counts)
    nm, ng, nb = int(m.value), int(groups.value), int(total.value)
    buf, out_off, doc_idx = _docs_out_tensors(text, nm, nb)
    kind = torch.empty(nm, dtype=torch.uint8, device=text.device)
    group_off = torch.empty(ng + 1, dtype=torch.int64, device=text.device)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, buf.data_ptr(), nb, out_off.data_ptr(), doc_idx.data_ptr() if nm else None, kind.data_ptr() if nm else None, nm,
         group_off.data_ptr(), ng, *counts)
    return buf[:nb], out_off, doc_idx, kind, group_off


def context_docs_host(blob, doc_off, rows, n_cols, want=None, mode="any", also=None, before=0, after=0, fence=None, cap_bytes=None,
                      cap_docs=None, cap_groups=None, guard=0, out_shift=0, count_only=False):
    """gft_debug_context_docs over host arrays -> (m, hits, groups, total, out uint8 [cap_bytes + guard], out_off uint64 [cap_docs + 1 +
    guard], doc_idx uint64 [cap_docs + guard], kind uint8 [cap_docs + guard], group_off uint64 [cap_groups + 1 + guard]); no device
    needed.  Caps None: count first, then exactly what the result needs; the guard entries behind the caps hold 0xA5 and must come
    back untouched.  out_shift: the output starts that many bytes into its allocation's 16-byte grid.  The two offset arrays are
    always passed; count_only: no array at all"""
    L = _lib.load()
    keep, n_docs, head, p_also = _docs_host_args(blob, doc_off, rows, n_cols, also)
    fe = np.ascontiguousarray(fence, dtype=np.uint8) if fence is not None else None
    w = _want_words(want, n_cols)
    m, hits, groups, total = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(out, cb, oo, di, ki, cd, go, cg):
        rc = L.gft_debug_context_docs(*head, _p(w), _select_mode(mode), p_also, int(before), int(after), _p(fe), out, cb, oo, di, ki, cd, go, cg,
                                      C.byref(m), C.byref(hits), C.byref(groups), C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_context_docs")
    if cap_bytes is None or cap_docs is None or cap_groups is None:
        call(None, 0, None, None, None, 0, None, 0)
        cap_bytes = int(total.value) if cap_bytes is None else cap_bytes
        cap_docs = int(m.value) if cap_docs is None else cap_docs
        cap_groups = int(groups.value) if cap_groups is None else cap_groups
    out, out_off, doc_idx = _docs_host_outputs(cap_bytes, cap_docs, guard, out_shift)
    kind = np.full(cap_docs + guard, 0xA5, dtype=np.uint8)
    group_off = np.full(cap_groups + 1 + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    if count_only:
        call(None, 0, None, None, None, 0, None, 0)
    else:
        call(out.ctypes.data if cap_bytes or guard else None, cap_bytes, out_off.ctypes.data, doc_idx.ctypes.data if cap_docs or guard else None,
             kind.ctypes.data if cap_docs or guard else None, cap_docs, group_off.ctypes.data, cap_groups)
    return int(m.value), int(hits.value), int(groups.value), int(total.value), out, out_off, doc_idx, kind, group_off


def context_shape():
    """(documents per tile, tiles per carry block, carry blocks per trip of the spine) of the context kernels (gft_debug_context_shape)"""
    t, c, s = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _lib.load().gft_debug_context_shape(C.byref(t), C.byref(c), C.byref(s))
    return int(t.value), int(c.value), int(s.value)


ROUTE_MODES = {"first": 0, "every": 1}              # gft_route_mode
ROUTE_REST = 1                                      # GFT_ROUTE_REST
ROUTE_MAX_BUCKETS = 64                              # GFT_ROUTE_MAX_BUCKETS


def _route_mode(mode):
    return ROUTE_MODES[mode] if isinstance(mode, str) else int(mode)


def _mask_rows(masks, n_cols):
    """the host masks of a route call: (K, the K x ceil(n_cols / 32) uint32 words); masks is a sequence of K rows"""
    W = (n_cols + 31) // 32
    K = len(masks)
    if K and W:
        w = np.ascontiguousarray(np.asarray([np.asarray(m, dtype=np.uint32).reshape(-1) for m in masks], dtype=np.uint32))
        if w.shape != (K, W):
            raise ValueError("every mask must have ceil(n_cols / 32) words")
    else:
        w = np.zeros((K, W), dtype=np.uint32)
    return K, (w.reshape(-1) if w.size else np.zeros(1, dtype=np.uint32))


def route_docs_tensor(call, text, doc_off, bitmap, n_cols, masks, mode, rest, also, count_only=False):
    """what Engine.route_docs_device and the finders' route calls share: `call(d_text, d_doc_off, n_docs, d_bitmap, n_cols, masks,
    n_buckets, mode, flags, d_also, d_out, cap_bytes, d_out_off, d_doc_idx, cap_docs, bucket_doc, bucket_byte)` is
    gft_route_docs_device on some handle and raises on an error.  Two calls: count only, then into tensors of exactly the sizes
    counted.  count_only: the first call alone -> (bucket_doc, bucket_byte)"""
    import torch
    n_docs, head, d_also = _docs_tensor_args("route_docs_device", text, doc_off, bitmap, n_cols, also)
    K, w = _mask_rows(masks, n_cols)
    B = K + (1 if rest else 0)
    args = head + (_p(w), K, _route_mode(mode), ROUTE_REST if rest else 0, d_also)
    bucket_doc, bucket_byte = np.zeros(B + 1, dtype=np.uint64), np.zeros(B + 1, dtype=np.uint64)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, None, 0, None, None, 0, _p(bucket_doc), _p(bucket_byte))
    if count_only:
        return bucket_doc, bucket_byte
    nm, nb = int(bucket_doc[B]), int(bucket_byte[B])
    buf, out_off, doc_idx = _docs_out_tensors(text, nm, nb)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, buf.data_ptr(), nb, out_off.data_ptr(), doc_idx.data_ptr() if nm else None, nm, _p(bucket_doc), _p(bucket_byte))
    return buf[:nb], out_off, doc_idx, bucket_doc, bucket_byte


def route_docs_host(blob, doc_off, rows, n_cols, masks, mode="every", rest=False, also=None, cap_bytes=None, cap_docs=None, guard=0, out_shift=0,
                    count_only=False):
    """gft_debug_route_docs over host arrays -> (bucket_doc uint64 [B + 1], bucket_byte uint64 [B + 1], out uint8 [cap_bytes + guard],
    out_off uint64 [cap_docs + 1 + guard], doc_idx uint64 [cap_docs + guard]); no device needed.  Caps None: count first, then
    exactly what the result needs; the guard entries behind the caps hold 0xA5 and must come back untouched.  out_shift: the output
    starts that many bytes into its allocation's 16-byte grid.  count_only: no array at all"""
    L = _lib.load()
    keep, n_docs, head, p_also = _docs_host_args(blob, doc_off, rows, n_cols, also)
    K, w = _mask_rows(masks, n_cols)
    B = K + (1 if rest else 0)
    bucket_doc, bucket_byte = np.zeros(B + 1, dtype=np.uint64), np.zeros(B + 1, dtype=np.uint64)

    def call(out, cb, oo, di, cd):
        rc = L.gft_debug_route_docs(*head, _p(w), K, _route_mode(mode), ROUTE_REST if rest else 0, p_also, out, cb, oo, di, cd, _p(bucket_doc),
                                    _p(bucket_byte))
        if rc != 0:
            raise GftError(rc, "gft_debug_route_docs")
    if cap_bytes is None or cap_docs is None or count_only:
        call(None, 0, None, None, 0)
        cap_bytes = int(bucket_byte[B]) if cap_bytes is None else cap_bytes
        cap_docs = int(bucket_doc[B]) if cap_docs is None else cap_docs
    out, out_off, doc_idx = _docs_host_outputs(cap_bytes, cap_docs, guard, out_shift)
    if not count_only:
        call(out.ctypes.data if cap_bytes or guard else None, cap_bytes, out_off.ctypes.data, doc_idx.ctypes.data if cap_docs or guard else None, cap_docs)
    return bucket_doc, bucket_byte, out, out_off, doc_idx


def route_shape():
    """the documents a counting tile of the route kernels holds (gft_debug_route_shape)"""
    t = C.c_uint32(0)
    _lib.load().gft_debug_route_shape(C.byref(t))
    return int(t.value)


def hit_spans_tensor(call, text, doc_off, bitmap, n_cols, want, row_idx):
    """what Engine.hit_spans_device and Finder.SpansDevice share: `call(d_text, d_doc_off, n_docs, d_bitmap, d_row_idx, want, d_span_off,
    d_span_start, d_span_len, d_span_term, cap, byref(total))` is gft_hit_spans_device on some handle and raises on an error.  Two
    calls: count only, then into tensors of exactly the size counted.  Returns (span_off int64 [n + 1], start, len, term int32 [total])"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    W = (n_cols + 31) // 32
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off")) + (((bitmap, 4, "bitmap"),) if W and n_docs > 0 else ()) + \
            (((row_idx, 8, "row_idx"),) if row_idx is not None else ()):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("hit_spans_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or (row_idx is not None and row_idx.numel() != n_docs) or \
            (row_idx is None and W and n_docs > 0 and bitmap.numel() != n_docs * W):
        raise ValueError("hit_spans_device: doc_off, bitmap and row_idx do not describe the same batch")
    w = _want_words(want, n_cols)
    args = (text.data_ptr(), doc_off.data_ptr(), n_docs, bitmap.data_ptr() if W and n_docs > 0 else None,
            row_idx.data_ptr() if row_idx is not None else None, _p(w))
    total = C.c_uint64(0)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, None, None, None, None, 0, C.byref(total))
    n = int(total.value)
    span_off = torch.empty(n_docs + 1, dtype=torch.int64, device=text.device)
    start, length, term = (torch.empty(n, dtype=torch.int32, device=text.device) for _ in range(3))
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, span_off.data_ptr(), start.data_ptr() if n else None, length.data_ptr() if n else None, term.data_ptr() if n else None, n,
         C.byref(total))
    return span_off, start, length, term


def redact_spans_tensor(call, text, doc_off, span_off, start, length, mask):
    """gft_redact_spans_device through `call(d_text, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len, mask_byte)`, in place"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off"), (span_off, 8, "span_off"), (start, 4, "start"), (length, 4, "len")):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("redact_spans_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or span_off.numel() != n_docs + 1 or start.numel() != length.numel():
        raise ValueError("redact_spans_device: doc_off, span_off and the span arrays do not describe the same batch")
    mask = mask[0] if isinstance(mask, (bytes, bytearray)) else int(mask)
    torch.cuda.current_stream(text.device).synchronize()
    call(text.data_ptr(), doc_off.data_ptr(), n_docs, span_off.data_ptr(), start.data_ptr() if start.numel() else None,
         length.data_ptr() if length.numel() else None, mask)


def witness_terms_host(programs, n_terms, n_slots):
    """gft_debug_witness_terms over a list of postfix programs -> (off uint64 [n_terms + 1], expr uint32 []); no device needed"""
    L = _lib.load()
    words = np.asarray([w for p in programs for w in p], dtype=np.uint32)
    poff = np.zeros(len(programs) + 1, dtype=np.uint64)
    if programs:
        poff[1:] = np.cumsum([len(p) for p in programs], dtype=np.uint64)
    if words.size == 0:
        words = np.zeros(1, dtype=np.uint32)
    off = np.zeros(n_terms + 1, dtype=np.uint64)
    needed = C.c_uint64(0)
    rc = L.gft_debug_witness_terms(_p(words), _p(poff), len(programs), n_terms, n_slots, _p(off), None, 0, C.byref(needed))
    if rc != 0:
        raise GftError(rc, "gft_debug_witness_terms")
    expr = np.zeros(max(int(needed.value), 1), dtype=np.uint32)
    rc = L.gft_debug_witness_terms(_p(words), _p(poff), len(programs), n_terms, n_slots, _p(off), _p(expr), int(needed.value), C.byref(needed))
    if rc != 0:
        raise GftError(rc, "gft_debug_witness_terms")
    return off, expr[:int(needed.value)]


def hit_spans_host(match_off, term_id, pos, term_len, pos_end, wit_off, wit_expr, rows, n_exprs, row_idx=None, want=None, cap=None, guard=0,
                   with_len=True, with_term=True):
    """gft_debug_hit_spans over host arrays -> (total, span_off uint64 [n + 1 + guard], start, len, term uint32 [cap + guard]); no
    device needed.  cap None: count first, then exactly the total; the guard entries behind the caps hold 0xA5.. and must come back
    untouched.  with_len / with_term False: that array is not passed (None is returned for it)"""
    L = _lib.load()
    mo = np.ascontiguousarray(match_off, dtype=np.uint64)
    n_docs = mo.size - 1
    tid, ps = np.ascontiguousarray(term_id, dtype=np.uint32), np.ascontiguousarray(pos, dtype=np.uint32)
    tl = np.ascontiguousarray(term_len, dtype=np.uint32)
    wo, we = np.ascontiguousarray(wit_off, dtype=np.uint64), np.ascontiguousarray(wit_expr, dtype=np.uint32)
    W = (n_exprs + 31) // 32
    bm = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1) if W else None
    ri = np.ascontiguousarray(row_idx, dtype=np.uint64) if row_idx is not None else None
    w = _want_words(want, n_exprs)
    total = C.c_uint64(0)

    def call(so, a, b, c, cp):
        rc = L.gft_debug_hit_spans(_p(mo), _p(tid) if tid.size else None, _p(ps) if ps.size else None, n_docs, _p(tl) if tl.size else None, int(pos_end),
                                   _p(wo), _p(we) if we.size else None, _p(bm) if bm is not None and bm.size else None, n_exprs, _p(ri), _p(w),
                                   _p(so), _p(a), _p(b), _p(c), cp, C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_hit_spans")
    if cap is None:
        call(None, None, None, None, 0)
        cap = int(total.value)
    span_off = np.full(n_docs + 1 + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    arrs = [np.full(cap + guard, 0xA5A5A5A5, dtype=np.uint32) for _ in range(3)]
    call(span_off, arrs[0] if cap or guard else None, arrs[1] if with_len and (cap or guard) else None,
         arrs[2] if with_term and (cap or guard) else None, cap)
    return int(total.value), span_off, arrs[0], arrs[1] if with_len else None, arrs[2] if with_term else None


def redact_spans_host(blob, doc_off, span_off, start, length, mask=0x2A):
    """gft_debug_redact_spans over a copy of `blob` -> the masked bytes (numpy uint8); no device needed"""
    L = _lib.load()
    a = np.frombuffer(bytes(blob), dtype=np.uint8).copy() if not isinstance(blob, np.ndarray) else np.array(blob, dtype=np.uint8)
    off, so = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(span_off, dtype=np.uint64)
    st, ln = np.ascontiguousarray(start, dtype=np.uint32), np.ascontiguousarray(length, dtype=np.uint32)
    rc = L.gft_debug_redact_spans(_p(a) if a.size else None, _p(off), off.size - 1, _p(so), _p(st) if st.size else None, _p(ln) if ln.size else None,
                                  int(mask))
    if rc != 0:
        raise GftError(rc, "gft_debug_redact_spans")
    return a


def map_spans_to_source_tensor(call, text, doc_off, span_off, start, length):
    """gft_map_spans_to_source_device through `call(d_text, d_doc_off, n_docs, d_span_off, d_span_start, d_span_len)`, in place"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off"), (span_off, 8, "span_off"), (start, 4, "start"), (length, 4, "len")):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("map_spans_to_source_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or span_off.numel() != n_docs + 1 or start.numel() != length.numel():
        raise ValueError("map_spans_to_source_device: doc_off, span_off and the span arrays do not describe the same batch")
    torch.cuda.current_stream(text.device).synchronize()
    call(text.data_ptr(), doc_off.data_ptr(), n_docs, span_off.data_ptr(), start.data_ptr() if start.numel() else None,
         length.data_ptr() if length.numel() else None)


def map_spans_to_source_host(blob, doc_off, span_off, start, length):
    """gft_debug_map_spans_to_source: the spans (span_off uint64 [n + 1]; start, length: contiguous numpy uint32 arrays) of the
    lower-case form of the batch (blob, doc_off) become spans of the batch itself, IN PLACE; no device needed.  A refusal raises
    GftError and leaves both arrays as they were"""
    L = _lib.load()
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
    off, so = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(span_off, dtype=np.uint64)
    for t, what in ((start, "start"), (length, "length")):
        if not isinstance(t, np.ndarray) or t.dtype != np.uint32 or not t.flags.c_contiguous or not t.flags.writeable:
            raise ValueError("map_spans_to_source_host: %s must be a writable contiguous numpy uint32 array" % what)
    rc = L.gft_debug_map_spans_to_source(_p(a) if a.size else None, _p(off), off.size - 1, _p(so), _p(start) if start.size else None,
                                         _p(length) if length.size else None)
    if rc != 0:
        raise GftError(rc, "gft_debug_map_spans_to_source")


EXCERPT_RUNES = 1                                   # GFT_EXCERPT_RUNES
EXCERPT_WORDS = 2                                   # GFT_EXCERPT_WORDS
EXCERPT_LINES = 4                                   # GFT_EXCERPT_LINES
EXCERPT_REACH_MAX = 4096                            # GFT_EXCERPT_REACH_MAX


def excerpt_snap_flag(snap):
    """snap=None | "words" | "lines" -> the flag bit of the snapped calls"""
    try:
        return {None: 0, "words": EXCERPT_WORDS, "lines": EXCERPT_LINES}[snap]
    except (KeyError, TypeError):
        raise ValueError('snap must be None, "words" or "lines", not %r' % (snap,)) from None


def excerpt_spans_tensor(call, text, doc_off, span_off, start, length, before, after, runes, snap=None, reach=64):
    """what Engine.excerpt_spans_device and Finder.ExcerptsDevice share: `call(d_text, d_doc_off, n_docs, d_span_off, d_span_start,
    d_span_len, before, after, flags, d_out, cap_bytes, d_exc_off, d_exc_doc, d_exc_start, d_exc_span_off, cap_exc, d_span_rel,
    d_doc_exc_off, byref(n_exc), byref(total))` is gft_excerpt_spans_device on some handle and raises on an error.  Two calls: count
    only, then into tensors of exactly the sizes counted.  Returns (out uint8 [total] -- a view with 64 zero bytes behind it --,
    exc_off int64 [m + 1], exc_doc int64 [m], exc_start int32 [m], exc_span_off int64 [m + 1], span_rel int32 [spans], doc_exc_off
    int64 [n + 1]).  snap "words" / "lines": `call` is gft_excerpt_spans_snap_device and gets `reach` behind flags"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off"), (span_off, 8, "span_off"), (start, 4, "start"), (length, 4, "len")):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("excerpt_spans_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or span_off.numel() != n_docs + 1 or start.numel() != length.numel():
        raise ValueError("excerpt_spans_device: doc_off, span_off and the span arrays do not describe the same batch")
    args = (text.data_ptr(), doc_off.data_ptr(), n_docs, span_off.data_ptr(), start.data_ptr() if start.numel() else None,
            length.data_ptr() if length.numel() else None, int(before), int(after), (EXCERPT_RUNES if runes else 0) | excerpt_snap_flag(snap))
    if snap is not None:
        args += (int(reach),)
    m, total = C.c_uint64(0), C.c_uint64(0)
    dev = text.device
    torch.cuda.current_stream(dev).synchronize()
    call(*args, None, 0, None, None, None, None, 0, None, None, C.byref(m), C.byref(total))
    nm, nb = int(m.value), int(total.value)
    buf = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)          # (64 bytes of slack: the result is a blob for the next call)
    exc_off, exc_span_off = (torch.empty(nm + 1, dtype=torch.int64, device=dev) for _ in range(2))
    exc_doc = torch.empty(nm, dtype=torch.int64, device=dev)
    exc_start = torch.empty(nm, dtype=torch.int32, device=dev)
    span_rel = torch.zeros(start.numel(), dtype=torch.int32, device=dev)
    doc_exc_off = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    call(*args, buf.data_ptr(), nb, exc_off.data_ptr(), exc_doc.data_ptr() if nm else None, exc_start.data_ptr() if nm else None,
         exc_span_off.data_ptr(), nm, span_rel.data_ptr() if span_rel.numel() else None, doc_exc_off.data_ptr(), C.byref(m), C.byref(total))
    return buf[:nb], exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off


def excerpt_spans_host(blob, doc_off, span_off, start, length, before=40, after=40, runes=True, cap_bytes=None, cap_exc=None, guard=0,
                       flags=None, omit=(), count_only=False, snap=None, reach=64, snap_call=None):
    """gft_debug_excerpt_spans over host arrays -> a dict: n_exc, total, out uint8 [cap_bytes + guard], exc_off / exc_span_off uint64
    [cap_exc + 1 + guard], exc_doc uint64 / exc_start uint32 [cap_exc + guard], span_rel uint32 [len(start) + guard], doc_exc_off
    uint64 [n + 1 + guard]; no device needed.  Caps None: count first, then exactly what the result needs; the guard entries behind
    the caps hold 0xA5.. and must come back untouched.  omit: names of outputs passed as NULL (they come back as None).  snap
    "words" / "lines" (or snap_call=True with any flags): gft_debug_excerpt_spans_snap with `reach`"""
    L = _lib.load()
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
    off, so = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(span_off, dtype=np.uint64)
    st, ln = np.ascontiguousarray(start, dtype=np.uint32), np.ascontiguousarray(length, dtype=np.uint32)
    n_docs = off.size - 1
    fl = ((EXCERPT_RUNES if runes else 0) | excerpt_snap_flag(snap)) if flags is None else int(flags)
    snapped = (snap is not None) if snap_call is None else bool(snap_call)
    m, total = C.c_uint64(0), C.c_uint64(0)

    def call(out, cb, eo, ed, es, eso, ce, rel, deo):
        head = (_p(a) if a.size else None, _p(off), n_docs, _p(so), _p(st) if st.size else None, _p(ln) if ln.size else None, int(before), int(after), fl)
        tail = (_p(out), cb, _p(eo), _p(ed), _p(es), _p(eso), ce, _p(rel), _p(deo), C.byref(m), C.byref(total))
        rc = L.gft_debug_excerpt_spans_snap(*head, int(reach), *tail) if snapped else L.gft_debug_excerpt_spans(*head, *tail)
        if rc != 0:
            raise GftError(rc, "gft_debug_excerpt_spans_snap" if snapped else "gft_debug_excerpt_spans")
    if cap_bytes is None or cap_exc is None or count_only:
        call(None, 0, None, None, None, None, 0, None, None)
        cap_bytes = int(total.value) if cap_bytes is None else cap_bytes
        cap_exc = int(m.value) if cap_exc is None else cap_exc
    r = {"n_exc": int(m.value), "total": int(total.value)}
    if count_only:
        return r
    big = 0xA5A5A5A5A5A5A5A5
    arrs = {"out": np.full(cap_bytes + guard, 0xA5, dtype=np.uint8), "exc_off": np.full(cap_exc + 1 + guard, big, dtype=np.uint64),
            "exc_doc": np.full(cap_exc + guard, big, dtype=np.uint64), "exc_start": np.full(cap_exc + guard, 0xA5A5A5A5, dtype=np.uint32),
            "exc_span_off": np.full(cap_exc + 1 + guard, big, dtype=np.uint64), "span_rel": np.full(st.size + guard, 0xA5A5A5A5, dtype=np.uint32),
            "doc_exc_off": np.full(n_docs + 1 + guard, big, dtype=np.uint64)}
    for k in omit:
        arrs[k] = None
    for k in ("out", "exc_doc", "exc_start", "span_rel"):
        if arrs[k] is not None and arrs[k].size == 0:
            arrs[k] = None
    call(arrs["out"], cap_bytes if arrs["out"] is not None else 0, arrs["exc_off"], arrs["exc_doc"], arrs["exc_start"], arrs["exc_span_off"], cap_exc,
         arrs["span_rel"], arrs["doc_exc_off"])
    r.update(arrs, n_exc=int(m.value), total=int(total.value))
    return r


def excerpt_snap_edges(doc, lo, hi, snap, reach=64, runes=False, flags=None):
    """the snapped window of the clipped window [lo, hi) of one document (gft_debug_excerpt_snap_edges) -> (lo, hi); no device needed"""
    a = np.frombuffer(bytes(doc), dtype=np.uint8)
    fl = ((EXCERPT_RUNES if runes else 0) | excerpt_snap_flag(snap)) if flags is None else int(flags)
    lo_out, hi_out = C.c_uint64(0), C.c_uint64(0)
    rc = _lib.load().gft_debug_excerpt_snap_edges(_p(a) if a.size else None, a.size, int(lo), int(hi), fl, int(reach), C.byref(lo_out), C.byref(hi_out))
    if rc != 0:
        raise GftError(rc, "gft_debug_excerpt_snap_edges")
    return int(lo_out.value), int(hi_out.value)


def excerpt_shape():
    """(spans of a tile of the excerpts' suffix-minimum scan, tiles of one carry trip) (gft_debug_excerpt_shape)"""
    t, k = C.c_uint32(0), C.c_uint32(0)
    _lib.load().gft_debug_excerpt_shape(C.byref(t), C.byref(k))
    return int(t.value), int(k.value)


MARK_MAX = 255                                      # GFT_MARK_MAX


def mark_spans_tensor(call, text, doc_off, span_off, start, length, open=b"<em>", close=b"</em>"):
    """what Engine.mark_spans_device and Finder.MarkDevice share: `call(d_text, d_doc_off, n_docs, d_span_off, d_span_start,
    d_span_len, open, open_len, close, close_len, flags, d_out, cap_bytes, d_out_off, d_span_new, d_doc_run_off, byref(n_runs),
    byref(total))` is gft_mark_spans_device on some handle and raises on an error.  Two calls: count only with NULL outputs, then
    into tensors of exactly the sizes counted.  Returns (out uint8 [total] -- the marked documents back to back, a view with 64
    zero bytes behind it --, out_off int64 [n + 1], span_new int32 [spans], doc_run_off int64 [n + 1])"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off"), (span_off, 8, "span_off"), (start, 4, "start"), (length, 4, "len")):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("mark_spans_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or span_off.numel() != n_docs + 1 or start.numel() != length.numel():
        raise ValueError("mark_spans_device: doc_off, span_off and the span arrays do not describe the same batch")
    open, close = bytes(open), bytes(close)
    args = (text.data_ptr(), doc_off.data_ptr(), n_docs, span_off.data_ptr(), start.data_ptr() if start.numel() else None,
            length.data_ptr() if length.numel() else None, open or None, len(open), close or None, len(close), 0)
    m, total = C.c_uint64(0), C.c_uint64(0)
    dev = text.device
    torch.cuda.current_stream(dev).synchronize()
    call(*args, None, 0, None, None, None, C.byref(m), C.byref(total))
    nb = int(total.value)
    buf = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)          # (64 bytes of slack: the result is a blob for the next call)
    out_off, doc_run_off = (torch.empty(n_docs + 1, dtype=torch.int64, device=dev) for _ in range(2))
    span_new = torch.zeros(start.numel(), dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    call(*args, buf.data_ptr(), nb, out_off.data_ptr(), span_new.data_ptr() if span_new.numel() else None, doc_run_off.data_ptr(),
         C.byref(m), C.byref(total))
    return buf[:nb], out_off, span_new, doc_run_off


def mark_spans_host(blob, doc_off, span_off, start, length, open=b"<em>", close=b"</em>", cap_bytes=None, guard=0, flags=0, omit=(),
                    count_only=False, open_len=None, close_len=None, shift=0):
    """gft_debug_mark_spans over host arrays -> a dict: n_runs, total, out uint8 [cap_bytes + guard], out_off / doc_run_off uint64
    [n + 1 + guard], span_new uint32 [len(start) + guard]; no device needed.  cap_bytes None: count first, then exactly what the
    result needs; the guard entries behind hold 0xA5.. and must come back untouched.  omit: names of outputs passed as NULL (they
    come back as None).  open_len / close_len: lengths to pass instead of the markers' own; a marker None is passed as NULL.
    shift: bytes the output's first byte lies behind a 16-byte border"""
    L = _lib.load()
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
    off, so = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(span_off, dtype=np.uint64)
    st, ln = np.ascontiguousarray(start, dtype=np.uint32), np.ascontiguousarray(length, dtype=np.uint32)
    n_docs = off.size - 1
    ol = (len(open) if open is not None else 0) if open_len is None else int(open_len)
    cl = (len(close) if close is not None else 0) if close_len is None else int(close_len)
    m, total = C.c_uint64(0), C.c_uint64(0)

    def call(out, cb, oo, sn, dro):
        rc = L.gft_debug_mark_spans(_p(a) if a.size else None, _p(off), n_docs, _p(so), _p(st) if st.size else None, _p(ln) if ln.size else None,
                                    bytes(open) if open else None, ol, bytes(close) if close else None, cl, int(flags), _p(out), cb, _p(oo), _p(sn),
                                    _p(dro), C.byref(m), C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_mark_spans")
    if cap_bytes is None or count_only:
        call(None, 0, None, None, None)
        cap_bytes = int(total.value) if cap_bytes is None else cap_bytes
    r = {"n_runs": int(m.value), "total": int(total.value)}
    if count_only:
        return r
    big = 0xA5A5A5A5A5A5A5A5
    raw = np.full(cap_bytes + guard + 32, 0xA5, dtype=np.uint8)
    lead = (-raw.ctypes.data) % 16 + int(shift)
    arrs = {"out": raw[lead:lead + cap_bytes + guard], "out_off": np.full(n_docs + 1 + guard, big, dtype=np.uint64),
            "span_new": np.full(st.size + guard, 0xA5A5A5A5, dtype=np.uint32), "doc_run_off": np.full(n_docs + 1 + guard, big, dtype=np.uint64)}
    for k in omit:
        arrs[k] = None
    for k in ("out", "span_new"):
        if arrs[k] is not None and arrs[k].size == 0:
            arrs[k] = None
    r.update(arrs)
    call(arrs["out"], cap_bytes if arrs["out"] is not None else 0, arrs["out_off"], arrs["span_new"], arrs["doc_run_off"])
    r.update(n_runs=int(m.value), total=int(total.value))
    return r


def mark_shape():
    """(spans of a tile of the run passes' suffix-minimum scan, tiles of one carry trip, bytes of a lane's chunk of the output, bytes
    of a wave's tile) (gft_debug_mark_shape)"""
    v = [C.c_uint32(0) for _ in range(4)]
    _lib.load().gft_debug_mark_shape(*(C.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


REPLACE_MAX = 255                                   # GFT_REPLACE_MAX
REPLACE_MAX_REPS = 65536


def replace_table(reps):
    """a list of replacements (bytes each; one bytes object: a table of one) -> (rep_bytes, rep_off uint64 [n + 1]) as the replace
    calls take them"""
    if isinstance(reps, (bytes, bytearray, memoryview)):
        reps = [reps]
    reps = [bytes(r) for r in reps]
    off = np.zeros(len(reps) + 1, dtype=np.uint64)
    if reps:
        off[1:] = np.cumsum([len(r) for r in reps], dtype=np.uint64)
    return b"".join(reps), off


def replace_spans_tensor(call, text, doc_off, span_off, start, length, reps=b"[REDACTED]", key=None, key_rep=None):
    """what Engine.replace_spans_device and Finder.ReplaceDevice share: `call(d_text, d_doc_off, n_docs, d_span_off, d_span_start,
    d_span_len, d_span_key, key_rep, n_keys, rep_bytes, rep_off, n_reps, flags, d_out, cap_bytes, d_out_off, d_doc_run_off, d_run_new,
    d_run_len, d_run_rep, cap_runs, byref(n_runs), byref(total))` is gft_replace_spans_device on some handle and raises on an error.
    Two calls: count only with NULL outputs, then into tensors of exactly the sizes counted.  Returns (out uint8 [total] -- the
    replaced documents back to back, a view with 64 zero bytes behind it --, out_off int64 [n + 1], doc_run_off int64 [n + 1],
    run_new, run_len, run_rep int32 [runs])"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    checks = [(text, 1, "text"), (doc_off, 8, "doc_off"), (span_off, 8, "span_off"), (start, 4, "start"), (length, 4, "len")]
    if key is not None:
        checks.append((key, 4, "key"))
    for t, size, what in checks:
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("replace_spans_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or span_off.numel() != n_docs + 1 or start.numel() != length.numel() or (key is not None and key.numel() != start.numel()):
        raise ValueError("replace_spans_device: doc_off, span_off and the span arrays do not describe the same batch")
    rep_bytes, rep_off = replace_table(reps)
    kr = None if key_rep is None else np.ascontiguousarray(key_rep, dtype=np.uint32)
    args = (text.data_ptr(), doc_off.data_ptr(), n_docs, span_off.data_ptr(), start.data_ptr() if start.numel() else None,
            length.data_ptr() if length.numel() else None, key.data_ptr() if key is not None and key.numel() else None,
            _p(kr) if kr is not None else None, kr.size if kr is not None else 0, rep_bytes or None, _p(rep_off), rep_off.size - 1, 0)
    m, total = C.c_uint64(0), C.c_uint64(0)
    dev = text.device
    torch.cuda.current_stream(dev).synchronize()
    call(*args, None, 0, None, None, None, None, None, 0, C.byref(m), C.byref(total))
    nb, nr = int(total.value), int(m.value)
    buf = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)          # (64 bytes of slack: the result is a blob for the next call)
    out_off, doc_run_off = (torch.empty(n_docs + 1, dtype=torch.int64, device=dev) for _ in range(2))
    run_new, run_len, run_rep = (torch.zeros(nr, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.current_stream(dev).synchronize()
    call(*args, buf.data_ptr(), nb, out_off.data_ptr(), doc_run_off.data_ptr(), *((t.data_ptr() if nr else None) for t in (run_new, run_len, run_rep)),
         nr, C.byref(m), C.byref(total))
    return buf[:nb], out_off, doc_run_off, run_new, run_len, run_rep


REPLACE_OUTPUTS = ("out", "out_off", "doc_run_off", "run_new", "run_len", "run_rep")


def replace_spans_host(blob, doc_off, span_off, start, length, reps=b"[REDACTED]", key=None, key_rep=None, cap_bytes=None, cap_runs=None,
                       guard=0, flags=0, omit=(), count_only=False, shift=0, table=None, n_keys=None):
    """gft_debug_replace_spans over host arrays -> a dict: n_runs, total, out uint8 [cap_bytes + guard], out_off / doc_run_off uint64
    [n + 1 + guard], run_new / run_len / run_rep uint32 [cap_runs + guard]; no device needed.  A cap None: count first, then exactly
    what the result needs; the guard entries behind hold 0xA5.. and must come back untouched.  omit: names of outputs passed as NULL
    (they come back as None).  key: the spans' keys, parallel to start (None: NULL); key_rep: the key map (None: NULL), n_keys: the
    count to pass instead of its own.  table: (rep_bytes or None, rep_off, n_reps) to pass as they are instead of `reps`.  shift:
    bytes the output's first byte lies behind a 16-byte border"""
    L = _lib.load()
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
    off, so = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(span_off, dtype=np.uint64)
    st, ln = np.ascontiguousarray(start, dtype=np.uint32), np.ascontiguousarray(length, dtype=np.uint32)
    ky = None if key is None else np.ascontiguousarray(key, dtype=np.uint32)
    kr = None if key_rep is None else np.ascontiguousarray(key_rep, dtype=np.uint32)
    nk = (kr.size if kr is not None else 0) if n_keys is None else int(n_keys)
    n_docs = off.size - 1
    if table is None:
        rep_bytes, rep_off = replace_table(reps)
        n_reps = rep_off.size - 1
    else:
        rep_bytes, rep_off, n_reps = table
        rep_off = None if rep_off is None else np.ascontiguousarray(rep_off, dtype=np.uint64)
    m, total = C.c_uint64(0), C.c_uint64(0)

    def call(out, cb, oo, dro, rn, rl, rr, cr):
        rc = L.gft_debug_replace_spans(_p(a) if a.size else None, _p(off), n_docs, _p(so), _p(st) if st.size else None, _p(ln) if ln.size else None,
                                       _p(ky) if ky is not None and ky.size else None, _p(kr) if kr is not None and kr.size else None, nk,
                                       rep_bytes or None, _p(rep_off), int(n_reps), int(flags), _p(out), cb, _p(oo), _p(dro), _p(rn), _p(rl),
                                       _p(rr), cr, C.byref(m), C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_replace_spans")
    if cap_bytes is None or cap_runs is None or count_only:
        call(None, 0, None, None, None, None, None, 0)
        cap_bytes = int(total.value) if cap_bytes is None else cap_bytes
        cap_runs = int(m.value) if cap_runs is None else cap_runs
    r = {"n_runs": int(m.value), "total": int(total.value)}
    if count_only:
        return r
    big = 0xA5A5A5A5A5A5A5A5
    raw = np.full(cap_bytes + guard + 32, 0xA5, dtype=np.uint8)
    lead = (-raw.ctypes.data) % 16 + int(shift)
    arrs = {"out": raw[lead:lead + cap_bytes + guard], "out_off": np.full(n_docs + 1 + guard, big, dtype=np.uint64),
            "doc_run_off": np.full(n_docs + 1 + guard, big, dtype=np.uint64)}
    for k in ("run_new", "run_len", "run_rep"):
        arrs[k] = np.full(cap_runs + guard, 0xA5A5A5A5, dtype=np.uint32)
    for k in omit:
        arrs[k] = None
    for k in ("out", "run_new", "run_len", "run_rep"):
        if arrs[k] is not None and arrs[k].size == 0:
            arrs[k] = None
    r.update(arrs)
    call(arrs["out"], cap_bytes if arrs["out"] is not None else 0, arrs["out_off"], arrs["doc_run_off"], arrs["run_new"], arrs["run_len"],
         arrs["run_rep"], cap_runs)
    r.update(n_runs=int(m.value), total=int(total.value))
    return r


def replace_shape():
    """(spans of a tile of the run passes' suffix-minimum scan, tiles of one carry trip, bytes of a lane's chunk of the output, bytes
    of a wave's tile, plan entries of a wave's window, bytes of a table that goes into LDS) (gft_debug_replace_shape)"""
    v = [C.c_uint32(0) for _ in range(6)]
    _lib.load().gft_debug_replace_shape(*(C.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


STATS_SHAPE_FIELDS = ("step_entries", "step_docs", "set_slots", "cache_slots", "large_entries", "bitset_lds_terms", "range_weight", "column_rows")


def stats_shape():
    """the borders of the term statistics' walk as a dict (gft_debug_stats_shape): STATS_SHAPE_FIELDS"""
    v = [C.c_uint32(0) for _ in STATS_SHAPE_FIELDS]
    _lib.load().gft_debug_stats_shape(*(C.byref(x) for x in v))
    return {k: int(x.value) for k, x in zip(STATS_SHAPE_FIELDS, v)}


def term_stats_host(off, term, n_terms, occ=None, docs=None, first=None, flags=0, doc_base=0, n_docs=None):
    """gft_debug_term_stats over host arrays, in place: off uint64 [n_docs + 1], term uint32 (indexed by off's values), occ / docs /
    first uint64 [n_terms] or None (passed as NULL).  Raises GftError on a refusal; no device needed"""
    o, t = np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(term, dtype=np.uint32)
    n_docs = o.size - 1 if n_docs is None else n_docs
    for a in (occ, docs, first):
        assert a is None or (a.dtype == np.uint64 and a.flags.c_contiguous)
    rc = _lib.load().gft_debug_term_stats(_p(o) if o.size else None, _p(t) if t.size else None, n_docs, n_terms, int(flags), int(doc_base),
                                          _p(occ), _p(docs), _p(first))
    if rc != 0:
        raise GftError(rc, "gft_debug_term_stats")


def count_columns_host(bitmap, n_rows, n_cols, count, row_idx=None, flags=0):
    """gft_debug_count_columns over host arrays, in place: bitmap uint32 rows of ceil(n_cols / 32) words, count uint64 [n_cols],
    row_idx uint64 [n_rows] or None.  Raises GftError on a refusal; no device needed"""
    bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
    ri = np.ascontiguousarray(row_idx, dtype=np.uint64) if row_idx is not None else None
    rc = _lib.load().gft_debug_count_columns(_p(bm) if bm.size else None, n_rows, n_cols, _p(ri) if ri is not None and ri.size else None,
                                             int(flags), _p(count) if count is not None and count.size else None)
    if rc != 0:
        raise GftError(rc, "gft_debug_count_columns")


RANK_SHAPE_FIELDS = ("step_entries", "step_docs", "large_entries", "set_slots", "weight_lds_terms", "bitset_lds_terms", "range_weight",
                     "digit_bits", "place_tile", "max_k")


def rank_shape():
    """the borders of the ranking's walks as a dict (gft_debug_rank_shape): RANK_SHAPE_FIELDS"""
    v = [C.c_uint32(0) for _ in RANK_SHAPE_FIELDS]
    _lib.load().gft_debug_rank_shape(*(C.byref(x) for x in v))
    return {k: int(x.value) for k, x in zip(RANK_SHAPE_FIELDS, v)}


def score_docs_host(off, term, n_terms, weights=None, distinct=False, score=None, flags=None, n_docs=None):
    """gft_debug_score_docs over host arrays: off uint64 [n_docs + 1], term uint32 (indexed by off's values), weights uint32 [n_terms]
    or None (every term 1) -> (score uint64 [n_docs] -- the given array, in place, or a new one --, max_score).  Raises GftError on a
    refusal; no device needed"""
    o, t = np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(term, dtype=np.uint32)
    n_docs = max(o.size - 1, 0) if n_docs is None else n_docs
    w = np.ascontiguousarray(weights, dtype=np.uint32) if weights is not None else None
    score = np.zeros(n_docs, dtype=np.uint64) if score is None else score
    assert score.dtype == np.uint64 and score.flags.c_contiguous
    mx = C.c_uint64(0)
    rc = _lib.load().gft_debug_score_docs(_p(o) if o.size else None, _p(t) if t.size else None, n_docs, n_terms, _p(w) if w is not None and w.size else None,
                                          int(flags) if flags is not None else (_lib.GFT_SCORE_DISTINCT if distinct else 0),
                                          _p(score) if score.size else None, C.byref(mx))
    if rc != 0:
        raise GftError(rc, "gft_debug_score_docs")
    return score, int(mx.value)


def top_docs_host(score, k, doc_base=0, top_idx=None, top_score=None, n_docs=None):
    """gft_debug_top_docs over a host uint64 array -> (top_idx, top_score) uint64 [n_top]; with the two arrays given ([k], written in
    place up to n_top) -> n_top.  Raises GftError on a refusal; no device needed"""
    sc = np.ascontiguousarray(score, dtype=np.uint64)
    n_docs = sc.size if n_docs is None else n_docs
    given = top_idx is not None
    if not given:
        top_idx, top_score = np.zeros(max(k, 1), dtype=np.uint64), np.zeros(max(k, 1), dtype=np.uint64)
    n = C.c_uint64(0)
    rc = _lib.load().gft_debug_top_docs(_p(sc) if sc.size else None, n_docs, int(k), int(doc_base), _p(top_idx), _p(top_score), C.byref(n))
    if rc != 0:
        raise GftError(rc, "gft_debug_top_docs")
    return int(n.value) if given else (top_idx[:n.value], top_score[:n.value])


def gather_docs_host(blob, doc_off, idx, idx_base=0, cap_bytes=None, guard=0, out_shift=0):
    """gft_debug_gather_docs over host arrays -> (total, out uint8 [cap_bytes + guard], out_off uint64 [m + 1 + guard]); no device
    needed.  cap_bytes None: count first (out NULL, cap 0), then exactly what the result needs; the guard entries behind the caps
    hold 0xA5 and must come back untouched; out_shift as select_docs_host takes it"""
    L = _lib.load()
    a = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
    off, ix = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(idx, dtype=np.uint64)
    n_docs, m = max(off.size - 1, 0), ix.size
    total = C.c_uint64(0)

    def call(out, cb, oo):
        rc = L.gft_debug_gather_docs(a.ctypes.data if a.size else None, _p(off) if n_docs else None, n_docs, _p(ix) if m else None, m, int(idx_base), out, cb,
                                     oo, C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_gather_docs")
    if cap_bytes is None:
        call(None, 0, np.zeros(m + 1, dtype=np.uint64).ctypes.data)
        cap_bytes = int(total.value)
    out, out_off, _ = _docs_host_outputs(cap_bytes, m, guard, out_shift)
    call(out.ctypes.data if cap_bytes else None, cap_bytes, out_off.ctypes.data)
    return int(total.value), out, out_off


WORDS_POS_END = 1                                   # GFT_WORDS_POS_END


def word_rune(cp):
    """True when cp is a word rune of the whole-word rule (gft_debug_word_rune): category L*, M*, N* or Pc"""
    return bool(_lib.load().gft_debug_word_rune(int(cp)))


def words_shape():
    """the borders of the word filter's walk as a dict (gft_debug_words_shape): tile_entries, table_rows, table_bytes"""
    v = [C.c_uint32(0) for _ in range(3)]
    _lib.load().gft_debug_words_shape(*(C.byref(x) for x in v))
    return dict(zip(("tile_entries", "table_rows", "table_bytes"), (int(x.value) for x in v)))


def filter_word_matches_host(blob, doc_off, off, pos, length=None, term=None, term_len=None, pos_end=False, cap=None, guard=0, flags=None,
                             with_len=True, with_term=True):
    """gft_debug_filter_word_matches over host arrays -> (total, out_off uint64 [n + 1 + guard], pos, len, term uint32 [cap + guard]); no
    device needed.  off uint64 [n_docs + 1] (off[0] may be non-zero), pos / length / term uint32 indexed by off's values; length
    None: the lengths are term_len[term].  cap None: count first, then exactly the total; the guard entries behind the caps hold
    0xA5.. and must come back untouched.  with_len / with_term False: that output is not passed (None is returned for it)"""
    L = _lib.load()
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    do, o = np.ascontiguousarray(doc_off, dtype=np.uint64), np.ascontiguousarray(off, dtype=np.uint64)
    n_docs = do.size - 1
    ps = np.ascontiguousarray(pos, dtype=np.uint32)
    ln = np.ascontiguousarray(length, dtype=np.uint32) if length is not None else None
    tm = np.ascontiguousarray(term, dtype=np.uint32) if term is not None else None
    tl = np.ascontiguousarray(term_len, dtype=np.uint32) if term_len is not None else None
    fl = (WORDS_POS_END if pos_end else 0) if flags is None else int(flags)
    with_term = with_term and tm is not None
    total = C.c_uint64(0)
    opt = lambda a: _p(a) if a is not None and a.size else None     # noqa: E731

    def call(oo, a, bb, c, cp):
        rc = L.gft_debug_filter_word_matches(opt(b), _p(do), n_docs, _p(o), opt(ps), opt(ln), opt(tm), opt(tl), tl.size if tl is not None else 0, fl,
                                             _p(oo), _p(a), _p(bb), _p(c), cp, C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_filter_word_matches")
    if cap is None:
        call(None, None, None, None, 0)
        cap = int(total.value)
    out_off = np.full(n_docs + 1 + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    arrs = [np.full(cap + guard, 0xA5A5A5A5, dtype=np.uint32) for _ in range(3)]
    call(out_off, arrs[0] if cap or guard else None, arrs[1] if with_len and (cap or guard) else None,
         arrs[2] if with_term and (cap or guard) else None, cap)
    return int(total.value), out_off, arrs[0], arrs[1] if with_len else None, arrs[2] if with_term else None


def filter_word_matches_tensor(call, text, doc_off, off, pos, length, term, term_len, pos_end):
    """gft_filter_word_matches_device through `call(d_text, d_doc_off, n_docs, d_off, d_pos, d_len, d_term, d_term_len, n_terms, flags,
    d_out_off, d_out_pos, d_out_len, d_out_term, cap, byref(total))`.  Two calls: count only, then into tensors of exactly the size
    counted.  Returns (out_off int64 [n + 1], pos, len, term int32 [total]; term None without term ids)"""
    import torch
    n_docs = int(doc_off.numel()) - 1
    for t, size, what in ((text, 1, "text"), (doc_off, 8, "doc_off"), (off, 8, "off"), (pos, 4, "pos")) + \
            tuple((t, 4, w) for t, w in ((length, "length"), (term, "term"), (term_len, "term_len")) if t is not None):
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != size:
            raise ValueError("filter_word_matches_device: %s must be a contiguous device tensor of %d-byte integers" % (what, size))
    if n_docs < 0 or off.numel() != n_docs + 1 or (length is None and (term is None or term_len is None)):
        raise ValueError("filter_word_matches_device: doc_off, off and the entry arrays do not describe the same list")
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
    args = (ptr(text), doc_off.data_ptr(), n_docs, off.data_ptr(), ptr(pos), ptr(length), ptr(term), ptr(term_len),
            int(term_len.numel()) if term_len is not None else 0, WORDS_POS_END if pos_end else 0)
    total = C.c_uint64(0)
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, None, None, None, None, 0, C.byref(total))
    n = int(total.value)
    out_off = torch.empty(n_docs + 1, dtype=torch.int64, device=text.device)
    o_pos, o_len, o_term = (torch.empty(n, dtype=torch.int32, device=text.device) for _ in range(3))
    torch.cuda.current_stream(text.device).synchronize()
    call(*args, out_off.data_ptr(), ptr(o_pos), ptr(o_len), ptr(o_term) if term is not None else None, n, C.byref(total))
    return out_off, o_pos, o_len, (o_term if term is not None else None)


def lowermap_shape():
    """(bytes of a piece, of a wave's trip, of a work unit at most, spans of a wave's tile) (gft_debug_lowermap_shape)"""
    v = [C.c_uint32(0) for _ in range(4)]
    _lib.load().gft_debug_lowermap_shape(*(C.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


def spans_shape():
    """(matches a workgroup of the mark pass takes per step, spans a wave of the fill owns) (gft_debug_spans_shape)"""
    t, k = C.c_uint32(0), C.c_uint32(0)
    _lib.load().gft_debug_spans_shape(C.byref(t), C.byref(k))
    return int(t.value), int(k.value)


class Engine:
    """Thin object wrapper of the C ABI (one gft_engine handle)."""

    def __init__(self, device=-1, devices=None):
        """devices: a list of HIP device ordinals -> one handle over all of them (gft_engine_create_multi)"""
        self._L = _lib.load()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            rc = self._L.gft_engine_create_multi(C.byref(h), C.cast(arr, C.c_void_p), len(devices))
        else:
            rc = self._L.gft_engine_create(C.byref(h), device)
        self._h = h
        self.warning = None
        if rc == _lib.GFT_W_NO_RCCL:          # a complete handle whose gathers are device-to-device copies, not RCCL's
            self.warning = self._L.gft_last_error(h).decode()
            rc = 0
        if rc != 0:
            msg = self._L.gft_last_error(h).decode() if h else "engine_create failed"
            self.close()
            raise GftError(rc, msg)

    def close(self):
        if getattr(self, "_h", None):
            self._L.gft_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise GftError(rc, self._L.gft_last_error(self._h).decode())

    def gather_mode(self):
        """"rccl" / "copy" / "" -- how gft_process_device_multi moves the shards' bitmaps (gft_gather_mode)"""
        return self._L.gft_gather_mode(self._h).decode()

    def set_stream(self, stream_ptr):
        self._check(self._L.gft_set_stream(self._h, stream_ptr))

    # -- SubstringEngine.BuildEngine ---------------------------------------------------------------
    def build(self, terms, pos_end=False):
        blob, off = pack(terms)
        self._check(self._L.gft_build(self._h, _p(blob), _p(off), len(terms), 1 if pos_end else 0))

    def export_tables(self):
        """the compiled tables of the current dictionary as bytes (gft_export_tables)"""
        need = C.c_uint64(0)
        self._L.gft_export_tables(self._h, None, 0, C.byref(need))
        if not need.value:
            self._check(_lib.GFT_E_NOT_BUILT)
        buf = (C.c_uint8 * need.value)()
        self._check(self._L.gft_export_tables(self._h, C.cast(buf, C.c_void_p), need.value, C.byref(need)))
        return bytes(buf)

    def import_tables(self, blob):
        """install tables written by export_tables: same effect as the build() that produced them"""
        self._check(self._L.gft_import_tables(self._h, blob, len(blob)))

    @property
    def n_terms(self):
        return self._L.gft_n_terms(self._h)

    @property
    def n_states(self):
        return self._L.gft_n_states(self._h)

    def term(self, i):
        p, n = C.c_void_p(), C.c_uint32()
        self._check(self._L.gft_term(self._h, i, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value)

    def terms(self):
        return [self.term(i) for i in range(self.n_terms)]

    def term_id(self, t):
        b = t.encode() if isinstance(t, str) else bytes(t)
        return int(self._L.gft_term_id(self._h, b, len(b)))

    # -- SubstringEngine.FindSubstrings, batched ------------------------------------------------------
    def scan(self, blob, doc_off, fold=False, unique=False, runes=False):
        """host numpy in -> CSR numpy out (match_off u64, term_id u32, pos u32).  unique=True: CloudflareEngine's output
        (GFT_SCAN_UNIQUE: every term once per document, first-occurrence order, positions 0)"""
        m = GftMatches()
        n_docs = len(doc_off) - 1
        self._check(self._L.gft_scan(self._h, _p(blob), _p(doc_off), n_docs, (1 if fold else 0) | (2 if unique else 0) | (4 if runes else 0), C.byref(m)))
        nm = int(m.n_matches)
        mo = np.ctypeslib.as_array(C.cast(m.match_off, C.POINTER(C.c_uint64)), shape=(n_docs + 1,)).copy()
        if nm == 0:
            return mo, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        ti = np.ctypeslib.as_array(C.cast(m.term_id, C.POINTER(C.c_uint32)), shape=(nm,)).copy()
        po = np.ctypeslib.as_array(C.cast(m.pos, C.POINTER(C.c_uint32)), shape=(nm,)).copy()
        return mo, ti, po

    def scan_device(self, d_text_ptr, d_doc_off_ptr, n_docs, fold=False, unique=False):
        """device pointers in -> GftMatches with DEVICE pointers (valid until the next call)"""
        m = GftMatches()
        self._check(self._L.gft_scan_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, (1 if fold else 0) | (2 if unique else 0), C.byref(m)))
        return m

    # -- solver ---------------------------------------------------------------------------------------
    def set_programs(self, programs, n_extra=0):
        """programs: list of lists of uint32 words"""
        off = np.zeros(len(programs) + 1, dtype=np.uint64)
        if programs:
            off[1:] = np.cumsum([len(p) for p in programs], dtype=np.uint64)
        words = np.asarray([w for p in programs for w in p] or [0], dtype=np.uint32)
        self._check(self._L.gft_set_programs(self._h, _p(words), _p(off), len(programs), n_extra))

    @property
    def n_exprs(self):
        return self._L.gft_n_exprs(self._h)

    def process(self, blob, doc_off, fold=False, extra=None):
        """host numpy in -> uint32 bitmap [n_docs, ceil(E/32)]"""
        n_docs = len(doc_off) - 1
        words = (self.n_exprs + 31) // 32
        bm = np.zeros((n_docs, words), dtype=np.uint32)
        x = None
        if extra is not None:
            eo, es, ep = extra
            keep = (eo, es, ep)  # noqa: F841  (keep arrays alive across the call)
            x = GftExtra(eo.ctypes.data, es.ctypes.data, ep.ctypes.data)
        self._check(self._L.gft_process(self._h, _p(blob), _p(doc_off), n_docs, 1 if fold else 0,
                                        C.byref(x) if x is not None else None, _p(bm) if bm.size else None))
        return bm

    def process_device(self, d_text_ptr, d_doc_off_ptr, n_docs, d_bitmap_ptr, fold=False, d_extra=None):
        x = None
        if d_extra is not None:
            x = GftExtra(*d_extra)
        self._check(self._L.gft_process_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, 1 if fold else 0,
                                               C.byref(x) if x is not None else None, d_bitmap_ptr))

    # -- sparse results: the batch form of []ExpressionResult ----------------------------------------------
    def set_expr_labels(self, labels):
        """one uint32 per expression (the finder puts tag ids there); None clears.  Any set_programs clears them"""
        if labels is None:
            self._check(self._L.gft_set_expr_labels(self._h, None, 0))
            return
        a = np.ascontiguousarray(labels, dtype=np.uint32)
        self._check(self._L.gft_set_expr_labels(self._h, _p(a) if a.size else None, a.size))

    def compact_device(self, d_bitmap_ptr, n_docs, d_row_off_ptr, d_expr_idx_ptr, d_label_ptr, cap, want_total=True):
        """device bitmap -> device CSR (gft_compact_device).  Entries at positions >= cap are not written; row_off is always
        complete.  want_total=True: waits and returns the total; False: only enqueues (the total is in d_row_off[n_docs])
        and returns None -- the form that is allowed while batches of process_device_begin are in flight"""
        total = C.c_uint64(0)
        self._check(self._L.gft_compact_device(self._h, d_bitmap_ptr, n_docs, d_row_off_ptr, d_expr_idx_ptr, d_label_ptr, cap,
                                               C.byref(total) if want_total else None))
        return int(total.value) if want_total else None

    def to_lower_device(self, d_text_ptr, d_doc_off_ptr, n_docs, d_out_ptr, cap, d_out_off_ptr):
        """strings.ToLower of a device-resident batch (gft_to_lower_device) -> the lowered size.  d_out_off (n_docs + 1 u64) is
        always complete; bytes at output positions >= cap are not written; d_out_ptr None with cap 0 counts only"""
        total = C.c_uint64(0)
        self._check(self._L.gft_to_lower_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, d_out_ptr, cap, d_out_off_ptr,
                                                C.byref(total)))
        return int(total.value)

    def split_lines_device(self, buf, length, mode=SPLIT_AFTER_NL):
        """a resident blob -> its documents' offsets, made on the device (gft_split_lines_device).  buf: a contiguous torch.uint8
        device tensor with buf.numel() >= length + 64; mode: SPLIT_AFTER_NL (a document per line, the newline stays with it) or
        SPLIT_JSON_LINES (a document per non-blank line, blank lines travel with the document in front).  Returns a torch.int64
        device tensor of n + 1 offsets (one entry, 0, for n == 0) -- what every *_device batch call takes as doc_off.  The call
        runs twice: count only, then into a tensor of exactly n + 1 entries"""
        return split_lines_tensor(lambda *a: self._check(self._L.gft_split_lines_device(self._h, *a)), buf, length, mode)

    def select_docs_device(self, text, doc_off, bitmap, n_cols, want=None, mode="any", also=None):
        """the documents of a resident batch whose rows hit `want`, gathered on the device (gft_select_docs_device).  text: torch.uint8
        with 64 readable bytes behind doc_off[-1]; doc_off: int64 [n + 1]; bitmap: int32 [n, ceil(n_cols / 32)] (not read for
        n_cols == 0); want: None (every column) or ceil(n_cols / 32) host uint32 words; mode: "any", "all" or "none"; also: uint8 [n],
        non-zero selects the document whatever its row says.  Returns device tensors (out uint8 [total] -- the selected documents
        back to back in input order, a view with 64 zero bytes behind it --, out_off int64 [m + 1], doc_idx int64 [m]).  The call
        runs twice: count only, then into tensors of exactly those sizes"""
        return select_docs_tensor(lambda *a: self._check(self._L.gft_select_docs_device(self._h, *a)), text, doc_off, bitmap, n_cols, want,
                                  mode, also)

    def context_docs_device(self, text, doc_off, bitmap, n_cols, want=None, mode="any", also=None, before=0, after=0, fence=None):
        """grep -A / -B / -C over a resident batch (gft_context_docs_device): the selected documents of select_docs_device and,
        round each of them, up to `before` documents in front and `after` behind (CONTEXT_MAX: no limit).  fence: uint8 [n], a
        non-zero byte at f lets no context cross between f - 1 and f.  Tensors as for select_docs_device.  Returns device tensors
        (out uint8 [total], out_off int64 [m + 1], doc_idx int64 [m], kind uint8 [m] -- 1: selected, 0: context only --, group_off
        int64 [g + 1]: the ranks at which the runs of consecutive kept documents begin, group_off[g] = m).  The call runs twice:
        count only, then into tensors of exactly those sizes"""
        return context_docs_tensor(lambda *a: self._check(self._L.gft_context_docs_device(self._h, *a)), text, doc_off, bitmap, n_cols,
                                   want, mode, also, before, after, fence)

    def route_docs_device(self, text, doc_off, bitmap, n_cols, masks, mode="every", rest=False, also=None):
        """the documents of a resident batch routed to one bucket per mask, on the device (gft_route_docs_device).  Tensors as for
        select_docs_device; masks: a sequence of K rows of ceil(n_cols / 32) uint32 words (host).  mode "every": a document goes to
        every bucket whose mask its row hits; "first": to the lowest-numbered one only.  rest: one more bucket, the last, for the
        documents that hit no mask; also (needs rest): uint8 [n_docs], non-zero sends the document to the rest bucket alone.
        Returns (out uint8 -- one blob, every bucket a contiguous run, input order inside a bucket --, out_off int64 [m + 1],
        doc_idx int64 [m]) on the device and (bucket_doc, bucket_byte) uint64 [B + 1] on the host: bucket b is entries
        bucket_doc[b]:bucket_doc[b + 1] and bytes bucket_byte[b]:bucket_byte[b + 1].  Counts first, then fills"""
        return route_docs_tensor(lambda *a: self._check(self._L.gft_route_docs_device(self._h, *a)), text, doc_off, bitmap, n_cols, masks, mode,
                                 rest, also)

    def route_count_device(self, text, doc_off, bitmap, n_cols, masks, mode="every", rest=False, also=None):
        """the count-only form of route_docs_device -> (bucket_doc, bucket_byte): how many documents and bytes every bucket gets,
        with nothing but those 2 (B + 1) numbers crossing the link"""
        return route_docs_tensor(lambda *a: self._check(self._L.gft_route_docs_device(self._h, *a)), text, doc_off, bitmap, n_cols, masks, mode,
                                 rest, also, count_only=True)

    def hit_spans_device(self, text, doc_off, bitmap, want=None, row_idx=None, fold=False):
        """where the expressions matched (gft_hit_spans_device): for a resident batch and its hit rows -- as process_device left them
        --, the byte spans of the keyword occurrences that belong to a true, wanted expression.  Tensors as for select_docs_device;
        want: None (every expression) or ceil(n_exprs / 32) host uint32 words; row_idx: None, or int64 [n]: the row of document d
        (the doc_idx of a select or a route of the processed batch).  Returns device tensors (span_off int64 [n + 1], start, len,
        term int32 [total]): document d's spans are span_off[d]:span_off[d + 1], start relative to the document.  The call runs
        twice: count only, then into tensors of exactly that size"""
        flags = _lib.GFT_FOLD_ASCII if fold else 0
        return hit_spans_tensor(lambda t, o, n, *a: self._check(self._L.gft_hit_spans_device(self._h, t, o, n, flags, *a)), text, doc_off, bitmap,
                                self.n_exprs, want, row_idx)

    def redact_spans_device(self, text, doc_off, span_off, start, length, mask=b"*"):
        """overwrites, in place, the bytes of every span with the mask byte (gft_redact_spans_device); every other byte of `text`
        keeps its value.  span_off, start, length: what hit_spans_device returned for (text, doc_off)"""
        redact_spans_tensor(lambda *a: self._check(self._L.gft_redact_spans_device(self._h, *a)), text, doc_off, span_off, start, length, mask)

    def map_spans_to_source_device(self, text, doc_off, span_off, start, length):
        """rewrites, in place, spans of the LOWER-CASE form of a resident batch -- what hit_spans_device gave for the output of
        to_lower_device over (text, doc_off) -- to spans of the batch itself (gft_map_spans_to_source_device).  text, doc_off: the
        SOURCE batch; the lowered text is not needed.  A span that begins or ends inside a rune's lower-case form covers the whole
        source rune"""
        map_spans_to_source_tensor(lambda *a: self._check(self._L.gft_map_spans_to_source_device(self._h, *a)), text, doc_off, span_off, start,
                                   length)

    def excerpt_spans_device(self, text, doc_off, span_off, start, length, before=40, after=40, runes=True, snap=None, reach=64):
        """the text around the hit spans, cut and gathered on the device (gft_excerpt_spans_device).  text, doc_off: the batch the
        spans index; span_off, start, length: what hit_spans_device returned for it (or map_spans_to_source_device rewrote).  The
        window of a span reaches `before` bytes in front of it and `after` behind it, clipped to its document; runes: widened so that
        it cuts no UTF-8 sequence; windows that overlap or touch are one excerpt.  Returns device tensors (out uint8 [total] -- the
        excerpts back to back, a view with 64 zero bytes behind it --, exc_off int64 [m + 1], exc_doc int64 [m], exc_start int32 [m],
        exc_span_off int64 [m + 1], span_rel int32 [spans], doc_exc_off int64 [n + 1]); (out, exc_off, exc_span_off, span_rel,
        length) is what redact_spans_device takes.  The call runs twice: count only, then into tensors of exactly those sizes.
        snap="words": every window then grows to the borders of the words its edges cut (the whole-word rule's word class; implies
        runes); snap="lines": to the line borders round it, the newlines outside -- with before = after = 0 the lines the hits stand
        in.  An edge moves `reach` bytes at most (up to EXCERPT_REACH_MAX) and stays where it was when its word or line is longer
        (gft_excerpt_spans_snap_device).  snap=None is the plain call"""
        if snap is None:
            return excerpt_spans_tensor(lambda *a: self._check(self._L.gft_excerpt_spans_device(self._h, *a)), text, doc_off, span_off, start,
                                        length, before, after, runes)
        return excerpt_spans_tensor(lambda *a: self._check(self._L.gft_excerpt_spans_snap_device(self._h, *a)), text, doc_off, span_off, start,
                                    length, before, after, runes, snap, reach)

    @staticmethod
    def excerpt_spans_host(blob, doc_off, span_off, start, length, before=40, after=40, runes=True, snap=None, reach=64):
        """the host twin of excerpt_spans_device over numpy arrays (gft_debug_excerpt_spans, with snap gft_debug_excerpt_spans_snap):
        the same tuple, as numpy arrays"""
        r = excerpt_spans_host(blob, doc_off, span_off, start, length, before, after, runes, snap=snap, reach=reach)
        m, total = r["n_exc"], r["total"]
        return (r["out"][:total] if r["out"] is not None else np.zeros(0, dtype=np.uint8), r["exc_off"][:m + 1],
                r["exc_doc"][:m] if m else np.zeros(0, dtype=np.uint64), r["exc_start"][:m] if m else np.zeros(0, dtype=np.uint32),
                r["exc_span_off"][:m + 1], r["span_rel"] if r["span_rel"] is not None else np.zeros(0, dtype=np.uint32), r["doc_exc_off"])

    def mark_spans_device(self, text, doc_off, span_off, start, length, open=b"<em>", close=b"</em>"):
        """the batch's text with `open` in front of every hit and `close` behind it, written on the device (gft_mark_spans_device).
        text, doc_off: the batch the spans index; span_off, start, length: what hit_spans_device returned for it,
        map_spans_to_source_device rewrote, or excerpt_spans_device handed back as (exc_span_off, span_rel, length) for its blob.
        Spans that overlap or touch share one pair of markers.  Returns device tensors (out uint8 [total] -- the marked documents
        back to back, a view with 64 zero bytes behind it --, out_off int64 [n + 1], span_new int32 [spans] -- every span's start in
        its marked document --, doc_run_off int64 [n + 1]); (out, out_off, span_off, span_new, length) is what redact_spans_device,
        excerpt_spans_device and this call take.  The call runs twice: count only, then into tensors of exactly those sizes"""
        return mark_spans_tensor(lambda *a: self._check(self._L.gft_mark_spans_device(self._h, *a)), text, doc_off, span_off, start, length,
                                 open, close)

    @staticmethod
    def mark_spans_tensor(call, text, doc_off, span_off, start, length, open=b"<em>", close=b"</em>"):
        """the module's mark_spans_tensor: the count call and the fill call round any gft_mark_spans_device-shaped `call`"""
        return mark_spans_tensor(call, text, doc_off, span_off, start, length, open, close)

    @staticmethod
    def mark_spans_host(blob, doc_off, span_off, start, length, open=b"<em>", close=b"</em>"):
        """the host twin of mark_spans_device over numpy arrays (gft_debug_mark_spans): the same tuple, as numpy arrays"""
        r = mark_spans_host(blob, doc_off, span_off, start, length, open, close)
        return (r["out"][:r["total"]] if r["out"] is not None else np.zeros(0, dtype=np.uint8), r["out_off"],
                r["span_new"] if r["span_new"] is not None else np.zeros(0, dtype=np.uint32), r["doc_run_off"])

    @staticmethod
    def mark_shape():
        """(tile_spans, trip_tiles, chunk_bytes, tile_bytes) of the highlight's walk (gft_debug_mark_shape)"""
        return mark_shape()

    # -- every hit run rewritten by its replacement (csrc/gft_replace.hip) -------------------------------------------------------
    def replace_spans_device(self, text, doc_off, span_off, start, length, reps=b"[REDACTED]", key=None, key_rep=None):
        """the batch's text with every run of hits replaced, written on the device (gft_replace_spans_device).  text, doc_off: the
        batch the spans index; span_off, start, length: what hit_spans_device returned for it, map_spans_to_source_device rewrote, or
        the excerpt, the mark or this call handed back for its own blob.  reps: one bytes object or a list of them, the table -- 0 ..
        255 bytes each, b"" deletes; key: an int32 device tensor parallel to start (hit_spans_device's term ids, say), None: every
        span asks for table entry 0; key_rep: a host array key -> table entry, None: the key is the entry.  A run of spans that
        overlap or touch gets the smallest entry its spans ask for.  Returns device tensors (out uint8 [total] -- the replaced
        documents back to back, a view with 64 zero bytes behind it --, out_off int64 [n + 1], doc_run_off int64 [n + 1], run_new,
        run_len, run_rep int32 [runs]); (out, out_off, doc_run_off, run_new, run_len) is what redact_spans_device,
        excerpt_spans_device, mark_spans_device and this call take.  The call runs twice: count only, then into tensors of exactly
        those sizes"""
        return replace_spans_tensor(lambda *a: self._check(self._L.gft_replace_spans_device(self._h, *a)), text, doc_off, span_off, start, length,
                                    reps, key, key_rep)

    @staticmethod
    def replace_spans_tensor(call, text, doc_off, span_off, start, length, reps=b"[REDACTED]", key=None, key_rep=None):
        """the module's replace_spans_tensor: the count call and the fill call round any gft_replace_spans_device-shaped `call`"""
        return replace_spans_tensor(call, text, doc_off, span_off, start, length, reps, key, key_rep)

    @staticmethod
    def replace_spans_host(blob, doc_off, span_off, start, length, reps=b"[REDACTED]", key=None, key_rep=None):
        """the host twin of replace_spans_device over numpy arrays (gft_debug_replace_spans): the same tuple, as numpy arrays"""
        r = replace_spans_host(blob, doc_off, span_off, start, length, reps, key, key_rep)
        z = np.zeros(0, dtype=np.uint32)
        return (r["out"][:r["total"]] if r["out"] is not None else np.zeros(0, dtype=np.uint8), r["out_off"], r["doc_run_off"],
                r["run_new"] if r["run_new"] is not None else z, r["run_len"] if r["run_len"] is not None else z,
                r["run_rep"] if r["run_rep"] is not None else z)

    @staticmethod
    def replace_shape():
        """(tile_spans, trip_tiles, chunk_bytes, tile_bytes, window, lds_table) of the replacement's walk (gft_debug_replace_shape)"""
        return replace_shape()

    # -- term statistics and column counts (csrc/gft_stats.hip) ----------------------------------------------------------------
    def term_stats_raw(self, d_off_ptr, d_term_ptr, n_docs, n_terms, flags, doc_base, d_occ_ptr, d_docs_ptr, d_first_ptr):
        """gft_term_stats_device on device pointers as they are (None: NULL); the caller has drained the streams that wrote them"""
        self._check(self._L.gft_term_stats_device(self._h, d_off_ptr, d_term_ptr, n_docs, n_terms, int(flags), int(doc_base), d_occ_ptr,
                                                  d_docs_ptr, d_first_ptr))

    def term_stats_device(self, off, term, n_docs, n_terms, occ=None, docs=None, first=None, accumulate=False, doc_base=0):
        """how often each term occurs in a term CSR on the device, in how many documents, and in which first
        (gft_term_stats_device).  off: int64 [n_docs + 1] (off[0] may be non-zero); term: int32, indexed by off's values -- the
        (match_off, term_id) of scan_device or the (span_off, term) of hit_spans_device, as tensors or as device pointers (int).
        occ, docs, first: int64 [n_terms] device tensors; what is not given is allocated (first reads -1, that is UINT64_MAX, where a
        term did not occur).  accumulate: add to what the given tensors hold, first becoming the minimum; doc_base: the documents in
        front of this batch.  Returns (occ, docs, first); only they would have to come down"""
        import torch
        given = [a for a in (off, occ, docs, first) if hasattr(a, "device")]
        dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
        occ, docs = (torch.zeros(n_terms, dtype=torch.int64, device=dev) if a is None else a for a in (occ, docs))
        first = torch.full((n_terms,), -1, dtype=torch.int64, device=dev) if first is None else first
        for a in (occ, docs, first):
            assert a.dtype == torch.int64 and a.numel() == n_terms and a.is_contiguous()
        torch.cuda.current_stream(dev).synchronize()
        ptr = lambda a: (a if isinstance(a, int) or a is None else (a.data_ptr() if a.numel() else None))  # noqa: E731
        self.term_stats_raw(ptr(off), ptr(term), n_docs, n_terms, _lib.GFT_STATS_ACCUMULATE if accumulate else 0, doc_base,
                            *(a.data_ptr() if n_terms else None for a in (occ, docs, first)))
        return occ, docs, first

    def count_columns_device(self, bitmap, n_cols, row_idx=None, count=None, accumulate=False):
        """in how many rows each column of a hit bitmap is set (gft_count_columns_device).  bitmap: int32 [n, ceil(n_cols / 32)] on the
        device, as process_device leaves it (bits at and above n_cols are ignored); row_idx: None, or int64 [m]: the rows to count,
        repeats counting repeatedly (the doc_idx of a routed bucket); count: int64 [n_cols], allocated when not given; accumulate:
        add to it.  Returns count"""
        import torch
        dev = bitmap.device
        n_rows = int(row_idx.numel()) if row_idx is not None else (int(bitmap.shape[0]) if bitmap.dim() == 2 else 0)
        if count is None:
            count = torch.zeros(n_cols, dtype=torch.int64, device=dev)
        assert count.dtype == torch.int64 and count.numel() == n_cols
        torch.cuda.current_stream(dev).synchronize()
        self._check(self._L.gft_count_columns_device(self._h, bitmap.data_ptr() if bitmap.numel() else None, n_rows, n_cols,
                                                     row_idx.data_ptr() if row_idx is not None and row_idx.numel() else None,
                                                     _lib.GFT_STATS_ACCUMULATE if accumulate else 0, count.data_ptr() if n_cols else None))
        return count

    @staticmethod
    def term_stats_host(off, term, n_terms, accumulate_into=None, doc_base=0):
        """the host twin of term_stats_device over numpy arrays (gft_debug_term_stats) -> (occ, docs, first) uint64"""
        if accumulate_into is None:
            occ, docs, first = (np.zeros(n_terms, dtype=np.uint64) for _ in range(3))
        else:
            occ, docs, first = accumulate_into
        term_stats_host(off, term, n_terms, occ, docs, first, _lib.GFT_STATS_ACCUMULATE if accumulate_into is not None else 0, doc_base)
        return occ, docs, first

    @staticmethod
    def count_columns_host(bitmap, n_cols, row_idx=None):
        """the host twin of count_columns_device over numpy arrays (gft_debug_count_columns) -> count uint64 [n_cols]"""
        bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
        n_rows = len(row_idx) if row_idx is not None else (bm.shape[0] if bm.ndim == 2 else 0)
        count = np.zeros(n_cols, dtype=np.uint64)
        count_columns_host(bm, n_rows, n_cols, count, row_idx)
        return count

    @staticmethod
    def stats_shape():
        """the borders of the statistics' walk (gft_debug_stats_shape) as a dict"""
        return stats_shape()

    # -- scores, the top list, documents by index list (csrc/gft_rank.hip) -------------------------------------------------------
    def score_docs_raw(self, d_off_ptr, d_term_ptr, n_docs, n_terms, weights, flags, d_score_ptr):
        """gft_score_docs_device on device pointers as they are (None: NULL); weights: a host uint32 array or None -> max_score; the
        caller has drained the streams that wrote the list"""
        mx = C.c_uint64(0)
        self._check(self._L.gft_score_docs_device(self._h, d_off_ptr, d_term_ptr, n_docs, n_terms, _p(weights), int(flags), d_score_ptr, C.byref(mx)))
        return int(mx.value)

    def score_docs_device(self, off, term, n_docs, n_terms, weights=None, distinct=False, score=None):
        """a score per document of a term CSR on the device (gft_score_docs_device): the sum of weights[t] over a document's entries,
        with distinct over its distinct terms.  off, term as term_stats_device takes them (tensors or device pointers); weights: a host
        array of n_terms uint32, None: every term 1; score: an int64 [n_docs] device tensor, allocated when not given.  Returns
        (score, max_score)"""
        import torch
        given = [a for a in (off, term, score) if hasattr(a, "device")]
        dev = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
        score = torch.zeros(n_docs, dtype=torch.int64, device=dev) if score is None else score
        assert score.dtype == torch.int64 and score.numel() == n_docs and score.is_contiguous()
        w = np.ascontiguousarray(weights, dtype=np.uint32) if weights is not None else None
        assert w is None or w.size == n_terms
        torch.cuda.current_stream(dev).synchronize()
        ptr = lambda a: (a if isinstance(a, int) or a is None else (a.data_ptr() if a.numel() else None))  # noqa: E731
        mx = self.score_docs_raw(ptr(off), ptr(term), n_docs, n_terms, w if w is not None and w.size else None,
                                 _lib.GFT_SCORE_DISTINCT if distinct else 0, ptr(score))
        return score, mx

    def top_docs_raw(self, d_score_ptr, n_docs, k, doc_base, d_top_idx_ptr, d_top_score_ptr):
        """gft_top_docs_device on device pointers as they are -> n_top"""
        n = C.c_uint64(0)
        self._check(self._L.gft_top_docs_device(self._h, d_score_ptr, n_docs, int(k), int(doc_base), d_top_idx_ptr, d_top_score_ptr, C.byref(n)))
        return int(n.value)

    def top_docs_device(self, score, k=10, doc_base=0):
        """the k best documents of an int64 device tensor read as uint64 (gft_top_docs_device): larger score first, among equals the
        smaller index first, no document of score 0.  Returns (top_idx, top_score): int64 device tensors of n_top entries"""
        import torch
        assert score.dtype == torch.int64 and score.is_contiguous()
        idx, val = (torch.empty(max(k, 1), dtype=torch.int64, device=score.device) for _ in range(2))
        torch.cuda.current_stream(score.device).synchronize()
        n = self.top_docs_raw(score.data_ptr() if score.numel() else None, int(score.numel()), k, doc_base, idx.data_ptr(), val.data_ptr())
        return idx[:n], val[:n]

    def gather_docs_raw(self, *args):
        """gft_gather_docs_device on device pointers as they are: (d_text, d_doc_off, n_docs, d_idx, m, idx_base, d_out, cap_bytes,
        d_out_off) -> total_bytes"""
        total = C.c_uint64(0)
        self._check(self._L.gft_gather_docs_device(self._h, *args, C.byref(total)))
        return int(total.value)

    def gather_docs_device(self, text, doc_off, idx, idx_base=0):
        """the documents idx names, in idx's order, repeats allowed, as one blob on the device (gft_gather_docs_device).  text: uint8
        with 64 bytes of slack; doc_off, idx: int64 device tensors.  Returns (out uint8 [total] -- a view with 64 zero bytes behind
        it --, out_off int64 [m + 1]).  Two calls: count only, then into a tensor of exactly the size counted"""
        import torch
        n_docs, m = int(doc_off.numel()) - 1, int(idx.numel())
        out_off = torch.empty(m + 1, dtype=torch.int64, device=text.device)
        torch.cuda.current_stream(text.device).synchronize()
        head = (text.data_ptr(), doc_off.data_ptr(), n_docs, idx.data_ptr() if m else None, m, int(idx_base))
        total = self.gather_docs_raw(*head, None, 0, out_off.data_ptr())
        buf = torch.zeros(total + 64, dtype=torch.uint8, device=text.device)
        torch.cuda.current_stream(text.device).synchronize()
        self.gather_docs_raw(*head, buf.data_ptr(), total, out_off.data_ptr())
        return buf[:total], out_off

    @staticmethod
    def score_docs_host(off, term, n_terms, weights=None, distinct=False):
        """the host twin of score_docs_device over numpy arrays (gft_debug_score_docs) -> (score uint64 [n_docs], max_score)"""
        return score_docs_host(off, term, n_terms, weights, distinct)

    @staticmethod
    def top_docs_host(score, k=10, doc_base=0):
        """the host twin of top_docs_device (gft_debug_top_docs) -> (top_idx, top_score) uint64 [n_top]"""
        return top_docs_host(score, k, doc_base)

    @staticmethod
    def gather_docs_host(blob, doc_off, idx, idx_base=0):
        """the host twin of gather_docs_device (gft_debug_gather_docs) -> (out uint8 [total], out_off uint64 [m + 1])"""
        total, out, out_off = gather_docs_host(blob, doc_off, idx, idx_base)
        return out[:total], out_off

    @staticmethod
    def rank_shape():
        """the borders of the ranking's walks (gft_debug_rank_shape) as a dict"""
        return rank_shape()

    # -- whole-word matching (csrc/gft_words.hip) ---------------------------------------------------------------------------------
    def filter_word_matches_device(self, text, doc_off, off, pos, length=None, term=None, term_len=None, pos_end=False):
        """a match or span list filtered at word borders on the device (gft_filter_word_matches_device).  text: torch.uint8; doc_off,
        off: int64 [n + 1] (off[0] may be non-zero); pos, length, term: int32 indexed by off's values -- (match_off, pos, None,
        term_id) of scan_device with term_len = the dictionary's lengths (int32 [n_terms]), or (span_off, start, len, term) of
        hit_spans_device.  pos_end: pos is the occurrence's last byte.  Returns device tensors (out_off int64 [n + 1], pos, len int32
        [total], term int32 [total] or None): the kept entries in the order given.  Counts first, then fills"""
        return filter_word_matches_tensor(lambda *a: self._check(self._L.gft_filter_word_matches_device(self._h, *a)), text, doc_off, off, pos,
                                          length, term, term_len, pos_end)

    def filter_word_matches_raw(self, *args):
        """gft_filter_word_matches_device on device pointers as they are (None: NULL), behind the handle: (d_text, d_doc_off, n_docs,
        d_off, d_pos, d_len, d_term, d_term_len, n_terms, flags, d_out_off, d_out_pos, d_out_len, d_out_term, cap) -> total"""
        total = C.c_uint64(0)
        self._check(self._L.gft_filter_word_matches_device(self._h, *args, C.byref(total)))
        return int(total.value)

    @staticmethod
    def filter_word_matches_host(blob, doc_off, off, pos, length=None, term=None, term_len=None, pos_end=False):
        """the host twin of filter_word_matches_device over numpy arrays (gft_debug_filter_word_matches) -> (out_off uint64 [n + 1],
        pos, len uint32 [total], term uint32 [total] or None)"""
        total, oo, p, ln, tm = filter_word_matches_host(blob, doc_off, off, pos, length, term, term_len, pos_end)
        return oo, p[:total], ln[:total], (tm[:total] if tm is not None else None)

    @staticmethod
    def words_shape():
        """the borders of the word filter's walk (gft_debug_words_shape) as a dict"""
        return words_shape()

    def scan_words_device(self, d_text_ptr, d_doc_off_ptr, n_docs, fold=False):
        """scan_device followed by the word filter: device pointers in -> GftMatches with DEVICE pointers to the whole-word matches
        (valid until the next call)"""
        m = GftMatches()
        self._check(self._L.gft_scan_words_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, _lib.GFT_FOLD_ASCII if fold else 0, C.byref(m)))
        return m

    def process_words_device(self, d_text_ptr, d_doc_off_ptr, n_docs, d_bitmap_ptr, fold=False):
        """process_device from the whole-word matches alone (gft_process_words_device)"""
        self._check(self._L.gft_process_words_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, _lib.GFT_FOLD_ASCII if fold else 0, d_bitmap_ptr))

    def process_words(self, blob, doc_off, fold=False):
        """host numpy in -> uint32 bitmap [n_docs, ceil(E/32)] from the whole-word matches alone (gft_process_words)"""
        n_docs = len(doc_off) - 1
        bm = np.zeros((n_docs, (self.n_exprs + 31) // 32), dtype=np.uint32)
        self._check(self._L.gft_process_words(self._h, _p(blob), _p(doc_off), n_docs, _lib.GFT_FOLD_ASCII if fold else 0, _p(bm) if bm.size else None))
        return bm

    def hit_spans_words_device(self, text, doc_off, bitmap, want=None, row_idx=None, fold=False):
        """hit_spans_device with the whole-word rule (gft_hit_spans_words_device): same arguments, same result, only the spans that
        stand at word borders"""
        flags = _lib.GFT_FOLD_ASCII if fold else 0
        return hit_spans_tensor(lambda t, o, n, *a: self._check(self._L.gft_hit_spans_words_device(self._h, t, o, n, flags, *a)), text, doc_off,
                                bitmap, self.n_exprs, want, row_idx)

    def process_sparse(self, blob, doc_off, fold=False, extra=None):
        """host numpy in -> (row_off u64 [n_docs + 1], expr_idx u32, label u32 or None) (gft_process_sparse)"""
        n_docs = len(doc_off) - 1
        x = None
        if extra is not None:
            eo, es, ep = extra
            x = GftExtra(eo.ctypes.data, es.ctypes.data, ep.ctypes.data)
        sp = GftSparse()
        self._check(self._L.gft_process_sparse(self._h, _p(blob), _p(doc_off), n_docs, 1 if fold else 0,
                                               C.byref(x) if x is not None else None, C.byref(sp)))
        return _sparse_arrays(sp.row_off, sp.expr_idx, sp.label, n_docs)

    # -- measurement ------------------------------------------------------------------------------------
    def profile(self, on=True):
        self._check(self._L.gft_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._check(self._L.gft_profile_reset(self._h))

    def profile_read(self, name):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self._L.gft_profile_read(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)


def _sparse_arrays(row_off_ptr, expr_idx_ptr, label_ptr, n_docs):
    """copies of a library-owned CSR result"""
    ro = np.ctypeslib.as_array(C.cast(row_off_ptr, C.POINTER(C.c_uint64)), shape=(n_docs + 1,)).copy()
    total = int(ro[n_docs])
    if total == 0:
        return ro, np.zeros(0, np.uint32), (np.zeros(0, np.uint32) if label_ptr else None)
    ei = np.ctypeslib.as_array(C.cast(expr_idx_ptr, C.POINTER(C.c_uint32)), shape=(total,)).copy()
    lb = np.ctypeslib.as_array(C.cast(label_ptr, C.POINTER(C.c_uint32)), shape=(total,)).copy() if label_ptr else None
    return ro, ei, lb


def compact_host(bitmap, n_exprs, labels=None, cap=None):
    """gft_debug_compact_host: bitmap [n_docs, ceil(n_exprs / 32)] (host) -> (row_off, expr_idx, label or None, total).
    cap=None: buffers of the size the result needs (two calls); otherwise the first min(total, cap) entries"""
    L = _lib.load()
    bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
    n_docs = bm.shape[0]
    lab = np.ascontiguousarray(labels, dtype=np.uint32) if labels is not None else None
    ro = np.zeros(n_docs + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    if cap is None:
        rc = L.gft_debug_compact_host(_p(bm) if bm.size else None, n_docs, n_exprs, _p(lab), _p(ro), None, None, 0, C.byref(total))
        if rc != 0:
            raise GftError(rc, "gft_debug_compact_host failed")
        cap = int(total.value)
    ei = np.zeros(max(cap, 1), dtype=np.uint32)
    lb = np.zeros(max(cap, 1), dtype=np.uint32) if lab is not None else None
    rc = L.gft_debug_compact_host(_p(bm) if bm.size else None, n_docs, n_exprs, _p(lab), _p(ro), _p(ei), _p(lb), cap, C.byref(total))
    if rc != 0:
        raise GftError(rc, "gft_debug_compact_host failed")
    n = min(cap, int(total.value))
    return ro, ei[:n], (lb[:n] if lb is not None else None), int(total.value)
