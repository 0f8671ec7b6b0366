"""Python mirror of the reference's finder package (finder/finder.go, substringEngine.go, regexEngine.go) over
libgft.so's gft_finder_* C ABI.  Same names and error behaviour; Go `error` values surface as FinderError whose
text is the reference's message (parser errors, injected-engine errors) or the library's (GPU errors).

All scanning and solving happens on the GPU inside libgft.so; this module only marshals arguments.
"""
import ctypes as C
import json
import re

import numpy as np

from . import _lib
from .engine import Engine, GftError, _sparse_arrays, pack


class FinderError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Match:
    """finder.Match (finder/finder.go:11-14)"""
    __slots__ = ("Position", "Term")

    def __init__(self, Position, Term):
        self.Position, self.Term = Position, Term

    def __eq__(self, o):
        return (self.Position, self.Term) == (o.Position, o.Term)

    def __repr__(self):
        return "Match(%d, %r)" % (self.Position, self.Term)


class ExpressionResult:
    """finder.ExpressionResult (finder/finder.go:25-29; field names as in the reference)"""
    __slots__ = ("ExpresionIndex", "ExpresionStr", "Tag")

    def __init__(self, ExpresionIndex, ExpresionStr, Tag):
        self.ExpresionIndex, self.ExpresionStr, self.Tag = ExpresionIndex, ExpresionStr, Tag

    def to_obj(self):
        return {"ExpresionIndex": self.ExpresionIndex, "ExpresionStr": self.ExpresionStr, "Tag": self.Tag}

    def __repr__(self):
        return "ExpressionResult(%r)" % (self.to_obj(),)


class SubstringEngine:
    """finder.SubstringEngine (finder/substringEngine.go:11-18): raise an Exception to return a Go error."""

    def BuildEngine(self, keywords, caseSensitive):
        raise NotImplementedError

    def FindSubstrings(self, text):
        raise NotImplementedError


class RegexEngine:
    """finder.RegexEngine (finder/regexEngine.go:8-15)"""

    def BuildEngine(self, regexes, caseSensitive):
        raise NotImplementedError

    def FindRegexes(self, text):
        raise NotImplementedError


class EmptyEngine(SubstringEngine):
    def BuildEngine(self, keywords, caseSensitive):
        return None

    def FindSubstrings(self, text):
        return []


class EmptyRgxEngine(RegexEngine):
    def BuildEngine(self, regexes, caseSensitive):
        return None

    def FindRegexes(self, text):
        return []


class GpuEngine(SubstringEngine):
    """Drop-in for finder.CloudflareForkEngine backed by the HIP kernels (one gft_engine)."""

    def __init__(self, device=-1):
        self.engine = Engine(device)

    def BuildEngine(self, keywords, caseSensitive):
        try:
            self.engine.build(sorted(keywords))
        except GftError as e:
            raise FinderError(e.code, e.msg)

    def FindSubstrings(self, text):
        b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        blob, off = pack([b])
        mo, ti, po = self.engine.scan(blob, off)
        terms = {}
        out = []
        for t, p in zip(ti.tolist(), po.tolist()):
            if t not in terms:
                terms[t] = self.engine.term(t).decode("utf-8", "surrogateescape")
            out.append(Match(p, terms[t]))
        return out


class PyRegexpEngine(RegexEngine):
    """Host-side stand-in for finder.RegexpEngine (finder/regexEngine.go:17-47): Python `re` instead of Go
    `regexp`; Position = byte offset of the start of each non-overlapping leftmost match, Term = regex source."""

    def __init__(self):
        self.compiled = []

    def BuildEngine(self, regexes, caseSensitive):
        self.compiled = [(r, re.compile(r.encode("utf-8") if isinstance(r, str) else r)) for r in regexes]

    def FindRegexes(self, text):
        b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        out = []
        for src, rx in self.compiled:
            for m in rx.finditer(b):
                out.append(Match(m.start(), src))
        return out


def _mk_build(obj):
    def cb(user, blob, off, n, cs, err, cap):
        try:
            offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), shape=(n + 1,))
            raw = C.string_at(blob, int(offs[n])) if n else b""
            items = [raw[int(offs[i]):int(offs[i + 1])].decode("utf-8", "surrogateescape") for i in range(n)]
            obj.BuildEngine(items, bool(cs))
            return 0
        except Exception as e:   # Go: return err
            msg = str(e).encode("utf-8")[:cap - 1] + b"\0"
            C.memmove(err, msg, len(msg))
            return 1
    return _lib.BUILD_FN(cb)


def _mk_find(obj, method):
    def cb(user, text, n, emit, sink, err, cap):
        try:
            t = C.string_at(text, n).decode("utf-8", "surrogateescape")
            for m in getattr(obj, method)(t) or []:
                term = m.Term.encode("utf-8", "surrogateescape") if isinstance(m.Term, str) else bytes(m.Term)
                emit(sink, term, len(term), int(m.Position))
            return 0
        except Exception as e:
            msg = str(e).encode("utf-8")[:cap - 1] + b"\0"
            C.memmove(err, msg, len(msg))
            return 1
    return _lib.FIND_FN(cb)


class Finder:
    """finder.Finder (finder/finder.go:32-240).  NewFinder(subEng, rgxEng, caseSensitive)."""

    def __init__(self, subEng=None, rgxEng=None, caseSensitive=True, device=-1, allow_no_device=False, devices=None, whole_words=False):
        """allow_no_device: keep the handle when no HIP device exists, so the host-only half (expression
        registry, parser, engine-build orchestration) can be exercised; every GPU step then fails with GFT_E_HIP.
        whole_words: a keyword occurrence counts only where it stands at word borders (gft_finder_set_whole_words): `he` no longer
        fires inside `ushers`.  Every Process*, Select*, Route*, Count*, Spans*, Redact*, Excerpt*, Highlight*, TermStats* and Top* call of
        this finder then answers from those occurrences; needs the GPU substring engine on one device and no regex terms."""
        self._L = _lib.load()
        h = C.c_void_p()
        if devices is not None:        # one finder over several devices (gft_finder_create_multi)
            arr = (C.c_int * len(devices))(*devices)
            rc = self._L.gft_finder_create_multi(C.byref(h), 1 if caseSensitive else 0, C.cast(arr, C.c_void_p), len(devices))
        else:
            rc = self._L.gft_finder_create(C.byref(h), 1 if caseSensitive else 0, device)
        self._h = h
        if rc != 0 and not (allow_no_device and rc == _lib.GFT_E_HIP and h):
            msg = self._L.gft_finder_last_error(h).decode() if h else "gft_finder_create failed"
            self.close()
            raise FinderError(rc, msg)
        self.caseSensitive = caseSensitive
        self._device = device if devices is None else devices[0]
        self._keep = []
        if subEng is not None and not isinstance(subEng, GpuEngine):
            b, f = _mk_build(subEng), _mk_find(subEng, "FindSubstrings")
            self._keep += [b, f, subEng]
            self._check(self._L.gft_finder_set_substring_engine(self._h, C.cast(b, C.c_void_p), C.cast(f, C.c_void_p), None))
        if rgxEng is not None and not isinstance(rgxEng, EmptyRgxEngine):
            b, f = _mk_build(rgxEng), _mk_find(rgxEng, "FindRegexes")
            self._keep += [b, f, rgxEng]
            self._check(self._L.gft_finder_set_regex_engine(self._h, C.cast(b, C.c_void_p), C.cast(f, C.c_void_p), None))
        if whole_words:
            self._check(self._L.gft_finder_set_whole_words(self._h, 1))

    @property
    def whole_words(self):
        return bool(self._L.gft_finder_whole_words(self._h))

    @whole_words.setter
    def whole_words(self, on):
        self._check(self._L.gft_finder_set_whole_words(self._h, 1 if on else 0))

    def close(self):
        if getattr(self, "_h", None):
            self._L.gft_finder_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise FinderError(rc, self._L.gft_finder_last_error(self._h).decode("utf-8", "replace"))

    # -- registry -------------------------------------------------------------------------------------
    def AddExpression(self, expression):
        return self.AddExpressionWithTag(expression, "")

    def AddExpressions(self, expressions):
        for e in expressions:
            self.AddExpressionWithTag(e, "")

    def AddExpressionsWithTag(self, expressions, tag):
        for e in expressions:
            self.AddExpressionWithTag(e, tag)

    def AddExpressionWithTag(self, expression, tag):
        e = expression.encode("utf-8") if isinstance(expression, str) else bytes(expression)
        t = tag.encode("utf-8") if isinstance(tag, str) else bytes(tag)
        self._check(self._L.gft_finder_add_expression(self._h, e, len(e), t, len(t)))

    def _literals(self, which):
        out = []
        p, n = C.c_void_p(), C.c_uint32()
        for i in range(self._L.gft_finder_n_literals(self._h, which)):
            self._check(self._L.gft_finder_literal(self._h, which, i, C.byref(p), C.byref(n)))
            out.append(C.string_at(p, n.value).decode("utf-8", "surrogateescape"))
        return out

    def GetKeywords(self):
        return set(self._literals(0))

    def GetRegexes(self):
        return set(self._literals(1))

    @property
    def n_expressions(self):
        return self._L.gft_finder_n_expressions(self._h)

    def expression(self, i, tree=True):
        """-> (exprString, tag, tree as dict); tree=False: source and tag only (the reference's own benchmarks build chains
        of 10 000 leaves, benchmarks/benchmark_test.go:56 -- a tree that deep is not something json.loads should recurse into)"""
        ptrs = [C.c_void_p() for _ in range(3)]
        lens = [C.c_uint32() for _ in range(3)]
        self._check(self._L.gft_finder_expression(self._h, i, C.byref(ptrs[0]), C.byref(lens[0]), C.byref(ptrs[1]),
                                                  C.byref(lens[1]), C.byref(ptrs[2]) if tree else None,
                                                  C.byref(lens[2]) if tree else None))
        s, t = (C.string_at(p, n.value) for p, n in zip(ptrs[:2], lens[:2]))
        j = json.loads(C.string_at(ptrs[2], lens[2].value).decode("utf-8")) if tree else None
        return s.decode("utf-8", "surrogateescape"), t.decode("utf-8", "surrogateescape"), j

    def tags(self):
        """distinct tags, numbered by first appearance in registration order (the empty tag of AddExpression included):
        tags()[k] is the tag whose id is k in the tag_id arrays"""
        out = []
        p, n = C.c_void_p(), C.c_uint32()
        for i in range(self._L.gft_finder_n_tags(self._h)):
            self._check(self._L.gft_finder_tag(self._h, i, C.byref(p), C.byref(n)))
            out.append(C.string_at(p, n.value).decode("utf-8", "surrogateescape"))
        return out

    def expression_tag_id(self, i):
        return int(self._L.gft_finder_expression_tag_id(self._h, i))

    def _pairs(self):
        cache = self.__dict__.setdefault("_expr_cache", [])      # (source, tag) per registered expression
        while len(cache) < self.n_expressions:
            s, t, _ = self.expression(len(cache), tree=False)
            cache.append((s, t))
        return cache

    # -- processing -----------------------------------------------------------------------------------
    def ForceBuild(self):
        self._check(self._L.gft_finder_force_build(self._h))

    def ProcessText(self, text):
        """-> list of ExpressionResult for the expressions that are true (registration order)"""
        b = text.encode("utf-8", "surrogateescape") if isinstance(text, str) else bytes(text)
        cap = max(self.n_expressions, 1)
        idx = np.zeros(cap, dtype=np.uint32)
        n = C.c_uint32()
        self._check(self._L.gft_finder_process_text(self._h, b, len(b), idx.ctypes.data, cap, C.byref(n)))
        cache = self._pairs()
        return [ExpressionResult(i, cache[i][0], cache[i][1]) for i in idx[:n.value].tolist()]

    def ProcessTexts(self, texts=None, blob=None, doc_off=None, out=None):
        """batch extension -> uint32 bitmap [n_docs, ceil(E/32)]; `out`: a caller's array of that shape to fill instead of a
        fresh one (a Go caller keeps its []uint32 from batch to batch: no page of the result is touched for the first time)"""
        if texts is not None:
            blob, doc_off = pack(texts)
        n_docs = len(doc_off) - 1
        words = (self.n_expressions + 31) // 32
        if out is not None:
            if out.dtype != np.uint32 or out.shape != (n_docs, words) or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a C-contiguous uint32 array of shape (n_docs, ceil(n_expressions / 32))")
            bm = out
        else:
            bm = np.zeros((n_docs, words), dtype=np.uint32)
        self._check(self._L.gft_finder_process_texts(self._h, blob.ctypes.data, doc_off.ctypes.data, n_docs,
                                                     bm.ctypes.data if bm.size else None))
        return bm

    def ProcessTextsSparse(self, texts=None, blob=None, doc_off=None):
        """batch form of ProcessText's result -> (row_off u64 [n_docs + 1], expr_idx u32, tag_id u32): document d's true
        expressions are expr_idx[row_off[d]:row_off[d + 1]] in registration order, tag_id[k] indexes tags().  Where the
        batch's bitmap is complete on the device it is compacted there and only these arrays are downloaded"""
        if texts is not None:
            blob, doc_off = pack(texts)
        n_docs = len(doc_off) - 1
        ro, ei, tg = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.gft_finder_process_texts_sparse(self._h, blob.ctypes.data, doc_off.ctypes.data, n_docs,
                                                            C.byref(ro), C.byref(ei), C.byref(tg)))
        return _sparse_arrays(ro, ei, tg, n_docs)

    def ProcessTextsResults(self, texts=None, blob=None, doc_off=None):
        """-> one list of ExpressionResult per document: what the reference's ProcessText returns for each of them"""
        ro, ei, _ = self.ProcessTextsSparse(texts, blob, doc_off)
        cache = self._pairs()
        ro, ei = ro.tolist(), ei.tolist()
        return [[ExpressionResult(i, cache[i][0], cache[i][1]) for i in ei[ro[d]:ro[d + 1]]] for d in range(len(ro) - 1)]

    def CompactDevice(self, d_bitmap_ptr, n_docs, d_row_off_ptr, d_expr_idx_ptr, d_tag_id_ptr, cap, want_total=True):
        """a device bitmap of ProcessDevice / ProcessDeviceBegin + End -> device CSR (gft_finder_compact_device): row_off
        (n_docs + 1 u64), expr_idx and tag_id (cap u32 each; tag_id may be None).  Entries at positions >= cap are not
        written, row_off is always complete.  want_total=True: waits and returns the total; False: only enqueues (the
        total is in d_row_off[n_docs]) and returns None -- allowed while a younger batch is in flight"""
        total = C.c_uint64(0)
        self._check(self._L.gft_finder_compact_device(self._h, d_bitmap_ptr, n_docs, d_row_off_ptr, d_expr_idx_ptr, d_tag_id_ptr,
                                                      cap, C.byref(total) if want_total else None))
        return int(total.value) if want_total else None

    def ProcessDevice(self, d_text_ptr, d_doc_off_ptr, n_docs, d_bitmap_ptr):
        self._check(self._L.gft_finder_process_device(self._h, d_text_ptr, d_doc_off_ptr, n_docs, d_bitmap_ptr))

    def SplitLinesDevice(self, buf, length, mode=0):
        """Engine.split_lines_device on the finder's engine (gft_finder_split_lines_device): needs what ProcessDevice needs"""
        from .engine import split_lines_tensor
        return split_lines_tensor(lambda *a: self._check(self._L.gft_finder_split_lines_device(self._h, *a)), buf, length, mode)

    def ProcessLinesDevice(self, buf, length):
        """a resident blob of text lines (a torch.uint8 device tensor of at least length + 64 bytes) -> (doc_off int64 [n + 1],
        bitmap int32 [n, ceil(E / 32)]) on the device: the blob is cut behind every newline on the device (SPLIT_AFTER_NL, Go's
        strings.SplitAfter without a final empty piece), then ProcessDevice runs over the result; the rows are those of
        ProcessTexts over the pieces.  Needs what ProcessDevice needs"""
        import torch
        off = self.SplitLinesDevice(buf, length, 0)
        n = int(off.numel()) - 1
        bm = torch.zeros((n, (self.n_expressions + 31) // 32), dtype=torch.int32, device=buf.device)
        torch.cuda.current_stream(buf.device).synchronize()
        self.ProcessDevice(buf.data_ptr(), off.data_ptr(), n, bm.data_ptr() if bm.numel() else None)
        return off, bm

    def ProcessLines(self, data):
        """the host-memory form: bytes -> (doc_off uint64 [n + 1], bitmap uint32 [n, ceil(E / 32)]) as numpy arrays: the blob goes
        up once with 64 bytes of slack, ProcessLinesDevice, offsets and rows come down"""
        import torch
        data = bytes(data)
        dev = torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())
        buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        if data:
            buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        off, bm = self.ProcessLinesDevice(buf, len(data))
        return off.cpu().numpy().astype(np.uint64), bm.cpu().numpy().view(np.uint32)

    # -- the documents that matched (csrc/gft_select.hip) ------------------------------------------------------------------
    def want_mask(self, indices=None, tags=None):
        """the host mask of the select calls: ceil(E / 32) uint32 words with the bits of the expressions named by index and / or
        by tag (every expression registered under one of `tags`).  Both None: every expression.  An index out of range or a tag no
        expression carries is a ValueError"""
        E = self.n_expressions
        w = np.zeros((E + 31) // 32, dtype=np.uint32)
        if indices is None and tags is None:
            indices = range(E)
        picked = []
        for i in indices or ():
            i = int(i)
            if not 0 <= i < E:
                raise ValueError("want_mask: no expression %d" % i)
            picked.append(i)
        if tags is not None:
            names = self.tags()
            ids = set()
            for t in [tags] if isinstance(tags, str) else tags:
                if t not in names:
                    raise ValueError("want_mask: no expression carries the tag %r" % (t,))
                ids.add(names.index(t))
            picked += [i for i in range(E) if self.expression_tag_id(i) in ids]
        for i in picked:
            w[i >> 5] |= np.uint32(1 << (i & 31))
        return w

    def SelectDevice(self, text, doc_off, bitmap, want=None, mode="any", also=None):
        """Engine.select_docs_device on the finder's engine with n_cols = n_expressions (gft_finder_select_docs_device): the
        documents whose rows -- as ProcessDevice left them -- hit `want` (want_mask(); None: any expression), as device tensors
        (out uint8, out_off int64 [m + 1], doc_idx int64 [m]).  Needs what ProcessDevice needs"""
        from .engine import select_docs_tensor

        def call(d_text, d_off, n, d_bm, n_cols, w, m, d_also, *rest):
            self._check(self._L.gft_finder_select_docs_device(self._h, d_text, d_off, n, d_bm, w, m, d_also, *rest))
        return select_docs_tensor(call, text, doc_off, bitmap, self.n_expressions, want, mode, also)

    def SelectLinesDevice(self, buf, length, want=None, mode="any"):
        """a resident blob of text lines -> the lines that hit: ProcessLinesDevice (split behind every newline, ProcessDevice), then
        SelectDevice over its rows.  Returns (out, out_off, doc_idx, doc_off, bitmap), all on the device; a line keeps its newline"""
        off, bm = self.ProcessLinesDevice(buf, length)
        out, out_off, doc_idx = self.SelectDevice(buf, off, bm, want, mode)
        return out, out_off, doc_idx, off, bm

    def SelectLines(self, data, want=None, mode="any"):
        """the host-memory form: bytes -> (the selected lines as bytes, out_off uint64 [m + 1], doc_idx uint64 [m]).  One upload;
        only the selected lines, their offsets and their indices come down.  A finder that does not take the device route (regex
        terms, injected engines, several devices) splits, processes and selects on the host -- the kernels' walk behind
        gft_debug_split_lines and gft_debug_select_docs --: the same result"""
        import torch
        data = bytes(data)
        if self._takes_device_route():
            dev = torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())
            buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
            if data:
                buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            out, out_off, doc_idx, _, _ = self.SelectLinesDevice(buf, len(data), want, mode)
            return out.cpu().numpy().tobytes(), out_off.cpu().numpy().astype(np.uint64), doc_idx.cpu().numpy().astype(np.uint64)
        from .engine import select_docs_host, split_lines_host
        n, off = split_lines_host(data, 0)
        off = off[:n + 1]
        bm = self.ProcessTexts(blob=np.frombuffer(data + b"\0" * 64, dtype=np.uint8), doc_off=off)
        m, total, out, out_off, doc_idx = select_docs_host(data, off, bm, self.n_expressions, want, mode)
        return out[:total].tobytes(), out_off[:m + 1].copy(), doc_idx[:m].copy()

    # -- context lines round the documents that matched (csrc/gft_context.hip) ---------------------------------------------------
    def ContextDevice(self, text, doc_off, bitmap, want=None, mode="any", also=None, before=0, after=0, fence=None):
        """Engine.context_docs_device on the finder's engine with n_cols = n_expressions (gft_finder_context_docs_device): the
        documents SelectDevice selects and up to `before` documents in front of each and `after` behind, as device tensors (out
        uint8, out_off int64 [m + 1], doc_idx int64 [m], kind uint8 [m], group_off int64 [g + 1]).  Needs what ProcessDevice needs"""
        from .engine import context_docs_tensor

        def call(d_text, d_off, n, d_bm, n_cols, w, m, d_also, *rest):
            self._check(self._L.gft_finder_context_docs_device(self._h, d_text, d_off, n, d_bm, w, m, d_also, *rest))
        return context_docs_tensor(call, text, doc_off, bitmap, self.n_expressions, want, mode, also, before, after, fence)

    def ContextLinesDevice(self, buf, length, before=0, after=0, want=None, mode="any"):
        """a resident blob of text lines -> the lines that hit and the lines round them (grep -B before -A after; mode "none": grep -v):
        ProcessLinesDevice, then ContextDevice over its rows.  Returns (out, out_off, doc_idx, kind, group_off, doc_off, bitmap), all
        on the device; a line keeps its newline"""
        off, bm = self.ProcessLinesDevice(buf, length)
        return self.ContextDevice(buf, off, bm, want, mode, None, before, after) + (off, bm)

    def ContextLines(self, data, before=0, after=0, want=None, mode="any"):
        """the host-memory form: bytes -> (the kept lines as bytes, out_off uint64 [m + 1], doc_idx uint64 [m], kind uint8 [m],
        group_off uint64 [g + 1]).  One upload; only the kept lines and their arrays come down.  A finder that does not take the
        device route splits, processes and decides on the host -- the kernels' walk behind gft_debug_split_lines and
        gft_debug_context_docs --: the same result"""
        import torch
        data = bytes(data)
        if self._takes_device_route():
            dev = torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())
            buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
            if data:
                buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
            out, out_off, doc_idx, kind, group_off, _, _ = self.ContextLinesDevice(buf, len(data), before, after, want, mode)
            return (out.cpu().numpy().tobytes(), out_off.cpu().numpy().astype(np.uint64), doc_idx.cpu().numpy().astype(np.uint64),
                    kind.cpu().numpy(), group_off.cpu().numpy().astype(np.uint64))
        from .engine import context_docs_host, split_lines_host
        n, off = split_lines_host(data, 0)
        off = off[:n + 1]
        bm = self.ProcessTexts(blob=np.frombuffer(data + b"\0" * 64, dtype=np.uint8), doc_off=off)
        m, _, g, total, out, out_off, doc_idx, kind, group_off = context_docs_host(data, off, bm, self.n_expressions, want, mode, None, before, after)
        return out[:total].tobytes(), out_off[:m + 1].copy(), doc_idx[:m].copy(), kind[:m].copy(), group_off[:g + 1].copy()

    # -- where the expressions matched (csrc/gft_spans.hip) ----------------------------------------------------------------------
    def SpansDevice(self, text, doc_off, bitmap, want=None, row_idx=None, source=False):
        """Engine.hit_spans_device on the finder's engine under the finder's case rule (gft_finder_hit_spans_device), over the rows
        ProcessDevice left: (span_off int64 [n + 1], start, len, term int32 [total], lowered).  lowered True: the batch left ASCII
        and was lowered on the device before it was scanned -- the spans index the LOWERED text (Engine.to_lower_device over the
        batch gives its bytes and offsets), not the caller's.  source=True (gft_finder_hit_spans_source_device): the spans of such
        a batch are mapped back on the device and always index `text`; lowered still says what happened.  Needs what ProcessDevice
        needs"""
        from .engine import hit_spans_tensor
        lowered = C.c_int(0)
        fn = self._L.gft_finder_hit_spans_source_device if source else self._L.gft_finder_hit_spans_device

        def call(*a):
            self._check(fn(self._h, *a, C.byref(lowered)))
        out = hit_spans_tensor(call, text, doc_off, bitmap, self.n_expressions, want, row_idx)
        return out + (bool(lowered.value),)

    def _spans_of_lines(self, buf, length, want, source=False):
        """split, process and spans of a resident blob of lines: (doc_off, bitmap, spans..., lowered)"""
        if not self._takes_device_route():
            raise FinderError(_lib.GFT_E_UNSUPPORTED, "hit spans need the device route: the GPU substring engine, no regex terms, one device")
        off, bm = self.ProcessLinesDevice(buf, length)
        return (off, bm) + self.SpansDevice(buf, off, bm, want, source=source)

    def _lowered_clone(self, buf, off, lowered):
        """the text the spans index, as a buffer of its own: a copy of the batch, or its lower-case form (gft_to_lower_device)"""
        import torch
        if not lowered:
            return buf.clone(), off
        eng = self.engine_handle()
        n = int(off.numel()) - 1
        total = C.c_uint64(0)
        low_off = torch.empty(n + 1, dtype=torch.int64, device=buf.device)
        torch.cuda.current_stream(buf.device).synchronize()
        self._check_engine(self._L.gft_to_lower_device(eng, buf.data_ptr(), off.data_ptr(), n, None, 0, low_off.data_ptr(), C.byref(total)))
        low = torch.zeros(int(total.value) + 64, dtype=torch.uint8, device=buf.device)
        torch.cuda.current_stream(buf.device).synchronize()
        self._check_engine(self._L.gft_to_lower_device(eng, buf.data_ptr(), off.data_ptr(), n, low.data_ptr(), int(total.value), low_off.data_ptr(),
                                                       C.byref(total)))
        return low, low_off

    def _check_engine(self, rc):
        if rc != 0:
            raise FinderError(rc, self._L.gft_last_error(self.engine_handle()).decode())

    def SpansLines(self, data, want=None, source=False):
        """bytes -> (idx, spans, lowered): idx the numbers of the lines that hit `want` (want_mask(); None: any expression), spans[k]
        the list of (start, end, keyword) of line idx[k] -- every occurrence of a keyword that is a witness of a true, wanted
        expression, in the scan's order, start / end relative to the line; a line that hit through negated keywords alone has an
        empty list.  One upload; only the rows and the spans come down.  lowered True: the batch left ASCII and the positions index
        the lines' lower-case form (strings.ToLower), whose lengths may differ -- unless source=True: the positions then always
        index the caller's lines (a span covers whole source runes; the keyword in the tuple stays the dictionary's lowered one).
        Device route only"""
        data = bytes(data)
        buf = self._resident(data)
        off, bm, span_off, start, length, term, lowered = self._spans_of_lines(buf, len(data), want, source)
        rows = bm.cpu().numpy().view(np.uint32).reshape(int(off.numel()) - 1, -1)
        w = self.want_mask() if want is None else np.ascontiguousarray(want, dtype=np.uint32)
        w = self.want_mask() & w
        hit = np.nonzero((rows & w[None, :]).any(axis=1))[0] if rows.shape[1] else np.zeros(0, dtype=np.int64)
        so, st, ln, tm = (t.cpu().numpy() for t in (span_off, start, length, term))
        terms = {}
        tp, tl = C.c_void_p(), C.c_uint32()
        for t in np.unique(tm).tolist():
            self._check_engine(self._L.gft_term(self.engine_handle(), int(t), C.byref(tp), C.byref(tl)))
            terms[t] = C.string_at(tp.value, tl.value)
        spans = [[(int(st[k]), int(st[k]) + int(ln[k]), terms[int(tm[k])]) for k in range(int(so[d]), int(so[d + 1]))] for d in hit.tolist()]
        return hit.astype(np.uint64), spans, lowered

    def RedactLines(self, data, want=None, mask=b"*", source=False):
        """bytes -> (bytes, lowered): the blob with every keyword occurrence that is a witness of a true, wanted expression
        overwritten by `mask`, byte for byte.  One upload, then split, process, spans and the redaction of a clone on the device,
        one download.  lowered True: the batch left ASCII -- the bytes are the lines' lower-case form (strings.ToLower) with the
        masks in it.  source=True: a clone of the CALLER's blob is redacted with the spans mapped back to it -- the result has
        len(data) bytes and differs from data only inside the source spans, whatever lowered says.  Device route only"""
        from .engine import redact_spans_tensor
        data = bytes(data)
        buf = self._resident(data)
        off, _, span_off, start, length, _, lowered = self._spans_of_lines(buf, len(data), want, source)
        text, text_off = self._lowered_clone(buf, off, lowered and not source)
        redact_spans_tensor(lambda *a: self._check_engine(self._L.gft_redact_spans_device(self.engine_handle(), *a)), text, text_off, span_off,
                            start, length, mask)
        n = int(text_off[-1].item()) if text_off.numel() else 0
        return text[:n].cpu().numpy().tobytes(), lowered

    # -- the text around the hits (csrc/gft_excerpt.hip) ---------------------------------------------------------------------------
    def ExcerptsDevice(self, text, doc_off, span_off, start, length, lowered=False, source=False, before=40, after=40, runes=True, snap=None,
                       reach=64):
        """Engine.excerpt_spans_device on the finder's engine behind SpansDevice (gft_finder_excerpts_device): text, doc_off the
        batch, span_off / start / length and `lowered` what SpansDevice returned for it, source as it was called.  With source, or
        for a batch that was not lowered, the excerpts are cut from `text`; otherwise from the batch's lower-case form, which the
        finder lowers on the device again.  Returns (out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, doc_exc_off, cut_lowered)
        -- device tensors as Engine.excerpt_spans_device gives them, and whether the lowered text was cut.  Needs what ProcessDevice
        needs.  snap="words" | "lines", reach: Engine.excerpt_spans_device's (gft_finder_excerpts_snap_device); the snap judges the
        text the excerpts are cut from"""
        from .engine import excerpt_spans_tensor
        cut = C.c_int(0)
        fn = self._L.gft_finder_excerpts_device if snap is None else self._L.gft_finder_excerpts_snap_device

        def call(d_text, d_off, n, d_so, d_st, d_ln, *rest):
            self._check(fn(self._h, d_text, d_off, n, d_so, d_st, d_ln, 1 if lowered else 0, 1 if source else 0, *rest, C.byref(cut)))
        out = excerpt_spans_tensor(call, text, doc_off, span_off, start, length, before, after, runes, snap, reach)
        return out + (bool(cut.value),)

    def ExcerptLines(self, data, before=40, after=40, want=None, source=True, runes=True, mark=None, snap=None, reach=64):
        """bytes -> (idx, excerpts, lowered): idx the numbers of the lines that hit `want` (want_mask(); None: any expression),
        excerpts[k] the list of (start_in_line, bytes, [(rel_start, rel_end, keyword), ...]) of line idx[k]: the text `before` bytes
        in front of and `after` bytes behind every hit of SpansLines, windows that overlap or touch merged, cut on rune borders
        (runes), with the hits' positions inside the excerpt.  A line that hit through negated keywords alone has no excerpt.  One
        upload; the excerpt blob, its index arrays, the span arrays and the rows come down -- never the lines.  lowered True: the
        batch left ASCII; with source=True (the default) the excerpts are still substrings of the caller's lines at start_in_line,
        with source=False they are cut from the lines' lower-case form.  Device route only, as SpansLines: a finder with regex
        terms, an injected engine or several devices has no host route to the spans (the cut itself has one:
        Engine.excerpt_spans_host) and is refused with GFT_E_UNSUPPORTED before anything is uploaded.  mark=(open, close): the excerpt
        blob goes through the mark call on the device before it comes down (MarkDevice's rule): every excerpt's bytes are the marked
        ones, and rel_start / rel_end index them.  snap="words": the excerpts begin and end at word borders (a word longer than
        `reach` bytes is cut where the window cut it); snap="lines" is for documents that hold several lines, as ExcerptsDevice
        takes them -- here every document is a line already, and the snap gives the whole line when it is within reach"""
        data = bytes(data)
        if not self._takes_device_route():
            raise FinderError(_lib.GFT_E_UNSUPPORTED, "ExcerptLines needs the device route, as the hit spans do: the GPU substring engine, no regex "
                                                      "terms, one device")
        buf = self._resident(data)
        off, bm, span_off, start, length, term, lowered = self._spans_of_lines(buf, len(data), want, source)
        out, exc_off, exc_doc, exc_start, exc_span_off, span_rel, _, _ = self.ExcerptsDevice(buf, off, span_off, start, length, lowered, source,
                                                                                             before, after, runes, snap, reach)
        if mark is not None:
            # the excerpts are a batch with a span CSR of their own: marked as such, never across an excerpt's border
            from .engine import mark_spans_tensor
            out, exc_off, span_rel, _ = mark_spans_tensor(lambda *a: self._check_engine(self._L.gft_mark_spans_device(self.engine_handle(), *a)),
                                                          out, exc_off, exc_span_off, span_rel, length, mark[0], mark[1])
        rows = bm.cpu().numpy().view(np.uint32).reshape(int(off.numel()) - 1, -1)
        w = self.want_mask() if want is None else np.ascontiguousarray(want, dtype=np.uint32)
        w = self.want_mask() & w
        hit = np.nonzero((rows & w[None, :]).any(axis=1))[0] if rows.shape[1] else np.zeros(0, dtype=np.int64)
        blob = out.cpu().numpy().tobytes()
        eo, ed, es, eso, rel, ln, tm = (t.cpu().numpy() for t in (exc_off, exc_doc, exc_start, exc_span_off, span_rel, length, term))
        terms = {}
        tp, tl = C.c_void_p(), C.c_uint32()
        for t in np.unique(tm).tolist():
            self._check_engine(self._L.gft_term(self.engine_handle(), int(t), C.byref(tp), C.byref(tl)))
            terms[t] = C.string_at(tp.value, tl.value)
        per_line = {}
        for k in range(ed.size):
            hits = [(int(rel[j]), int(rel[j]) + int(ln[j]), terms[int(tm[j])]) for j in range(int(eso[k]), int(eso[k + 1]))]
            per_line.setdefault(int(ed[k]), []).append((int(es[k]), blob[int(eo[k]):int(eo[k + 1])], hits))
        return hit.astype(np.uint64), [per_line.get(d, []) for d in hit.tolist()], lowered

    # -- markers written round the hits (csrc/gft_mark.hip) ---------------------------------------------------------------------------
    def MarkDevice(self, text, doc_off, span_off, start, length, lowered=False, source=False, open=b"<em>", close=b"</em>"):
        """Engine.mark_spans_device on the finder's engine behind SpansDevice (gft_finder_mark_device): text, doc_off the batch,
        span_off / start / length and `lowered` what SpansDevice returned for it, source as it was called.  With source, or for a
        batch that was not lowered, the caller's batch is marked; otherwise the batch's lower-case form, which the finder lowers on
        the device again.  Returns (out, out_off, span_new, doc_run_off, marked_lowered) -- device tensors as
        Engine.mark_spans_device gives them, and whether the lowered text was marked.  Needs what ProcessDevice needs"""
        from .engine import mark_spans_tensor
        low = C.c_int(0)

        def call(d_text, d_off, n, d_so, d_st, d_ln, *rest):
            self._check(self._L.gft_finder_mark_device(self._h, d_text, d_off, n, d_so, d_st, d_ln, 1 if lowered else 0, 1 if source else 0,
                                                       *rest, C.byref(low)))
        out = mark_spans_tensor(call, text, doc_off, span_off, start, length, open, close)
        return out + (bool(low.value),)

    def HighlightLines(self, data, open=b"<em>", close=b"</em>", want=None, source=True):
        """bytes -> (bytes, lowered): the blob with `open` in front of and `close` behind every keyword occurrence that is a witness of
        a true, wanted expression; occurrences that overlap or touch share one pair.  One upload, then split, process, spans and the
        marks on the device, one download of the marked blob.  lowered True: the batch left ASCII; with source=True (the default)
        the caller's bytes are marked all the same (the spans are mapped back to them), with source=False the lines' lower-case
        form.  Device route only, as SpansLines: a finder with regex terms, an injected engine or several devices has no host route
        to the spans and is refused with GFT_E_UNSUPPORTED before anything is uploaded"""
        data = bytes(data)
        if not self._takes_device_route():
            raise FinderError(_lib.GFT_E_UNSUPPORTED, "HighlightLines needs the device route, as the hit spans do: the GPU substring engine, no "
                                                      "regex terms, one device")
        buf = self._resident(data)
        off, _, span_off, start, length, _, lowered = self._spans_of_lines(buf, len(data), want, source)
        out = self.MarkDevice(buf, off, span_off, start, length, lowered, source, open, close)[0]
        return out.cpu().numpy().tobytes(), lowered

    # -- every hit run rewritten by its replacement (csrc/gft_replace.hip) ------------------------------------------------------------
    def ReplaceDevice(self, text, doc_off, span_off, start, length, term=None, lowered=False, source=False, reps=b"[REDACTED]", term_rep=None):
        """Engine.replace_spans_device on the finder's engine behind SpansDevice (gft_finder_replace_device): text, doc_off the batch,
        span_off / start / length / term and `lowered` what SpansDevice returned for it, source as it was called.  With source, or
        for a batch that was not lowered, the caller's text is replaced; otherwise the batch's lower-case form, which the finder
        lowers on the device again.  reps: the table (one bytes object or a list); term_rep: a host array with a table entry per term
        of the engine, None: entry 0 for every term.  Returns (out, out_off, doc_run_off, run_new, run_len, run_rep,
        replaced_lowered) -- device tensors as Engine.replace_spans_device gives them, and whether the lowered text was replaced.
        Needs what ProcessDevice needs"""
        from .engine import _p, replace_spans_tensor
        low = C.c_int(0)
        tr = None if term_rep is None else np.ascontiguousarray(term_rep, dtype=np.uint32)
        if tr is not None and tr.size != int(self._L.gft_n_terms(self.engine_handle())):
            raise ValueError("ReplaceDevice: term_rep needs an entry per term of the engine")

        def call(d_text, d_off, n, d_so, d_st, d_ln, d_key, _key_rep, _n_keys, *rest):
            self._check(self._L.gft_finder_replace_device(self._h, d_text, d_off, n, d_so, d_st, d_ln, 1 if lowered else 0, 1 if source else 0,
                                                          d_key, _p(tr), *rest, C.byref(low)))
        out = replace_spans_tensor(call, text, doc_off, span_off, start, length, reps, term if tr is not None else None)
        return out + (bool(low.value),)

    def _engine_terms(self):
        """{the dictionary's text of a term: its id} of the expressions added so far"""
        self.ForceBuild()                                           # (the dictionary of the expressions added so far: what the scan will use)
        eng = self.engine_handle()
        tp, tl = C.c_void_p(), C.c_uint32()
        terms = {}
        for t in range(int(self._L.gft_n_terms(eng))):
            self._check_engine(self._L.gft_term(eng, t, C.byref(tp), C.byref(tl)))
            terms[C.string_at(tp.value, tl.value)] = t
        return terms

    @staticmethod
    def _term_of(terms, kw, who):
        key = kw.encode("utf-8") if isinstance(kw, str) else bytes(kw)
        t = terms.get(key)
        if t is None:                                               # (a case-insensitive finder holds its keywords lowered)
            t = terms.get(key.decode("utf-8", "surrogateescape").lower().encode("utf-8", "surrogateescape"))
        if t is None:
            raise ValueError("%s: %r is no keyword of this finder" % (who, kw))
        return t

    def _replace_table(self, with_):
        """with_ of ReplaceLines -> (the table, a table entry per term of the engine or None)"""
        if isinstance(with_, (bytes, bytearray, memoryview)):
            return [bytes(with_)], None
        terms = self._engine_terms()
        default = bytes(with_.get(None, b"[REDACTED]"))
        reps, ids = [], {}
        term_rep = np.full(len(terms), -1, dtype=np.int64)
        for kw, rep in with_.items():
            if kw is None:
                continue
            rep = bytes(rep)
            if rep not in ids:
                ids[rep] = len(reps)
                reps.append(rep)
            term_rep[self._term_of(terms, kw, "ReplaceLines")] = ids[rep]
        if default not in ids:
            ids[default] = len(reps)
            reps.append(default)
        term_rep[term_rep < 0] = ids[default]
        return reps, term_rep.astype(np.uint32)

    def ReplaceLines(self, data, with_=b"[REDACTED]", want=None, source=True):
        """bytes -> (bytes, lowered): the blob with every keyword occurrence that is a witness of a true, wanted expression replaced;
        occurrences that overlap or touch are replaced together, once.  with_: bytes, one replacement for every keyword (b"" deletes),
        or a dict {keyword: bytes}; its optional key None is the default for the keywords it does not name, b"[REDACTED]" without
        it.  Distinct byte strings become table entries in the dict's insertion order, the default last: where occurrences of
        several keywords form one run, the run gets the replacement that comes first in the dict.  A keyword the finder's dictionary
        does not hold is a ValueError.  One upload, then split, process, spans and the replacement on the device, one download of
        the replaced blob.  lowered True: the batch left ASCII; with source=True (the default) the caller's bytes are replaced all
        the same (the spans are mapped back to them), with source=False the lines' lower-case form.  Device route only, as
        SpansLines: a finder with regex terms, an injected engine or several devices has no host route to the spans and is refused
        with GFT_E_UNSUPPORTED before anything is uploaded"""
        data = bytes(data)
        if not self._takes_device_route():
            raise FinderError(_lib.GFT_E_UNSUPPORTED, "ReplaceLines needs the device route, as the hit spans do: the GPU substring engine, no "
                                                      "regex terms, one device")
        reps, term_rep = self._replace_table(with_)
        buf = self._resident(data)
        off, _, span_off, start, length, term, lowered = self._spans_of_lines(buf, len(data), want, source)
        out = self.ReplaceDevice(buf, off, span_off, start, length, term, lowered, source, reps, term_rep)[0]
        return out.cpu().numpy().tobytes(), lowered

    # -- documents routed to one bucket per tag (csrc/gft_route.hip) -----------------------------------------------------------
    def route_masks(self, buckets=None):
        """the host masks of the route calls: a list of want_mask() rows, one per bucket.  None: one bucket per tag in tag-id order
        (tags()).  Otherwise a list whose items are what want_mask takes: a tag or a list of tags, a list of expression indices, or a
        dict of want_mask's keywords (indices=, tags=).  More than 64 buckets is a ValueError"""
        from .engine import ROUTE_MAX_BUCKETS
        if buckets is None:
            buckets = list(self.tags())
        if len(buckets) > ROUTE_MAX_BUCKETS:
            raise ValueError("route_masks: %d buckets, the limit is %d (GFT_ROUTE_MAX_BUCKETS)" % (len(buckets), ROUTE_MAX_BUCKETS))
        out = []
        for b in buckets:
            if isinstance(b, dict):
                out.append(self.want_mask(**b))
            elif isinstance(b, str):
                out.append(self.want_mask(tags=[b]))
            else:
                b = list(b)
                out.append(self.want_mask(tags=b) if b and all(isinstance(x, str) for x in b) else self.want_mask(indices=b))
        return out

    def _route_call(self):
        def call(d_text, d_off, n, d_bm, n_cols, *rest):
            self._check(self._L.gft_finder_route_docs_device(self._h, d_text, d_off, n, d_bm, *rest))
        return call

    def RouteDevice(self, text, doc_off, bitmap, masks, mode="every", rest=False, also=None):
        """Engine.route_docs_device on the finder's engine with n_cols = n_expressions (gft_finder_route_docs_device) over the rows
        ProcessDevice left; masks: route_masks().  Returns (out, out_off, doc_idx) on the device and (bucket_doc, bucket_byte) on the
        host.  Needs what ProcessDevice needs"""
        from .engine import route_docs_tensor
        return route_docs_tensor(self._route_call(), text, doc_off, bitmap, self.n_expressions, masks, mode, rest, also)

    def RouteLinesDevice(self, buf, length, buckets=None, mode="every", rest=False):
        """a resident blob of text lines -> the lines of every bucket: ProcessLinesDevice, then RouteDevice over its rows with
        route_masks(buckets).  Returns (out, out_off, doc_idx, bucket_doc, bucket_byte, doc_off, bitmap); a line keeps its newline"""
        off, bm = self.ProcessLinesDevice(buf, length)
        out, out_off, doc_idx, bucket_doc, bucket_byte = self.RouteDevice(buf, off, bm, self.route_masks(buckets), mode, rest)
        return out, out_off, doc_idx, bucket_doc, bucket_byte, off, bm

    def _resident(self, data):
        import torch
        dev = torch.device("cuda", self._device if self._device >= 0 else torch.cuda.current_device())
        buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        if data:
            buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        return buf

    def _host_lines(self, data):
        """(doc_off, rows) of a blob of lines by the host walk of the split and ProcessTexts"""
        from .engine import split_lines_host
        n, off = split_lines_host(data, 0)
        off = off[:n + 1]
        return off, self.ProcessTexts(blob=np.frombuffer(data + b"\0" * 64, dtype=np.uint8), doc_off=off)

    def RouteLines(self, data, buckets=None, mode="every", rest=False):
        """the host-memory form: bytes -> (parts, idx): parts a list of bytes, the lines of every bucket (the rest bucket last when
        asked for), idx a list of uint64 arrays, their input line numbers.  One upload; one blob, its offsets and indices come down.
        A finder that does not take the device route splits, processes and routes on the host -- the kernels' walk behind
        gft_debug_split_lines and gft_debug_route_docs --: the same result"""
        data = bytes(data)
        if self._takes_device_route():
            out, _, doc_idx, bucket_doc, bucket_byte, _, _ = self.RouteLinesDevice(self._resident(data), len(data), buckets, mode, rest)
            out, doc_idx = out.cpu().numpy().tobytes(), doc_idx.cpu().numpy().astype(np.uint64)
        else:
            from .engine import route_docs_host
            off, bm = self._host_lines(data)
            bucket_doc, bucket_byte, out, _, doc_idx = route_docs_host(data, off, bm, self.n_expressions, self.route_masks(buckets), mode, rest)
            out = out.tobytes()
        B = len(bucket_doc) - 1
        return ([out[int(bucket_byte[b]):int(bucket_byte[b + 1])] for b in range(B)],
                [doc_idx[int(bucket_doc[b]):int(bucket_doc[b + 1])].copy() for b in range(B)])

    def CountLines(self, data, buckets=None):
        """the count-only form: bytes -> (documents, bytes) per bucket as uint64 arrays -- a tag histogram of the lines.  Neither rows
        nor lines come down: the per-bucket counts are all that crosses the link"""
        data = bytes(data)
        masks = self.route_masks(buckets)
        if self._takes_device_route():
            from .engine import route_docs_tensor
            buf = self._resident(data)
            off, bm = self.ProcessLinesDevice(buf, len(data))
            bucket_doc, bucket_byte = route_docs_tensor(self._route_call(), buf, off, bm, self.n_expressions, masks, "every", False, None, count_only=True)
        else:
            from .engine import route_docs_host
            off, bm = self._host_lines(data)
            bucket_doc, bucket_byte = route_docs_host(data, off, bm, self.n_expressions, masks, "every", False, count_only=True)[:2]
        return np.diff(bucket_doc), np.diff(bucket_byte)

    # -- how often each keyword hit, and where (csrc/gft_stats.hip) ------------------------------------------------------------
    def _want_words(self, want):
        """want (None: every expression) as the mask words TermStatsDevice and TopDevice hand on: those of want_mask() among them"""
        return None if want is None else np.ascontiguousarray(self.want_mask() & np.ascontiguousarray(want, dtype=np.uint32))

    def _list_lines(self, data, kept, what, check=None):
        """the opening of TermStatsLines and TopLines: the blob resident and split into lines -> (buf, off, bm), bm the rows
        ProcessLinesDevice left (kept) or None (every occurrence); None when nothing can occur: no dictionary, or kept and no lines.
        what: the noun of the refusal off the device route; check: what the caller has to refuse in front of the upload"""
        if not self._takes_device_route():
            raise FinderError(_lib.GFT_E_UNSUPPORTED, what + " the device route: the GPU substring engine, no regex terms, one device")
        if not self.n_expressions:                                   # (no dictionary: nothing can occur)
            return None
        if check:
            check()
        buf = self._resident(data)
        if not kept:
            return buf, self.SplitLinesDevice(buf, len(data), 0), None
        off, bm = self.ProcessLinesDevice(buf, len(data))
        return (buf, off, bm) if bm.numel() else None                # (no lines)

    def TermStatsDevice(self, text, doc_off, bitmap=None, want=None, accumulate_into=None, doc_base=0):
        """the keyword statistics of a resident batch (gft_finder_term_stats_device).  text, doc_off as for ProcessDevice; bitmap: the
        rows ProcessDevice left -- the statistics are those of the KEPT matches, the witness occurrences of true, wanted expressions
        (want: want_mask(), None: every expression) --, or None: of every dictionary match of the batch.  accumulate_into: None, or
        the (occ, docs, first) a former call returned: the batch is added to them, doc_base being the documents in front of it.
        Returns (occ, docs, first, lowered): int64 [n_terms] device tensors indexed by the engine's term id -- occurrences, documents,
        doc_base + first document (-1: none) -- and whether the batch left ASCII and was lowered on the device first.  Needs what
        ProcessDevice needs"""
        import torch
        n = int(doc_off.numel()) - 1
        lowered = C.c_int(0)
        w = self._want_words(want)
        # (the dictionary is built by the first call that scans: n_terms is known only then -- a count-free call builds it)
        self._check(self._L.gft_finder_term_stats_device(self._h, text.data_ptr(), doc_off.data_ptr(), 0, None, None, 0, 0, None, None, None,
                                                         C.byref(lowered)))
        nt = int(self._L.gft_n_terms(self.engine_handle()))
        if accumulate_into is None:
            occ, docs = (torch.zeros(nt, dtype=torch.int64, device=text.device) for _ in range(2))
            first = torch.full((nt,), -1, dtype=torch.int64, device=text.device)
        else:
            occ, docs, first = accumulate_into
            assert all(a.dtype == torch.int64 and a.numel() == nt for a in (occ, docs, first))
        torch.cuda.current_stream(text.device).synchronize()
        self._check(self._L.gft_finder_term_stats_device(
            self._h, text.data_ptr(), doc_off.data_ptr(), n, bitmap.data_ptr() if bitmap is not None and bitmap.numel() else None,
            w.ctypes.data if w is not None and w.size else None, _lib.GFT_STATS_ACCUMULATE if accumulate_into is not None else 0, int(doc_base),
            *(a.data_ptr() if nt else None for a in (occ, docs, first)), C.byref(lowered)))
        return occ, docs, first, bool(lowered.value)

    def TermStatsLines(self, data, want=None, kept=True):
        """bytes -> ({keyword: (occurrences, documents, first_line)}, lowered) over the lines of a blob, for the keywords that
        occurred, keyed by the dictionary's text of the term (bytes, as gft_term gives it).  kept=True: the occurrences that are
        witnesses of a true, wanted expression (want: want_mask(), None: any) -- what SpansLines lists; kept=False: every occurrence
        of every keyword.  One upload; only the counters come down.  lowered as SpansLines returns it.  Device route only"""
        lines = self._list_lines(bytes(data), kept, "term statistics need")
        if lines is None:
            return {}, False
        buf, off, bm = lines
        occ, docs, first, lowered = self.TermStatsDevice(buf, off, bm, want if kept else None)
        occ, docs, first = (a.cpu().numpy() for a in (occ, docs, first))
        out = {}
        tp, tl = C.c_void_p(), C.c_uint32()
        for t in np.nonzero(occ)[0].tolist():
            self._check_engine(self._L.gft_term(self.engine_handle(), int(t), C.byref(tp), C.byref(tl)))
            out[C.string_at(tp.value, tl.value)] = (int(occ[t]), int(docs[t]), int(first[t]))
        return out, lowered

    # -- which documents matched most (csrc/gft_rank.hip) ----------------------------------------------------------------------
    def TopDevice(self, text, doc_off, bitmap=None, want=None, k=10, weights=None, distinct=False):
        """the scores of a resident batch and its k best documents (gft_finder_top_docs_device).  text, doc_off, bitmap and want as
        TermStatsDevice takes them: with the rows ProcessDevice left the KEPT matches score, with None every dictionary match.  A
        document's score is the sum of weights[t] over its scoring occurrences, with distinct over its distinct keywords; weights: a
        host array with a uint32 per term of the engine, None: every keyword 1.  Returns (top_idx, top_score, scores, lowered): int64
        device tensors -- the at most k documents with a score above 0, larger score first, among equals the smaller index first;
        their scores; every document's score -- and whether the batch left ASCII and was lowered on the device first (the indices
        are the caller's either way).  Needs what ProcessDevice needs"""
        import torch
        n = int(doc_off.numel()) - 1
        lowered, n_top = C.c_int(0), C.c_uint64(0)
        w = self._want_words(want)
        wt = None
        if weights is not None:
            self.ForceBuild()
            wt = np.ascontiguousarray(weights, dtype=np.uint32)
            if wt.size != int(self._L.gft_n_terms(self.engine_handle())):
                raise ValueError("TopDevice: weights needs an entry per term of the engine")
        scores = torch.zeros(n, dtype=torch.int64, device=text.device)
        idx, val = (torch.empty(max(k, 1), dtype=torch.int64, device=text.device) for _ in range(2))
        torch.cuda.current_stream(text.device).synchronize()
        self._check(self._L.gft_finder_top_docs_device(
            self._h, text.data_ptr(), doc_off.data_ptr(), n, bitmap.data_ptr() if bitmap is not None and bitmap.numel() else None,
            w.ctypes.data if w is not None and w.size else None, wt.ctypes.data if wt is not None and wt.size else None,
            _lib.GFT_SCORE_DISTINCT if distinct else 0, int(k), 0, scores.data_ptr() if n else None, idx.data_ptr(), val.data_ptr(),
            C.byref(n_top), C.byref(lowered)))
        return idx[:n_top.value], val[:n_top.value], scores, bool(lowered.value)

    def TopLines(self, data, k=10, weights=None, distinct=False, want=None, kept=True):
        """bytes -> ([(line_index, score, line_bytes), ...], lowered): the at most k lines of a blob that matched most, best first.  A
        line's score is the sum of its scoring occurrences' weights -- kept=True: the occurrences that are witnesses of a true, wanted
        expression (want: want_mask(), None: any), what SpansLines lists; kept=False: every occurrence of every keyword --, with
        distinct every keyword of a line once.  weights: None (every keyword 1), or a dict {keyword: int}; its optional key None is
        the weight of the keywords it does not name, 1 without it; 0 mutes a keyword; a keyword the finder's dictionary does not hold
        is a ValueError.  One upload; the k lines come down through gft_gather_docs_device, from the caller's own bytes even when the
        batch was lowered (lowered True), each with its newline.  Device route only"""
        wt = None

        def weigh():
            nonlocal wt
            if weights is not None:
                terms = self._engine_terms()
                wt = np.full(len(terms), int(weights.get(None, 1)), dtype=np.uint32)
                for kw, v in weights.items():
                    if kw is not None:
                        wt[self._term_of(terms, kw, "TopLines")] = int(v)
        lines = self._list_lines(bytes(data), kept, "the top lines need", weigh)
        if lines is None:
            return [], False
        buf, off, bm = lines
        idx, val, _, lowered = self.TopDevice(buf, off, bm, want if kept else None, k, wt, distinct)
        m = int(idx.numel())
        if not m:
            return [], lowered
        import torch
        out_off = torch.empty(m + 1, dtype=torch.int64, device=buf.device)
        total = C.c_uint64(0)
        head = (self.engine_handle(), buf.data_ptr(), off.data_ptr(), int(off.numel()) - 1, idx.data_ptr(), m, 0)
        torch.cuda.current_stream(buf.device).synchronize()
        self._check_engine(self._L.gft_gather_docs_device(*head, None, 0, out_off.data_ptr(), C.byref(total)))
        out = torch.zeros(total.value + 64, dtype=torch.uint8, device=buf.device)
        torch.cuda.current_stream(buf.device).synchronize()
        self._check_engine(self._L.gft_gather_docs_device(*head, out.data_ptr(), total.value, out_off.data_ptr(), C.byref(total)))
        blob, oo = out[:total.value].cpu().numpy().tobytes(), out_off.cpu().numpy()
        return [(int(i), int(v), blob[int(oo[j]):int(oo[j + 1])]) for j, (i, v) in enumerate(zip(idx.cpu().tolist(), val.cpu().tolist()))], lowered

    def CountExpressions(self, data):
        """bytes -> a uint64 array with one count per expression index: the number of lines of the blob on which the expression is
        true.  Neither rows nor lines come down (gft_count_columns_device over the rows ProcessLinesDevice left).  Device route only"""
        if not self._takes_device_route():
            raise FinderError(_lib.GFT_E_UNSUPPORTED, "expression counts need the device route: the GPU substring engine, no regex terms, one device")
        import torch
        data = bytes(data)
        buf = self._resident(data)
        off, bm = self.ProcessLinesDevice(buf, len(data))
        E = self.n_expressions
        count = torch.zeros(E, dtype=torch.int64, device=buf.device)
        torch.cuda.current_stream(buf.device).synchronize()
        self._check_engine(self._L.gft_count_columns_device(self.engine_handle(), bm.data_ptr() if bm.numel() else None, int(off.numel()) - 1, E, None,
                                                            0, count.data_ptr() if E else None))
        return count.cpu().numpy().astype(np.uint64)

    def _takes_device_route(self):
        """asks the handle: the split of an empty blob (gft_finder_split_lines_device, count only) answers what ProcessDevice asks
        of the finder -- the GPU substring engine, no regex terms, one device -- and whether there is a device at all.  Any other
        refusal (batches in flight) is the caller's"""
        if not self.engine_handle():                         # (a finder kept without a device has no engine handle)
            return False
        n = C.c_uint64(0)
        rc = self._L.gft_finder_split_lines_device(self._h, None, 0, 0, None, 0, C.byref(n))
        if rc in (_lib.GFT_E_UNSUPPORTED, _lib.GFT_E_HIP):
            return False
        self._check(rc)
        return True

    def ProcessDeviceBegin(self, d_text_ptr, d_doc_off_ptr, n_docs, d_bitmap_ptr):
        """pipelined ProcessDevice: enqueue the batch and return; ProcessDeviceEnd() completes the oldest batch begun (at
        most two in flight; inputs and bitmap stay untouched until then)"""
        self._check(self._L.gft_finder_process_device_begin(self._h, d_text_ptr, d_doc_off_ptr, n_docs, d_bitmap_ptr))

    def ProcessDeviceEnd(self):
        self._check(self._L.gft_finder_process_device_end(self._h))

    def lowered_batches(self):
        """-> (on_device, on_host): batches ProcessDevice / ProcessDeviceEnd repeated because their text left ASCII, by the
        path that lowered them (the device's ToLower kernels; the host with GFT_DEVICE_TOLOWER=0 or several devices)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.gft_finder_lowered_batches(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def engine_handle(self):
        return self._L.gft_finder_engine(self._h)

    # -- test hooks (finder_test.go pokes struct fields) --------------------------------------------------
    def debug_add_literal(self, which, lit):
        b = lit.encode("utf-8")
        self._check(self._L.gft_finder_debug_add_literal(self._h, which, b, len(b)))

    def debug_set_updated(self, sub, rgx):
        self._check(self._L.gft_finder_debug_set_updated(self._h, int(sub), int(rgx)))

    def debug_get_updated(self):
        a, b = C.c_int(), C.c_int()
        self._check(self._L.gft_finder_debug_get_updated(self._h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)


def NewFinder(subEng, rgxEng, caseSensitive, device=-1):
    return Finder(subEng, rgxEng, caseSensitive, device)
