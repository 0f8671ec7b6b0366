"""A run of documents cut from a larger batch, for the four calls that take "the spans [span_off[0], span_off[n_docs]) of the
caller's span arrays" (gft_excerpt_spans_device, gft_mark_spans_device, gft_redact_spans_device, gft_map_spans_to_source_device and
their host walks): cut() gives the argument list for the documents [a, b) of a batch -- doc_off and span_off sliced, the text and the
span arrays left whole, so span_off[0] != 0 --, restrict() what the contract promises for that run, computed from the reference's
answer for the whole batch; own_excerpt() / own_mark() / own_fill() build the same run as a case of its own behind span_lead
entries of poison, the second route to the same answer.  Batch, Out and the four run_*() drive either form of a call -- the host
walk over numpy arrays (HostMem) or the device call over device tensors (the Mem of tests/test_gpu_span_runs.py) -- through one
argument list, into guarded outputs that several runs of a partition share.  No tests in here and none of the code under test."""
import collections
import ctypes as C

import numpy as np

FULL = 0xFFFFFFFF
KINDS = ("excerpt", "mark", "redact", "map")
# the reference's answer for a whole batch: arrays = (blob, doc_off, span_off, start, len) as the call gets them; want: excerpts /
# mark: the dict of expected(); redact: the masked blob (bytes); map: (start, len) after the map, at the caller's indexes
Whole = collections.namedtuple("Whole", "kind arrays want")


def cut(arrays, a, b):
    """the argument list for the documents [a, b): doc_off[a .. b], span_off[a .. b]; the text and the span arrays stay whole"""
    blob, off, so, st, ln = arrays
    assert 0 <= a <= b < len(off)
    return blob, off[a:b + 1].copy(), so[a:b + 1].copy(), st, ln


def restrict(whole, a, b):
    """what the contract promises for the call over cut(whole.arrays, a, b), from the answer for the whole batch: the per-run outputs
    cut out and rebased to the run (document and excerpt numbers, byte offsets), the outputs that index the caller's span arrays
    (exc_span_off) as they are, the parallel outputs only inside [span_off[a], span_off[b]) -- None elsewhere: left alone"""
    blob, off, so, st, ln = whole.arrays
    w = whole.want
    lo, hi = int(so[a]), int(so[b])
    inside = lambda xs: [v if lo <= i < hi else None for i, v in enumerate(xs)]     # noqa: E731
    if whole.kind == "excerpt":
        e0, e1 = w["doc_exc_off"][a], w["doc_exc_off"][b]
        o0, o1 = w["exc_off"][e0], w["exc_off"][e1]
        return {"n_exc": e1 - e0, "total": o1 - o0, "out": w["out"][o0:o1], "exc_off": [v - o0 for v in w["exc_off"][e0:e1 + 1]],
                "exc_doc": [d - a for d in w["exc_doc"][e0:e1]], "exc_start": w["exc_start"][e0:e1], "exc_span_off": w["exc_span_off"][e0:e1] + [hi],
                "span_rel": inside(w["span_rel"]), "doc_exc_off": [v - e0 for v in w["doc_exc_off"][a:b + 1]]}
    if whole.kind == "mark":
        r0, o0, o1 = w["doc_run_off"][a], w["out_off"][a], w["out_off"][b]
        return {"n_runs": w["doc_run_off"][b] - r0, "total": o1 - o0, "out": w["out"][o0:o1], "out_off": [v - o0 for v in w["out_off"][a:b + 1]],
                "span_new": inside(w["span_new"]), "doc_run_off": [v - r0 for v in w["doc_run_off"][a:b + 1]]}
    if whole.kind == "redact":
        t0, t1 = int(off[a]), int(off[b])
        src = blob.tobytes()
        return src[:t0] + w[t0:t1] + src[t1:]
    assert whole.kind == "map"
    new_st, new_ln = st.copy(), ln.copy()
    new_st[lo:hi], new_ln[lo:hi] = w[0][lo:hi], w[1][lo:hi]
    return new_st, new_ln


def partition(n_docs, parts, rng):
    """`parts` consecutive runs [a, b) of at least one document each that cover [0, n_docs)"""
    assert 1 <= parts <= n_docs
    cuts = sorted(rng.choice(np.arange(1, n_docs), parts - 1, replace=False).tolist()) if parts > 1 else []
    edges = [0] + cuts + [n_docs]
    return list(zip(edges, edges[1:]))


def joined(kind, runs):
    """the per-run outputs of the consecutive runs of a partition, concatenated and rebased: what the whole-batch call hands back
    (the parallel outputs are not here: the runs wrote them into one array).  runs: [(a, b, result dict)]"""
    if kind == "excerpt":
        j = {"n_exc": 0, "total": 0, "out": b"", "exc_off": [0], "exc_doc": [], "exc_start": [], "exc_span_off": [], "doc_exc_off": [0]}
        for a, b, r in runs:
            j["exc_off"] += [v + j["total"] for v in r["exc_off"][1:]]
            j["exc_doc"] += [d + a for d in r["exc_doc"]]
            j["exc_start"] += list(r["exc_start"])
            j["exc_span_off"] = j["exc_span_off"][:-1] + list(r["exc_span_off"])
            j["doc_exc_off"] += [v + j["n_exc"] for v in r["doc_exc_off"][1:]]
            j["out"] += r["out"]
            j["n_exc"] += r["n_exc"]
            j["total"] += r["total"]
        return j
    assert kind == "mark"
    j = {"n_runs": 0, "total": 0, "out": b"", "out_off": [0], "doc_run_off": [0]}
    for a, b, r in runs:
        j["out_off"] += [v + j["total"] for v in r["out_off"][1:]]
        j["doc_run_off"] += [v + j["n_runs"] for v in r["doc_run_off"][1:]]
        j["out"] += r["out"]
        j["n_runs"] += r["n_runs"]
        j["total"] += r["total"]
    return j


def differs(got, want, untouched=None):
    """None, or what differs first between two result dicts / byte strings / tuples of arrays.  A None in `want` stands for an entry
    the call must leave alone: `got` must hold `untouched` there"""
    if isinstance(want, (bytes, bytearray)):
        if bytes(got) == bytes(want):
            return None
        g, w = np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(want), np.uint8)
        if g.size != w.size:
            return "%d bytes, want %d" % (g.size, w.size)
        i = int(np.nonzero(g != w)[0][0])
        return "byte %d: got %#x, want %#x" % (i, g[i], w[i])
    if isinstance(want, tuple):
        want = {str(i): v for i, v in enumerate(want)}
        got = {str(i): v for i, v in enumerate(got)}
    for k, w in want.items():
        g = got[k]
        if isinstance(w, (int, bytes)):
            if (bytes(g) if isinstance(w, bytes) else int(g)) != w:
                return "%s: got %r, want %r" % (k, g if isinstance(w, int) else "other bytes", w if isinstance(w, int) else "%d bytes" % len(w))
            continue
        unt = -1 if untouched is None else untouched                # (two references against each other: None is None)
        w = np.asarray([unt if v is None else v for v in (w.tolist() if isinstance(w, np.ndarray) else w)], dtype=np.int64)
        g = np.asarray([unt if v is None else v for v in (g.tolist() if isinstance(g, np.ndarray) else g)], dtype=np.int64)
        if g.shape != w.shape:
            return "%s: %d entries, want %d" % (k, g.size, w.size)
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            return "%s[%d]: got %d, want %d" % (k, i, g[i], w[i])
    return None


# ---- the run as a case of its own ---------------------------------------------------------------------------------------------
def own_excerpt(case, so, n_entries, a, b, off):
    """(case, span_lead, span_tail): the documents [a, b) of an excerpt or mark case as a case of their own whose arrays() lie as
    the cut's do: doc_off[0] = off[a], span_off[0] = so[a], n_entries span entries in all"""
    own = case.but("%s [%d, %d)" % (case.name, a, b), docs=case.docs[a:b], spans=case.spans[a:b], lead=int(off[a]))
    return own, int(so[a]), n_entries - int(so[b])


own_mark = own_excerpt


def own_fill(S, f, a, b):
    """the documents [a, b) of a FillCase (tests/spans.py) as a FillCase of its own over the same blob: its span arrays hold poison
    outside [span_off[a], span_off[b])"""
    lo, hi = int(f.span_off[a]), int(f.span_off[b])
    st, ln = np.full(f.start.size, FULL, np.uint32), np.full(f.length.size, FULL, np.uint32)
    st[lo:hi], ln[lo:hi] = f.start[lo:hi], f.length[lo:hi]
    return S.FillCase("%s [%d, %d)" % (f.name, a, b), f.blob, f.doc_off[a:b + 1].copy(), f.span_off[a:b + 1].copy(), st, ln, f.mask, f.ok)


# ---- either form of a call through one argument list --------------------------------------------------------------------------
class HostMem:
    """byte buffers on the host.  The device's form (tests/test_gpu_span_runs.py) has the same four methods"""

    def put(self, a):
        return np.ascontiguousarray(a).view(np.uint8).copy()

    def ptr(self, h, at=0):
        return h.ctypes.data + at if h.size else None

    def get(self, h):
        return h

    def sync(self):
        pass


G = 8                                                               # guard entries on either side of every output


class Out:
    """an output of n entries with G guard entries on either side, every byte of the allocation `pat`; shift: bytes further on"""

    def __init__(self, mem, n, dtype, pat=0xA5, shift=0):
        self.mem, self.n, self.dtype, self.pat, self.item = mem, n, np.dtype(dtype), pat, np.dtype(dtype).itemsize
        self.lo = G * self.item + shift
        self.h = mem.put(np.full(self.lo + (n + G) * self.item, pat, np.uint8))

    @property
    def ptr(self):
        return self.mem.ptr(self.h, self.lo)

    def at(self, i):
        """the address of entry i (for the overlap checks)"""
        return self.mem.ptr(self.h, self.lo + i * self.item)

    def untouched(self):
        return int(np.full(self.item, self.pat, np.uint8).view(self.dtype)[0])

    def whole(self):
        return self.mem.get(self.h)

    def read(self, n=None, what=""):
        """the first n entries (default: all); every byte of the allocation outside them must hold the pattern"""
        n = self.n if n is None else n
        raw = np.array(self.mem.get(self.h))
        hi = self.lo + n * self.item
        assert (raw[:self.lo] == self.pat).all() and (raw[hi:] == self.pat).all(), "%s: a store outside the output" % what
        return raw[self.lo:hi].view(self.dtype)


class Batch:
    """a batch in some memory: the text `at` bytes into an allocation whose every other byte -- in front, the 64 bytes of slack --
    holds `fill`; doc_off, span_off and the span arrays whole.  args(a, b): the pointers the four calls take for the documents
    [a, b): doc_off + a, span_off + a, n = b - a, everything else as it is"""

    def __init__(self, mem, arrays, fill=0x00, at=0):
        blob, off, so, st, ln = arrays
        self.mem, self.arrays, self.at, self.n_docs = mem, arrays, at, len(off) - 1
        raw = np.full(at + blob.size + 64, fill, np.uint8)
        raw[at:at + blob.size] = blob
        self.text, self.off, self.so = mem.put(raw), mem.put(off.astype(np.uint64)), mem.put(so.astype(np.uint64))
        self.st, self.ln = mem.put(st.astype(np.uint32)), mem.put(ln.astype(np.uint32))
        self.n_entries = st.size

    def args(self, a=0, b=None):
        b = self.n_docs if b is None else b
        m = self.mem
        return (m.ptr(self.text, self.at), m.ptr(self.off, 8 * a), b - a, m.ptr(self.so, 8 * a), m.ptr(self.st), m.ptr(self.ln))

    def text_now(self):
        """the whole allocation of the text as it is now (bytes)"""
        return np.array(self.mem.get(self.text)).tobytes()

    def text_want(self, blob_bytes, fill):
        """the allocation that holds blob_bytes and `fill` everywhere else"""
        raw = np.full(self.at + len(blob_bytes) + 64, fill, np.uint8)
        raw[self.at:self.at + len(blob_bytes)] = np.frombuffer(blob_bytes, np.uint8)
        return raw.tobytes()

    def spans_now(self):
        return np.array(self.mem.get(self.st)).view(np.uint32), np.array(self.mem.get(self.ln)).view(np.uint32)


EXC_OUTS = (("out", np.uint8), ("exc_off", np.uint64), ("exc_doc", np.uint64), ("exc_start", np.uint32), ("exc_span_off", np.uint64),
            ("doc_exc_off", np.uint64))


def run_excerpt(call, bt, a, b, before, after, flags, span_rel, cap_bytes=None, cap_exc=None, pat=0xA5, shift=0, count_only=False):
    """call: gft_debug_excerpt_spans, or gft_excerpt_spans_device behind its handle.  Counts with NULL outputs, then fills guarded
    outputs of exactly the sizes counted (or what the caps allow); span_rel: an Out of n_entries entries that the runs of a
    partition share, or None -> (rc, result dict: the arrays cut to what the caps allow, guards checked; span_rel is not in it)"""
    m, total = C.c_uint64(0), C.c_uint64(0)
    head = bt.args(a, b) + (before, after, flags)
    bt.mem.sync()
    rc = call(*head, None, 0, None, None, None, None, 0, None, None, C.byref(m), C.byref(total))
    if rc or count_only:
        return rc, {"n_exc": int(m.value), "total": int(total.value)}
    nm, nb = int(m.value), int(total.value)
    cb, ce = nb if cap_bytes is None else cap_bytes, nm if cap_exc is None else cap_exc
    sizes = {"out": min(nb, cb), "exc_off": min(nm, ce) + 1, "exc_doc": min(nm, ce), "exc_start": min(nm, ce), "exc_span_off": min(nm, ce) + 1,
             "doc_exc_off": b - a + 1}
    outs = {k: Out(bt.mem, sizes[k], t, pat, shift if k == "out" else 0) for k, t in EXC_OUTS}
    bt.mem.sync()
    rc = call(*head, outs["out"].ptr, cb, outs["exc_off"].ptr, outs["exc_doc"].ptr, outs["exc_start"].ptr, outs["exc_span_off"].ptr, ce,
              span_rel.ptr if span_rel is not None else None, outs["doc_exc_off"].ptr, C.byref(m), C.byref(total))
    r = {"n_exc": int(m.value), "total": int(total.value)}
    if rc == 0:
        assert (r["n_exc"], r["total"]) == (nm, nb), "the fill call counts otherwise than the count-only call"
        for k, _ in EXC_OUTS:
            r[k] = outs[k].read(what=k).tobytes() if k == "out" else outs[k].read(what=k).tolist()
    else:
        r["outs"] = outs
    return rc, r


MARK_OUTS = (("out", np.uint8), ("out_off", np.uint64), ("doc_run_off", np.uint64))


def run_mark(call, bt, a, b, open, close, span_new, cap_bytes=None, pat=0xA5, shift=0, count_only=False):
    """run_excerpt's protocol for gft_debug_mark_spans / gft_mark_spans_device; span_new: the shared Out, or None"""
    m, total = C.c_uint64(0), C.c_uint64(0)
    head = bt.args(a, b) + (open or None, len(open), close or None, len(close), 0)
    bt.mem.sync()
    rc = call(*head, None, 0, None, None, None, C.byref(m), C.byref(total))
    if rc or count_only:
        return rc, {"n_runs": int(m.value), "total": int(total.value)}
    nm, nb = int(m.value), int(total.value)
    cb = nb if cap_bytes is None else cap_bytes
    sizes = {"out": min(nb, cb), "out_off": b - a + 1, "doc_run_off": b - a + 1}
    outs = {k: Out(bt.mem, sizes[k], t, pat, shift if k == "out" else 0) for k, t in MARK_OUTS}
    bt.mem.sync()
    rc = call(*head, outs["out"].ptr, cb, outs["out_off"].ptr, span_new.ptr if span_new is not None else None, outs["doc_run_off"].ptr,
              C.byref(m), C.byref(total))
    r = {"n_runs": int(m.value), "total": int(total.value)}
    if rc == 0:
        assert (r["n_runs"], r["total"]) == (nm, nb), "the fill call counts otherwise than the count-only call"
        for k, _ in MARK_OUTS:
            r[k] = outs[k].read(what=k).tobytes() if k == "out" else outs[k].read(what=k).tolist()
    else:
        r["outs"] = outs
    return rc, r


def run_redact(call, bt, a, b, mask):
    """gft_debug_redact_spans / gft_redact_spans_device over the documents [a, b), in place in bt's text -> rc"""
    bt.mem.sync()
    rc = call(*bt.args(a, b), mask)
    bt.mem.sync()
    return rc


def run_map(call, bt, a, b, limit=None):
    """gft_debug_map_spans_to_source / gft_map_spans_to_source_device (limit: gft_map_spans_limit) over the documents [a, b), in
    place in bt's span arrays -> rc"""
    bt.mem.sync()
    rc = call(*bt.args(a, b)) if limit is None else call(*bt.args(a, b), limit)
    bt.mem.sync()
    return rc


def parallel(out, want, what):
    """the shared parallel output against the reference's list at the caller's indexes (None: left alone), guards checked"""
    d = differs({what: out.read(what=what)}, {what: want}, out.untouched())
    assert d is None, d


# ---- the checks both forms of the calls go through ----------------------------------------------------------------------------
class Driver:
    """mem: HostMem or the device's; calls: {"excerpt", "mark", "redact", "map"[, "map_limit"]} -> the C calls without their handle;
    X, M, S, LM: the case modules (tests/excerpts.py, mark.py, spans.py, lowermap_cases.py); invalid: GFT_E_INVALID"""

    def __init__(self, mem, calls, X, M, S, LM, invalid):
        self.mem, self.calls, self.X, self.M, self.S, self.LM, self.invalid = mem, calls, X, M, S, LM, invalid

    # a whole batch behind span_lead entries of poison, span_tail behind it
    def excerpt_case(self, case, lead, tail, fill=0x00, at=0, shift=0, want=None):
        bt = Batch(self.mem, case.arrays(fill, lead, tail), fill, at)
        pat = 0xBF if fill else 0x5A
        rel = Out(self.mem, bt.n_entries, np.uint32, pat)
        rc, r = run_excerpt(self.calls["excerpt"], bt, 0, bt.n_docs, case.before, case.after, int(case.runes), rel, pat=pat, shift=shift)
        assert rc == 0, "%s behind %d: refused (%d)" % (case.name, lead, rc)
        r["span_rel"] = rel.read(what="span_rel").tolist()
        d = differs(r, want or self.X.expected(case, None, lead, tail), rel.untouched())
        assert d is None, "%s behind %d spans, fill %#x, text at +%d: %s" % (case.name, lead, fill, at, d)

    def mark_case(self, case, lead, tail, fill=0x00, at=0, shift=0, want=None):
        bt = Batch(self.mem, case.arrays(fill, lead, tail), fill, at)
        pat = 0xBF if fill else 0x5A
        new = Out(self.mem, bt.n_entries, np.uint32, pat)
        rc, r = run_mark(self.calls["mark"], bt, 0, bt.n_docs, case.open, case.close, new, pat=pat, shift=shift)
        assert rc == 0, "%s behind %d: refused (%d)" % (case.name, lead, rc)
        r["span_new"] = new.read(what="span_new").tolist()
        d = differs(r, want or self.M.expected(case, None, lead, tail), new.untouched())
        assert d is None, "%s behind %d spans, fill %#x, text at +%d: %s" % (case.name, lead, fill, at, d)

    def fill_case(self, f, fill=0x00, at=0, a=0, b=None, want=None):
        """a FillCase, or its documents [a, b); a case that is not ok must be refused with every byte as it was"""
        bt = Batch(self.mem, (f.blob, f.doc_off, f.span_off, f.start, f.length), fill, at)
        rc = run_redact(self.calls["redact"], bt, a, bt.n_docs if b is None else b, f.mask)
        if want is None and not f.ok:
            assert rc == self.invalid and bt.text_now() == bt.text_want(f.blob.tobytes(), fill), "%s: not refused, or written" % f.name
            return
        assert rc == 0, "%s behind %d: refused (%d)" % (f.name, int(f.span_off[0]), rc)
        d = differs(bt.text_now(), bt.text_want(want or self.S.redact_reference(f), fill))
        assert d is None, "%s behind %d spans, text at +%d: %s" % (f.name, int(f.span_off[a]), at, d)

    def map_case(self, docs, spans, lead, tail, doc_lead=0, fill=0x00, at=0, limit=None, a=0, b=None, what=""):
        """the documents [a, b) of a lowered batch's spans mapped in place; limit: through gft_map_spans_limit"""
        import tolower_cases as TC
        blob, off = TC.pack(list(docs), doc_lead)
        so, st, ln = self.LM.flat(spans, lead, tail)
        bt = Batch(self.mem, (blob, off, so, st, ln), fill, at)
        b = bt.n_docs if b is None else b
        rc = run_map(self.calls["map" if limit is None else "map_limit"], bt, a, b, limit)
        assert rc == 0, "%s behind %d: refused (%d)" % (what, lead, rc)
        w = self.LM.expected(docs, spans, lead, tail, limit)
        want = restrict(Whole("map", (blob, off, so, st, ln), w[1:]), a, b)
        d = differs(bt.spans_now(), want)
        assert d is None, "%s behind %d spans, [%d, %d), limit %r: %s" % (what, lead, a, b, limit, d)

    # the documents [a, b) of a batch, against restrict() of the reference's answer for the whole batch
    def excerpt_cut(self, case, a, b, whole_want, lead=0, tail=0, fill=0xBF, at=0):
        arrays = case.arrays(fill, lead, tail)
        bt = Batch(self.mem, arrays, fill, at)
        rel = Out(self.mem, bt.n_entries, np.uint32)
        rc, r = run_excerpt(self.calls["excerpt"], bt, a, b, case.before, case.after, int(case.runes), rel)
        assert rc == 0, "%s [%d, %d): refused (%d)" % (case.name, a, b, rc)
        r["span_rel"] = rel.read(what="span_rel").tolist()
        d = differs(r, restrict(Whole("excerpt", arrays, whole_want), a, b), rel.untouched())
        assert d is None, "%s, documents [%d, %d) behind %d spans: %s" % (case.name, a, b, int(arrays[2][a]), d)

    def mark_cut(self, case, a, b, whole_want, lead=0, tail=0, fill=0xEE, at=0):
        arrays = case.arrays(fill, lead, tail)
        bt = Batch(self.mem, arrays, fill, at)
        new = Out(self.mem, bt.n_entries, np.uint32)
        rc, r = run_mark(self.calls["mark"], bt, a, b, case.open, case.close, new)
        assert rc == 0, "%s [%d, %d): refused (%d)" % (case.name, a, b, rc)
        r["span_new"] = new.read(what="span_new").tolist()
        d = differs(r, restrict(Whole("mark", arrays, whole_want), a, b), new.untouched())
        assert d is None, "%s, documents [%d, %d) behind %d spans: %s" % (case.name, a, b, int(arrays[2][a]), d)

    def fill_cut(self, f, a, b, whole_want, at=0):
        want = restrict(Whole("redact", (f.blob, f.doc_off, f.span_off, f.start, f.length), whole_want), a, b)
        self.fill_case(f, 0x00, at, a, b, want)

    # the consecutive runs of a partition, all writing into the same parallel arrays
    def excerpt_partition(self, case, runs, whole_want, lead=0, tail=0, fill=0x00, at=0):
        bt = Batch(self.mem, case.arrays(fill, lead, tail), fill, at)
        rel = Out(self.mem, bt.n_entries, np.uint32)
        got = []
        for a, b in runs:
            rc, r = run_excerpt(self.calls["excerpt"], bt, a, b, case.before, case.after, int(case.runes), rel)
            assert rc == 0, "%s [%d, %d): refused (%d)" % (case.name, a, b, rc)
            got.append((a, b, r))
        j = joined("excerpt", got)
        d = differs(j, {k: v for k, v in whole_want.items() if k != "span_rel"})
        assert d is None, "%s in %d runs, joined: %s" % (case.name, len(runs), d)
        parallel(rel, whole_want["span_rel"], "span_rel")

    def mark_partition(self, case, runs, whole_want, lead=0, tail=0, fill=0x00, at=0):
        bt = Batch(self.mem, case.arrays(fill, lead, tail), fill, at)
        new = Out(self.mem, bt.n_entries, np.uint32)
        got = []
        for a, b in runs:
            rc, r = run_mark(self.calls["mark"], bt, a, b, case.open, case.close, new)
            assert rc == 0, "%s [%d, %d): refused (%d)" % (case.name, a, b, rc)
            got.append((a, b, r))
        d = differs(joined("mark", got), {k: v for k, v in whole_want.items() if k != "span_new"})
        assert d is None, "%s in %d runs, joined: %s" % (case.name, len(runs), d)
        parallel(new, whole_want["span_new"], "span_new")

    def fill_partition(self, f, runs, at=0):
        """run by run in place: the whole batch's masked text exactly"""
        bt = Batch(self.mem, (f.blob, f.doc_off, f.span_off, f.start, f.length), 0x00, at)
        for a, b in runs:
            assert run_redact(self.calls["redact"], bt, a, b, f.mask) == 0, "%s [%d, %d): refused" % (f.name, a, b)
        d = differs(bt.text_now(), bt.text_want(self.S.redact_reference(f), 0x00))
        assert d is None, "%s in %d runs: %s" % (f.name, len(runs), d)

    def map_partition(self, docs, spans, runs, lead=0, tail=0, doc_lead=0):
        """run by run in place: the whole batch's mapped spans exactly"""
        import tolower_cases as TC
        blob, off = TC.pack(list(docs), doc_lead)
        so, st, ln = self.LM.flat(spans, lead, tail)
        bt = Batch(self.mem, (blob, off, so, st, ln))
        for a, b in runs:
            assert run_map(self.calls["map"], bt, a, b) == 0, "[%d, %d): refused" % (a, b)
        d = differs(bt.spans_now(), self.LM.expected(docs, spans, lead, tail)[1:])
        assert d is None, "in %d runs: %s" % (len(runs), d)

    # refusals behind a base: every output as it was
    def excerpt_refused(self, case, lead, tail, a=0, b=None, so=None, what=""):
        """the call over the case (span_off replaced by `so` if given) is refused, and nothing is written: neither the guarded
        outputs sized for `sizes` nor span_rel"""
        arrays = list(case.arrays(0xBF, lead, tail))
        if so is not None:
            arrays[2] = np.asarray(so, np.uint64)
        bt = Batch(self.mem, tuple(arrays), 0xBF)
        b = bt.n_docs if b is None else b
        rel = Out(self.mem, bt.n_entries, np.uint32)
        outs = {k: Out(self.mem, 64, t) for k, t in EXC_OUTS}
        m, total = C.c_uint64(7), C.c_uint64(7)
        self.mem.sync()
        rc = self.calls["excerpt"](*bt.args(a, b), case.before, case.after, int(case.runes), outs["out"].ptr, 64, outs["exc_off"].ptr,
                                   outs["exc_doc"].ptr, outs["exc_start"].ptr, outs["exc_span_off"].ptr, 63, rel.ptr,
                                   outs["doc_exc_off"].ptr if b - a < 64 else None, C.byref(m), C.byref(total))
        assert rc == self.invalid and (m.value, total.value) == (0, 0), "%s: %s is not refused (%d)" % (case.name, what, rc)
        for k, o in list(outs.items()) + [("span_rel", rel)]:
            assert (np.array(o.whole()) == o.pat).all(), "%s, %s: %s was written" % (case.name, what, k)

    def mark_refused(self, case, lead, tail, a=0, b=None, so=None, what=""):
        arrays = list(case.arrays(0xBF, lead, tail))
        if so is not None:
            arrays[2] = np.asarray(so, np.uint64)
        bt = Batch(self.mem, tuple(arrays), 0xBF)
        b = bt.n_docs if b is None else b
        new = Out(self.mem, bt.n_entries, np.uint32)
        outs = {k: Out(self.mem, 64, t) for k, t in MARK_OUTS}
        m, total = C.c_uint64(7), C.c_uint64(7)
        self.mem.sync()
        rc = self.calls["mark"](*bt.args(a, b), case.open, len(case.open), case.close, len(case.close), 0, outs["out"].ptr, 64,
                                outs["out_off"].ptr if b - a < 64 else None, new.ptr, outs["doc_run_off"].ptr if b - a < 64 else None,
                                C.byref(m), C.byref(total))
        assert rc == self.invalid and (m.value, total.value) == (0, 0), "%s: %s is not refused (%d)" % (case.name, what, rc)
        for k, o in list(outs.items()) + [("span_new", new)]:
            assert (np.array(o.whole()) == o.pat).all(), "%s, %s: %s was written" % (case.name, what, k)

    def fill_refused(self, f, what=""):
        bt = Batch(self.mem, (f.blob, f.doc_off, f.span_off, f.start, f.length), 0x00)
        rc = run_redact(self.calls["redact"], bt, 0, bt.n_docs, f.mask)
        assert rc == self.invalid and bt.text_now() == bt.text_want(f.blob.tobytes(), 0x00), "%s, %s: not refused (%d), or written" % (f.name, what, rc)

    def map_refused(self, docs, so, st, ln, what=""):
        import tolower_cases as TC
        blob, off = TC.pack(list(docs))
        bt = Batch(self.mem, (blob, off, np.asarray(so, np.uint64), st, ln))
        rc = run_map(self.calls["map"], bt, 0, bt.n_docs)
        now = bt.spans_now()
        assert rc == self.invalid and np.array_equal(now[0], st) and np.array_equal(now[1], ln), "%s: not refused (%d), or written" % (what, rc)
