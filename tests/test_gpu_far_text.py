"""The resident-batch calls at text positions past 4 GiB (far_text.py).  Layer A: the fixed cases of the per-call suites placed
across position 2^32 of ONE allocation of 4 GiB + 1 MiB -- the call gets the allocation's base as `text` and doc_off + at, and must
answer exactly what it answers for the bare case, since every output is stated relative to the batch or the document --, at the
seven border placements of far_text.border_placements.  Layer B: one batch of about 4.6 GiB, islands of fixed cases between
documents of just under 1 GiB of position-dependent filler, laid out so that input position 2^32 -- and, for the calls that grow or
shrink the text, output position 2^32 -- falls inside a span in the middle of an island; the outputs against the sparse references
of far_text.py, arrays exactly on the host, blobs segment by segment on the device.  All comparisons are exact."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import excerpts as X
import far_text as F
import lowermap_cases as LM
import mark as M
import placement as pl
import replace as R
import route_docs as RD
import select_docs as SD
import span_runs as SR
import spans as S
import tolower_cases as TC
import word_cases as W
from gofindthem_amd.engine import Engine, excerpt_shape, mark_shape, replace_shape, words_shape
from gofindthem_amd.finder import EmptyRgxEngine, Finder, GpuEngine
from helpers import assert_csr_equal, tree_to_program
from oracle import dsl_ref
from oracle.pyoracle import POS_END, POS_START, Oracle, pack_strings

pytestmark = pytest.mark.gpu

B, SLACK, POISON = F.B, F.SLACK, F.POISON
AROUND = 4096
_HELD = {}                                                          # the two big allocations; one at a time


def _release(name):
    if name in _HELD:
        del _HELD[name]
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def dev(a):
    """a numpy array as a device tensor of signed integers of its width (an empty one gets an address)"""
    a = np.ascontiguousarray(a)
    signed = a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(np.concatenate([signed.ravel(), np.zeros(1, signed.dtype)])).cuda()[:a.size]


# ---- layer A ---------------------------------------------------------------------------------------------------------------------------
class Window:
    """the allocation of B + 1 MiB + 64 bytes, poisoned once; a case writes its text and the 64 bytes of slack and wipes them again"""

    def __init__(self):
        self.buf = torch.full((B + F.WINDOW + SLACK,), POISON, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    def place(self, text, at, slack=b""):
        """text: the lead bytes and the documents (numpy uint8 or bytes); slack: what lies behind them, padded with zeros to 64"""
        text = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
        slack = bytes(slack)[:SLACK] + bytes(SLACK - min(len(slack), SLACK))
        data = np.concatenate([text, np.frombuffer(slack, np.uint8)])
        assert at >= 0 and at + data.size <= self.buf.numel()
        self.buf[at:at + data.size] = torch.from_numpy(data.copy()).cuda()
        self.at, self.n = at, data.size
        return self.buf

    def wipe(self, what):
        """4 KiB on either side of the text and its slack kept the poison; the window gets it back"""
        a, b = self.at, self.at + self.n
        around = bool((self.buf[max(a - AROUND, 0):a] == POISON).all()) and bool((self.buf[b:b + AROUND] == POISON).all())
        assert around, (what, "a store outside the text")
        self.buf[a:b] = POISON


@pytest.fixture(scope="module")
def win():
    _release("long")
    _HELD["win"] = Window()
    yield _HELD["win"]
    _release("win")


def run_layer_a(win, cases, call, what):
    """cases: [(name, text bytes with the lead, slack, intervals)]; call(name, at) runs the case with its text at `at` and returns
    None or what differs.  Every case at every border placement; a case is left out only by far_text.fits, and that is said; at
    least one placement put B strictly inside one of the case's intervals (spans, runs, matches or documents, as `what` says)"""
    inside, skipped, bad, n = [], [], [], 0
    for name, text, slack, intervals in cases:
        if not F.fits(len(text)):
            skipped.append(name)
            continue
        for label, at in F.border_placements(len(text)):
            win.place(text, at, slack)
            d = call(name, at)
            n += 1
            if d:
                bad.append((name, label, d))
            win.wipe((name, label))
            if F.strictly_inside(at, intervals):
                inside.append((name, label))
    print("%s: %d runs of %d cases; left out as too long for the window: %s; 2^32 strictly inside %s in %d runs, the first %s"
          % (what, n, len(cases) - len(skipped), skipped or "none", what, len(inside), inside[:3]))
    assert not bad, "%d of %d runs differ; the first: %s" % (len(bad), n, bad[:5])
    assert n >= 6 * len(F.BORDER_NAMES) and len(cases) - len(skipped) >= 6
    assert inside, "no placement put 2^32 strictly inside %s" % what


def span_intervals(arrays):
    """the spans of a case's arrays() in positions of the placed text"""
    blob, off, so, st, ln = arrays[:5]
    out = []
    for d in range(len(off) - 1):
        for s in range(int(so[d]), int(so[d + 1])):
            out.append((int(off[d]) + int(st[s]), int(off[d]) + int(st[s]) + int(ln[s])))
    return out


def doc_intervals(off):
    return [(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


def tensors(arrays, at):
    blob, off, so, st, ln = arrays[:5]
    return dev((off + np.uint64(at)).astype(np.int64)), dev(so.astype(np.int64)), dev(st), dev(ln)


XT, XTRIP = excerpt_shape()
LEAD, TAIL = 3, 2                                                   # span_lead / span_tail of the cases that have them


def with_bases(cases, pick):
    """[(case, span_lead, span_tail)]: every case bare, the picked ones behind a span base as well"""
    return [(c, 0, 0) for c in cases] + [(c, LEAD, TAIL) for c in cases if c.name in pick]


def test_a_mark(eng, win):
    assert mark_shape()[2:] == (M.CHUNK, M.TILE)
    cs = with_bases([c for c in M.fixed_cases() if c.docs], ("straddle_tile", "straddle_trip", "touch_across_docs", "text_residue_5", "second_doc_ranks"))
    table = {}
    for c, lead, tail in cs:
        a = c.arrays(0x3C, lead, tail)
        table["%s behind %d" % (c.name, lead)] = (c, a, M.expected(c, None, lead, tail))
    assert {"straddle_tile behind 0", "straddle_trip behind 3", "touch_across_docs behind 0", "text_residue_5 behind 3"} <= set(table)

    def call(name, at):
        c, a, want = table[name]
        off, so, st, ln = tensors(a, at)
        out, out_off, span_new, dro = eng.mark_spans_device(win.buf, off, so, st, ln, c.open, c.close)
        got = {"n_runs": int(dro[-1]), "total": int(out.numel()), "out": out.cpu().numpy().tobytes(), "out_off": out_off.cpu().tolist(),
               "span_new": span_new.cpu().tolist(), "doc_run_off": dro.cpu().tolist()}
        return SR.differs(got, want, 0)
    run_layer_a(win, [(k, a[0], b"", span_intervals(a)) for k, (c, a, _) in table.items()], call, "a span")


def test_a_replace(eng, win):
    lds = replace_shape()[5]
    base = {c.name: c for c in R.fixed_cases()}
    big = base["straddle_tile"].but("straddle_tile_table_over_lds", reps=[b"[NAME]"] + [R._rep(40, k) for k in range(200)])
    cases = [c for c in R.fixed_cases() if c.docs] + [big]
    sizes = [sum(len(r) for r in c.reps) for c in cases]
    assert min(sizes) <= lds < sum(len(r) for r in big.reps) and sum(len(r) for r in base["table_65536"].reps) > lds
    cs = with_bases(cases, ("straddle_tile", "straddle_trip", "touch_across_docs", "text_residue_5", "key_rep_given", "straddle_tile_table_over_lds"))
    table = {}
    for c, lead, tail in cs:
        table["%s behind %d" % (c.name, lead)] = (c, c.arrays(0x3C, lead, tail), R.expected(c, None, lead))

    def call(name, at):
        c, a, want = table[name]
        off, so, st, ln = tensors(a, at)
        key = dev(a[5]) if a[5] is not None else None
        t = eng.replace_spans_device(win.buf, off, so, st, ln, c.reps, key, c.key_rep)
        got = {"n_runs": int(t[2][-1]), "total": int(t[0].numel()), "out": t[0].cpu().numpy().tobytes()}
        got.update({k: v.cpu().tolist() for k, v in zip(R.ARRAYS, t[1:])})
        return SR.differs(got, want)
    run_layer_a(win, [(k, a[0], b"", span_intervals(a)) for k, (c, a, _) in table.items()], call, "a span")


def test_a_excerpt(eng, win):
    # (every fixed case with documents but the two of more than a carry trip of spans, which take seconds to upload seven times)
    cases = [c for c in X.fixed_cases(XT, XTRIP) if c.docs and sum(len(s) for s in c.spans) <= 4 * XT]
    cs = with_bases(cases, ("a run crosses a tile border", "a document border on a tile border", "windows touch in the blob", "doc_off[0] != 0"))
    table = {}
    for c, lead, tail in cs:
        table["%s behind %d" % (c.name, lead)] = (c, c.arrays(0xBF, lead, tail), X.expected(c, None, lead, tail))
    assert "a run crosses a tile border behind 3" in table and "a lead byte is not the document's behind 0" in table

    def call(name, at):
        c, a, want = table[name]
        off, so, st, ln = tensors(a, at)
        t = eng.excerpt_spans_device(win.buf, off, so, st, ln, c.before, c.after, c.runes)
        got = {"n_exc": int(t[2].numel()), "total": int(t[0].numel()), "out": t[0].cpu().numpy().tobytes()}
        got.update({k: v.cpu().numpy().tolist() for k, v in zip(X.ARRAYS, t[1:7])})
        return SR.differs(got, want, 0)
    run_layer_a(win, [(k, a[0], b"", span_intervals(a)) for k, (c, a, _) in table.items()], call, "a span")


def test_a_redact_in_place(eng, win):
    """... and 4 KiB on either side of the window keep their bytes (Window.wipe), the text outside the spans its own"""
    table = {}
    for lead, tail in ((0, 0), (LEAD, TAIL)):
        for f in S.fill_cases(lead, tail):
            if f.ok and len(f.doc_off) > 1:
                table["%s behind %d" % (f.name, lead)] = f

    def call(name, at):
        f = table[name]
        off, so = dev((f.doc_off + np.uint64(at)).astype(np.int64)), dev(f.span_off.astype(np.int64))
        eng.redact_spans_device(win.buf, off, so, dev(f.start), dev(f.length), f.mask)
        got = win.buf[at:at + f.blob.size].cpu().numpy().tobytes()
        return SR.differs(got, S.redact_reference(f))
    cases = []
    for k, f in table.items():
        a = (f.blob, f.doc_off, f.span_off, f.start, f.length)
        cases.append((k, f.blob[:int(f.doc_off[-1])], f.blob[int(f.doc_off[-1]):].tobytes(), span_intervals(a)))
    run_layer_a(win, cases, call, "a span")


def test_a_select(eng, win):
    table = {c.name: c for c in SD.fixed_cases() if len(c.doc_off) > 1}

    def call(name, at):
        c = table[name]
        off = dev((c.doc_off + np.uint64(at)).astype(np.int64))
        also = dev(c.also) if c.also is not None else None
        out, out_off, idx = eng.select_docs_device(win.buf, off, dev(c.rows), c.n_cols, c.want, c.mode, also)
        data, w_off, w_idx = SD.expected()[name]
        return SR.differs({"out": out.cpu().numpy().tobytes(), "out_off": out_off.cpu().tolist(), "doc_idx": idx.cpu().tolist()},
                          {"out": data, "out_off": w_off, "doc_idx": w_idx})
    cases = []
    for k, c in table.items():
        idx = SD.expected()[k][2]
        cases.append((k, np.ascontiguousarray(c.blob[:int(c.doc_off[-1])]), b"", [doc_intervals(c.doc_off)[d] for d in idx]))
    run_layer_a(win, cases, call, "a selected document")


def test_a_route(eng, win):
    # (every fixed case with documents but the two of thousands of documents, whose reference slices for seconds)
    table = {c.name: c for c in RD.fixed_cases() if len(c.doc_off) > 1 and len(c.doc_off) < 3000}

    def call(name, at):
        c = table[name]
        off = dev((c.doc_off + np.uint64(at)).astype(np.int64))
        also = dev(c.also) if c.also is not None else None
        out, out_off, idx, bd, bb = eng.route_docs_device(win.buf, off, dev(c.rows), c.n_cols, c.masks, c.mode, c.rest, also)
        data, w_off, w_idx, w_bd, w_bb = RD.expected()[name]
        return SR.differs({"out": out.cpu().numpy().tobytes(), "out_off": out_off.cpu().tolist(), "doc_idx": idx.cpu().tolist(), "bucket_doc": bd.tolist(),
                           "bucket_byte": bb.tolist()}, {"out": data, "out_off": w_off, "doc_idx": w_idx, "bucket_doc": w_bd, "bucket_byte": w_bb})
    cases = []
    for k, c in table.items():
        idx = RD.expected()[k][2]
        cases.append((k, np.ascontiguousarray(c.blob[:int(c.doc_off[-1])]), b"", [doc_intervals(c.doc_off)[d] for d in set(idx)]))
    run_layer_a(win, cases, call, "a routed document")


def test_a_to_lower(eng, win):
    """the edge batches of tolower_cases.py bare and behind five lead bytes, in front a rune's lead byte, behind a continuation byte"""
    table = {}
    for name, docs in TC.edge_batches().items():
        if name == "only_empty":
            continue
        for lead in (0, 5):
            table["%s behind %d bytes" % (name, lead)] = (docs, lead, TC.pack(docs, lead), TC.reference(docs))
    assert len(table) >= 12

    def call(name, at):
        docs, lead, (blob, off), (want, want_off) = table[name]
        o = dev((off + np.uint64(at)).astype(np.int64))
        out_off = torch.full((len(docs) + 1,), 0x5A5A, dtype=torch.int64, device="cuda")
        total = eng.to_lower_device(win.buf.data_ptr(), o.data_ptr(), len(docs), None, 0, out_off.data_ptr())
        counted = out_off.cpu().tolist()
        out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        assert eng.to_lower_device(win.buf.data_ptr(), o.data_ptr(), len(docs), out.data_ptr(), total, out_off.data_ptr()) == total
        got = out.cpu().numpy()
        if not (got[total:] == 0xA5).all():
            return "a store behind the output"
        return SR.differs({"counted": counted, "out_off": out_off.cpu().tolist(), "out": got[:total].tobytes()},
                          {"counted": [int(v) for v in want_off], "out_off": [int(v) for v in want_off], "out": want})
    cases = []
    for k, (docs, lead, (blob, off), _) in table.items():
        n = int(off[-1])
        runes = [(int(off[d]), int(off[d + 1])) for d in range(len(docs)) if max(docs[d], default=0) >= 0x80]
        cases.append((k, blob[:n], blob[n:].tobytes(), runes))
    run_layer_a(win, cases, call, "a document that leaves ASCII")


def test_a_map_spans_to_source(eng, win):
    docs, spans = LM.base_docs()
    d130 = [("É%d İ" % i).encode() for i in range(130)]
    rnd = TC.random_docs()[:300]
    piece = [d for d, _ in LM.border_docs(("piece",), every=4)]
    trip = [d for d, _ in LM.border_docs(("trip", "unit cut"), every=8)]
    none = (np.zeros(0, np.int64),) * 2
    batches = {"base": (docs, spans, 0, 0, 0), "base behind a base": (docs, spans, LEAD, TAIL, 5),
               "130 documents": (d130, [(np.array([i % 3]), np.array([2])) for i in range(130)], LEAD, TAIL, 0),
               "one document": (docs[:1], spans[:1], 0, 0, 1), "no spans": (docs, [none] * len(docs), 0, 0, 0),
               "random documents": (rnd, [LM.every_byte(d, n_random=3, seed=i) if i % 5 else none for i, d in enumerate(rnd)], 1, 1, 3),
               "runes at the piece border": (piece, [LM.every_byte(d, n_random=5, seed=i) for i, d in enumerate(piece)], 0, 0, 0),
               "runes at the trip border and the unit cut": (trip, [LM.every_byte(d, n_random=5, seed=i) for i, d in enumerate(trip)], LEAD, TAIL, 7)}
    table = {}
    for name, (ds, sp, lead, tail, doc_lead) in batches.items():
        blob, off = TC.pack(list(ds), doc_lead)
        so, st, ln = LM.flat(sp, lead, tail)
        table[name] = (blob, off, so, st, ln, LM.expected(ds, sp, lead, tail))
        assert table[name][5] is not None

    def call(name, at):
        blob, off, so, st, ln, want = table[name]
        d_st, d_ln = dev(st), dev(ln)
        eng.map_spans_to_source_device(win.buf, dev((off + np.uint64(at)).astype(np.int64)), dev(so.astype(np.int64)), d_st, d_ln)
        return SR.differs((d_st.cpu().numpy().view(np.uint32), d_ln.cpu().numpy().view(np.uint32)), want[1:])
    cases = []
    for k, (blob, off, so, st, ln, want) in table.items():
        n = int(off[-1])
        # the SOURCE spans the map answers with: where the call has to read
        cases.append((k, blob[:n], blob[n:].tobytes(), span_intervals((blob, off, so, want[1], want[2]))))
    run_layer_a(win, cases, call, "a mapped span")


class Engines:
    """an engine per (expressions, fold, position mode) of spans.py's cases"""

    def __init__(self):
        self.made = {}

    def of(self, c):
        key = (c.exprs, c.fold, c.pos_end)
        if key not in self.made:
            k = S.compiled(c.exprs, c.fold)
            e = Engine()
            e.build(k.terms, pos_end=c.pos_end)
            assert e.terms() == k.terms
            e.set_programs(k.programs, n_extra=k.n_extra)
            self.made[key] = e
        return self.made[key]

    def close(self):
        for e in self.made.values():
            e.close()


def test_a_hit_spans(win):
    pick = [c for c in S.fixed_cases() if c.docs and ("tile" in c.name or "abcd" in c.name or "lead bytes" in c.name or "fold" in c.name.lower()
                                                      or c.name.startswith("mixed documents") or "one document of" in c.name)]
    table = {c.name: c for c in pick}
    assert len(table) >= 12 and any(c.lead for c in pick) and any(c.row_idx is not None for c in pick) and any(c.pos_end for c in pick)
    es = Engines()

    def call(name, at):
        c = table[name]
        blob, off = S.packed(c)
        rows = dev(c.rows)
        idx = dev(c.row_idx.astype(np.int64)) if c.row_idx is not None else None
        so, a, b, t = es.of(c).hit_spans_device(win.buf, dev((off + np.uint64(at)).astype(np.int64)), rows, c.want, idx, fold=c.fold)
        total, w_so, w_a, w_b, w_t = S.expected()[name]
        return SR.differs({"span_off": so.cpu().tolist(), "start": a.cpu().tolist(), "len": b.cpu().tolist(), "term": t.cpu().tolist()},
                          {"span_off": w_so, "start": w_a, "len": w_b, "term": w_t})
    try:
        cases = []
        for k, c in table.items():
            blob, off = S.packed(c)
            total, so, a, b, t = S.expected()[k]
            iv = [(int(off[d]) + a[s], int(off[d]) + a[s] + b[s]) for d in range(len(c.docs)) for s in range(so[d], so[d + 1])]
            cases.append((k, blob, c.slack, iv))
        run_layer_a(win, cases, call, "a hit span")
    finally:
        es.close()


# -- scan and process: the lists, dictionaries and surroundings of placement.py
SURROUND = {"short": ("completes", 24), "long": ("neighbour", 7), "long_mixed": ("rune", 7), "long_mixed_safe": ("rune", 22), "short_mixed_safe": ("ones", 6),
            "short_mixed": ("zeros", 0)}


def placed_list(name):
    """(text with the lead, slack, doc_off) of a list of placement.py in its surroundings"""
    kind, lead_len = SURROUND[name]
    buf, off, _ = pl.placed(name, kind, 0, lead_len)
    n = int(off[-1])
    return buf[:n], buf[n:n + SLACK].tobytes(), off


def match_intervals(name, off, fold):
    mo, ti, po = pl.expected_csr(name, POS_START, fold)
    terms = sorted(set(pl.batch(name).terms))
    return [(int(off[d]) + int(po[m]), int(off[d]) + int(po[m]) + len(terms[ti[m]])) for d in range(len(off) - 1) for m in range(int(mo[d]), int(mo[d + 1]))]


def _download(ptr, dtype, n):
    a = np.zeros(max(n, 1), dtype=dtype)
    if n:
        assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.itemsize * n), C.c_int(2)) == 0
    return a[:n]


def test_a_scan(win):
    """both position modes, fold off and on; the mixed list (runes cut by borders) without folding, its fold-safe documents with"""
    runs = [("short", pl.TERMS_ASCII, (False, True)), ("long", pl.TERMS_ASCII, (False, True)), ("long_mixed", pl.TERMS_MIXED, (False,)),
            ("long_mixed_safe", pl.TERMS_MIXED, (True,)), ("short_mixed", pl.TERMS_MIXED, (False,)), ("short_mixed_safe", pl.TERMS_MIXED, (True,))]
    engines = {}
    for terms in (pl.TERMS_ASCII, pl.TERMS_MIXED):
        for m in pl.POS_MODES:
            engines[(id(terms), m)] = Engine()
            engines[(id(terms), m)].build(terms, pos_end=(m == POS_END))
    table = {name: (terms, folds, placed_list(name)) for name, terms, folds in runs}

    def call(name, at):
        terms, folds, (text, slack, off) = table[name]
        o = dev((off + np.uint64(at)).astype(np.int64))
        n = len(off) - 1
        for m in pl.POS_MODES:
            for fold in folds:
                e = engines[(id(terms), m)]
                r = e.scan_device(win.buf.data_ptr(), o.data_ptr(), n, fold=fold)
                nm = int(r.n_matches)
                got = (_download(r.match_off, np.uint64, n + 1), _download(r.term_id, np.uint32, nm), _download(r.pos, np.uint32, nm))
                try:
                    assert_csr_equal(got, pl.expected_csr(name, m, fold))
                except AssertionError as err:
                    return "%s, %s: %s" % ("end" if m == POS_END else "start", "fold" if fold else "raw", err)
        return None
    try:
        cases = [(name, text, slack, match_intervals(name, off, folds[0])) for name, (terms, folds, (text, slack, off)) in table.items()]
        run_layer_a(win, cases, call, "a match")
    finally:
        for e in engines.values():
            e.close()


@functools.lru_cache(maxsize=None)
def _programs(which):
    ids = {t.decode(): i for i, t in enumerate(sorted(set(pl.TERMS_ASCII)))}
    return [tree_to_program(dsl_ref.parse(x, True)[0], lambda lit: ids[lit]) for x in pl.expressions(which)]


@functools.lru_cache(maxsize=None)
def lowered_rows(name, which):
    """the rows of a list that leaves ASCII under the finder's case rule: strings.ToLower document by document (tolower_cases.
    ref_lower), then the oracle without folding -- the dictionary is lower-case"""
    docs = [TC.ref_lower(d) for d in pl.batch(name).docs]
    o = Oracle(pl.TERMS_ASCII)
    o.set_expressions(list(pl.expressions(which)), True)
    blob, off = pack_strings(docs)
    return o.process(blob, off, fold=False)


def test_a_process(win):
    """gft_process_device with and without folding over the ASCII lists and the fold-safe ones, in both position modes; and the
    finder over a list whose documents leave ASCII, which it lowers on the device and scans again"""
    names = ("short", "long", "short_mixed_safe", "long_mixed_safe", "short_mixed", "long_mixed")
    table = {name: placed_list(name) for name in names}
    engines = {}
    for m in pl.POS_MODES:
        for which in (pl.PRESENCE, pl.POSITIONS):
            e = Engine()
            e.build(pl.TERMS_ASCII, pos_end=(m == POS_END))
            e.set_programs(_programs(which))
            engines[(m, which)] = e
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    f.AddExpressions(list(pl.expressions(pl.POSITIONS)))
    lowered = []

    def call(name, at):
        text, slack, off = table[name]
        o = dev((off + np.uint64(at)).astype(np.int64))
        n = len(off) - 1
        if name in ("short_mixed", "long_mixed"):                   # not fold-safe: the finder's lowered path
            words = (len(pl.expressions(pl.POSITIONS)) + 31) // 32
            bm = torch.zeros((n, words), dtype=torch.int32, device="cuda")
            before = f.lowered_batches()
            f.ProcessDevice(win.buf.data_ptr(), o.data_ptr(), n, bm.data_ptr())
            lowered.append(f.lowered_batches()[0] - before[0])
            if not np.array_equal(bm.cpu().numpy().view(np.uint32), lowered_rows(name, pl.POSITIONS)):
                return "the finder's rows over the lowered batch differ"
            return None
        for (m, which), e in engines.items():
            for fold in (False, True):
                words = (len(pl.expressions(which)) + 31) // 32
                bm = torch.zeros((n, words), dtype=torch.int32, device="cuda")
                e.process_device(win.buf.data_ptr(), o.data_ptr(), n, bm.data_ptr(), fold=fold)
                if not np.array_equal(bm.cpu().numpy().view(np.uint32), pl.expected_rows(name, which, fold)):
                    return "%s, %s, %s: the rows differ" % ("end" if m == POS_END else "start", which, "fold" if fold else "raw")
        return None
    try:
        cases = [(name, text, slack, match_intervals(name, off, False)) for name, (text, slack, off) in table.items()]
        run_layer_a(win, cases, call, "a match")
        assert lowered and all(k == 1 for k in lowered), "the finder did not lower the lists that leave ASCII: %r" % lowered
    finally:
        f.close()
        for e in engines.values():
            e.close()


def test_a_filter_word_matches(eng, win):
    T = words_shape()["tile_entries"]
    table = {c.name: c for c in W.neighbour_cases() + W.border_cases(T) if c.n_docs and c.n}

    def call(name, at):
        c = table[name]
        off = dev((c.doc_off + np.uint64(at)).astype(np.int64))
        oo, p, ln, tm = eng.filter_word_matches_device(win.buf, off, dev(c.off.astype(np.int64)), dev(c.pos), None, dev(c.term), dev(c.term_len), c.pos_end)
        w_off, w_pos, w_len, w_term = c.reference()
        return SR.differs({"out_off": oo.cpu().tolist(), "pos": p.cpu().numpy().view(np.uint32), "len": ln.cpu().numpy().view(np.uint32),
                           "term": tm.cpu().numpy().view(np.uint32)},
                          {"out_off": [int(v) for v in w_off], "pos": w_pos, "len": w_len, "term": w_term})
    cases = []
    for k, c in table.items():
        n = int(c.doc_off[-1])
        iv = [(int(c.doc_off[d]) + s, int(c.doc_off[d]) + s + ln) for d, s, ln, _ in c.entries]
        cases.append((k, c.blob[:n], c.blob[n:n + SLACK].tobytes(), iv))
    run_layer_a(win, cases, call, "an entry")


def test_a_process_words(win):
    import test_gpu_words as TW
    lists = {"the documents": TW.DOCS, "reversed": TW.DOCS[::-1], "eight times": TW.DOCS * 8, "without the empty one": [d for d in TW.DOCS if d],
             "behind a long one": [b"he " * 3000 + b"she"] + TW.DOCS, "a long one between": TW.DOCS[:5] + [b"x" * 9000 + b" cat a b"] + TW.DOCS[5:]}
    table = {}
    for name, docs in lists.items():
        text = b"ab" + b"".join(docs)
        off = np.zeros(len(docs) + 1, np.uint64)
        off[0] = 2
        off[1:] = 2 + np.cumsum([len(d) for d in docs], dtype=np.uint64)
        table[name] = (docs, text, off)
    engines = {pe: TW.make_engine(pe) for pe in (False, True)}

    def call(name, at):
        docs, text, off = table[name]
        o = dev((off + np.uint64(at)).astype(np.int64))
        for pe, e in engines.items():
            for fold in (False, True):
                bm = torch.full((len(docs), 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                e.process_words_device(win.buf.data_ptr(), o.data_ptr(), len(docs), bm.data_ptr(), fold=fold)
                if not np.array_equal(bm.cpu().numpy().view(np.uint32) & 0xFF, TW.expected_rows(docs, True, fold)):
                    return "pos_end %s, fold %s: the rows differ" % (pe, fold)
        return None
    try:
        cases = []
        for k, (docs, text, off) in table.items():
            iv = [(int(off[d]) + s, int(off[d]) + s + len(t)) for d, doc in enumerate(docs) for t in TW.TERMS for s in W.occurrences(doc, t)]
            cases.append((k, text, b"cd" + b"a" * 62, iv))
        run_layer_a(win, cases, call, "an occurrence")
    finally:
        for e in engines.values():
            e.close()


# ---- layer B ---------------------------------------------------------------------------------------------------------------------------
CHUNK = 64 << 20


class Long:
    """the long batch on the device, built once in chunks of 64 MiB of positions"""

    def __init__(self):
        lb = self.lb = F.long_batch()
        self.text = torch.empty(lb.total + SLACK, dtype=torch.uint8, device="cuda")
        table = torch.frombuffer(bytearray(F.ALPHABET), dtype=torch.uint8).cuda()
        for lo in range(0, lb.total, CHUNK):
            hi = min(lo + CHUNK, lb.total)
            self.text[lo:hi] = F.filler_torch(torch.arange(lo, hi, dtype=torch.int64, device="cuda"), table)
        self.text[lb.total:] = 0
        for d, doc in enumerate(lb.docs):
            if doc.body:
                self.text[lb.off[d]:lb.off[d + 1]] = torch.frombuffer(bytearray(doc.body), dtype=torch.uint8).cuda()
            elif doc.body is None:
                for p, h in lb.hits(d):
                    self.text[p:p + len(h)] = torch.frombuffer(bytearray(h), dtype=torch.uint8).cuda()
        self.off = torch.tensor(lb.off, dtype=torch.int64, device="cuda")
        so, st, ln, ky = lb.span_arrays()
        self.so = torch.tensor(so, dtype=torch.int64, device="cuda")
        self.st, self.ln, self.ky = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (st, ln, ky))
        torch.cuda.synchronize()

    def seg_same(self, out):
        def same(at, s):
            n = F.seg_len(s)
            if s[0] == "text":
                return torch.equal(out[at:at + n], self.text[s[1]:s[2]])
            return torch.equal(out[at:at + n], torch.frombuffer(bytearray(s[1]), dtype=torch.uint8).cuda())
        return same


@pytest.fixture(scope="module")
def long():
    _release("win")
    torch.cuda.reset_peak_memory_stats()
    _HELD["long"] = Long()
    yield _HELD["long"]
    print("peak device memory of layer B: %.1f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    _release("long")


def where(call):
    at_in, at_out, delta = F.crossings(call)
    return ("%s: input position 2^32 is byte %d of island 4; the output of island 4 begins at 2^32 %+d (net change in front %+d), so output "
            "position 2^32 lies inside island 4 too: " % (call, F.TILE + 2, at_out - B, delta))


def test_b_the_text_is_the_layout(long):
    lb = long.lb
    for d in lb.long_at:                                            # samples of every long document against the numpy filler
        for p in (lb.off[d], lb.off[d] + lb.docs[d].length // 2 - 512, lb.off[d + 1] - 1024):
            assert long.text[p:p + 1024].cpu().numpy().tobytes() == lb.read(p, p + 1024).tobytes(), (d, p)
    # the comparison itself: a segment equals its own bytes and not those 2^32 further on, of the next long document or one byte on
    same = long.seg_same(long.text)
    far = lb.off[lb.long_at[4]] + 4096
    assert same(far, ("text", far, far + (1 << 20))) and not same(far, ("text", far - B, far - B + (1 << 20)))
    assert not same(far, ("text", far + 1, far + 1 + (1 << 20)))
    one, two = lb.off[lb.long_at[1]] + 4096, lb.off[lb.long_at[2]] + 4096
    assert not same(one, ("text", two, two + 4096))
    hit = lb.off[lb.long_at[0]] + 5
    assert same(hit, ("bytes", F.HIT)) and not same(hit + 1, ("bytes", F.HIT))
    d4 = lb.island_at[4]
    assert long.text[B - 64:B + 64].cpu().numpy().tobytes() == lb.docs[d4].body[B - 64 - lb.off[d4]:B + 64 - lb.off[d4]]


def test_b_mark(eng, long):
    want = F.sparse("mark")
    out, out_off, span_new, dro = eng.mark_spans_device(long.text, long.off, long.so, long.st, long.ln, F.OPEN, F.CLOSE)
    got = {"total": out.numel(), "n_runs": int(dro[-1]), "out_off": out_off.cpu().tolist(), "span_new": span_new.cpu().tolist(),
           "doc_run_off": dro.cpu().tolist()}
    d = F.compare(want, got, long.seg_same(out))
    del out
    assert d is None, where("mark") + d


def test_b_replace(eng, long):
    want = F.sparse("replace")
    t = eng.replace_spans_device(long.text, long.off, long.so, long.st, long.ln, F.REPS, long.ky, F.KEY_REP)
    got = {"total": t[0].numel(), "n_runs": int(t[2][-1])}
    got.update({k: v.cpu().tolist() for k, v in zip(R.ARRAYS, t[1:])})
    d = F.compare(want, got, long.seg_same(t[0]))
    del t
    assert d is None, where("replace") + d


def test_b_excerpt(eng, long):
    want = F.sparse("excerpt")
    t = eng.excerpt_spans_device(long.text, long.off, long.so, long.st, long.ln, F.BEFORE, F.AFTER, True)
    got = {"total": t[0].numel(), "n_exc": t[2].numel()}
    got.update({k: v.cpu().tolist() for k, v in zip(X.ARRAYS, t[1:7])})
    d = F.compare(want, got, long.seg_same(t[0]))
    assert d is None, d


def test_b_to_lower(eng, long):
    want = F.sparse("lower")
    n = long.lb.n
    out_off = torch.full((n + 1,), 0x5A5A, dtype=torch.int64, device="cuda")
    total = eng.to_lower_device(long.text.data_ptr(), long.off.data_ptr(), n, None, 0, out_off.data_ptr())
    assert total == want["total"] and out_off.cpu().tolist() == want["out_off"], where("lower") + "the count-only call"
    out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert eng.to_lower_device(long.text.data_ptr(), long.off.data_ptr(), n, out.data_ptr(), total, out_off.data_ptr()) == total
    d = F.compare(want, {"total": total, "out_off": out_off.cpu().tolist()}, long.seg_same(out))
    ok = bool((out[total:] == 0xA5).all())
    del out
    assert d is None, where("lower") + d
    assert ok, "a store behind the output"


def test_b_route(eng, long):
    want = F.sparse("route")
    rows, masks = F.route_rows(long.lb)
    out, out_off, idx, bd, bb = eng.route_docs_device(long.text, long.off, dev(rows), F.N_COLS, masks, F.ROUTE_MODE, F.ROUTE_REST)
    assert int(bb[1]) > B and int(bb[2]) > 2 * B
    got = {"total": out.numel(), "out_off": out_off.cpu().tolist(), "doc_idx": idx.cpu().tolist(), "bucket_doc": bd.tolist(), "bucket_byte": bb.tolist()}
    d = F.compare(want, got, long.seg_same(out))
    del out
    assert d is None, d


def test_b_redact_in_place(eng, long):
    """on a copy of the text: every byte outside the spans as it was, MASK over every span"""
    want = F.sparse("redact")
    copy = long.text.clone()
    eng.redact_spans_device(copy, long.off, long.so, long.st, long.ln, F.MASK)
    d = F.compare(want, {"total": long.lb.total}, long.seg_same(copy))
    ok = torch.equal(copy[long.lb.total:], long.text[long.lb.total:])
    del copy
    assert d is None, d
    assert ok, "the slack was written"


# -- the scan, the solver, the hit spans, the map and the word filter over the long batch, against the compressed twin's answers
def b_engine(pos_end=False):
    e = Engine()
    e.build(F.TERMS, pos_end=pos_end)
    ids = {t.decode(): i for i, t in enumerate(sorted(F.TERMS))}
    e.set_programs([tree_to_program(dsl_ref.parse(x, True)[0], lambda lit: ids[lit]) for x in F.EXPRS])
    return e


@pytest.mark.parametrize("pos_end", [False, True], ids=["pos_start", "pos_end"])
def test_b_scan(long, pos_end):
    e = b_engine(pos_end)
    try:
        for fold in (False, True):
            want = F.sparse_scan(pos_end, fold)
            # (with folding, the island that leaves ASCII is scanned as its bytes are: GFT_FOLD_ASCII, as the reference's bytes.lower)
            r = e.scan_device(long.text.data_ptr(), long.off.data_ptr(), long.lb.n, fold=fold)
            nm = int(r.n_matches)
            got = {"match_off": _download(r.match_off, np.uint64, long.lb.n + 1), "term_id": _download(r.term_id, np.uint32, nm),
                   "pos": _download(r.pos, np.uint32, nm)}
            d = SR.differs(got, {"match_off": want[0], "term_id": want[1], "pos": want[2]})
            assert d is None, ("fold" if fold else "raw", d)
            assert max(want[2]) > (1 << 30) - 4096                      # in-document positions near 2^30
    finally:
        e.close()


def test_b_process(long):
    want = F.sparse_rows(False)
    for pos_end in (False, True):
        e = b_engine(pos_end)
        try:
            bm = torch.zeros((long.lb.n, 1), dtype=torch.int32, device="cuda")
            e.process_device(long.text.data_ptr(), long.off.data_ptr(), long.lb.n, bm.data_ptr(), fold=False)
            got = bm.cpu().numpy().view(np.uint32)
            assert np.array_equal(got & 0xFF, want & 0xFF), (pos_end, np.nonzero(((got ^ want) & 0xFF).ravel())[0][:8].tolist())
        finally:
            e.close()


def test_b_process_lowered(long):
    """the finder's case rule: an island document leaves ASCII, so the WHOLE batch is lowered on the device and scanned again"""
    want = F.sparse_rows(True)
    assert not np.array_equal(want & 0xFF, F.sparse_rows(False) & 0xFF)
    f = Finder(GpuEngine(), EmptyRgxEngine(), False)
    try:
        f.AddExpressions(list(F.EXPRS))
        bm = torch.zeros((long.lb.n, 1), dtype=torch.int32, device="cuda")
        f.ProcessDevice(long.text.data_ptr(), long.off.data_ptr(), long.lb.n, bm.data_ptr())
        assert f.lowered_batches() == (1, 0)
        got = bm.cpu().numpy().view(np.uint32)
        assert np.array_equal(got & 0xFF, want & 0xFF), np.nonzero(((got ^ want) & 0xFF).ravel())[0][:8].tolist()
    finally:
        f.close()


def test_b_hit_spans(long):
    want = F.sparse_hit_spans(False)
    e = b_engine()
    try:
        so, st, ln, tm = e.hit_spans_device(long.text, long.off, dev(want["rows"]))
        d = SR.differs({"span_off": so.cpu().tolist(), "start": st.cpu().tolist(), "len": ln.cpu().tolist(), "term": tm.cpu().tolist()},
                       {k: want[k] for k in ("span_off", "start", "len", "term")})
        assert d is None, d
    finally:
        e.close()


def test_b_hit_spans_of_the_lowered_batch_mapped_to_the_source(eng, long):
    """to_lower_device, hit_spans_device over the lowered text, then map_spans_to_source_device over the batch itself"""
    want, mapped = F.sparse_hit_spans(True), F.sparse_mapped()
    assert mapped["start"] != want["start"] or mapped["len"] != want["len"]
    n = long.lb.n
    low_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    total = eng.to_lower_device(long.text.data_ptr(), long.off.data_ptr(), n, None, 0, low_off.data_ptr())
    low = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    assert eng.to_lower_device(long.text.data_ptr(), long.off.data_ptr(), n, low.data_ptr(), total, low_off.data_ptr()) == total
    e = b_engine()
    try:
        so, st, ln, tm = e.hit_spans_device(low, low_off, dev(want["rows"]))
        d = SR.differs({"span_off": so.cpu().tolist(), "start": st.cpu().tolist(), "len": ln.cpu().tolist(), "term": tm.cpu().tolist()},
                       {k: want[k] for k in ("span_off", "start", "len", "term")})
        del low
        assert d is None, d
        e.map_spans_to_source_device(long.text, long.off, so, st, ln)
        d = SR.differs({"start": st.cpu().tolist(), "len": ln.cpu().tolist()}, mapped)
        assert d is None, d
    finally:
        e.close()


def test_b_filter_word_matches(eng, long):
    """the batch's spans as the entries: kept and dropped ones in long_4 and in island 5 (test_far_text_host.py)"""
    want = F.sparse_words()
    oo, p, ln, tm = eng.filter_word_matches_device(long.text, long.off, long.so, long.st, long.ln)
    assert tm is None
    d = SR.differs({"out_off": oo.cpu().tolist(), "pos": p.cpu().tolist(), "len": ln.cpu().tolist()}, {k: want[k] for k in ("out_off", "pos", "len")})
    assert d is None, d
