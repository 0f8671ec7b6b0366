"""Every (output, input) and (output, output) pair of the resident-batch calls that refuse overlapping buffers, on the smallest batch
that has every range non-empty: 3 documents, 4 spans (or matches, or rows), every optional output present, every cap at least 2.

A call is a list of ranges -- name, input or output, bytes, element size -- written out here from the sizes include/gft.h documents
(not read from the library), and a function that makes the call from a name -> address map.  Every range has a home of its own in
one arena, SLOT bytes apart with the bytes in front of it free.  For a pair (O, X), O an output and X any other range, O is moved so
that

    (a) its last element is X's first  -> the call is refused: GFT_E_INVALID, and no byte of the arena changes (but for the route's
        two host arrays, which the call clears on entry as it clears a result word)
    (b) it ends exactly where X begins -> the call is taken, with the outputs of the disjoint call

What to expect comes from expect_refused(): an interval intersection over the ranges, which knows nothing of the library.  The host
walks (tests/test_overlap_pairs_host.py) and the device entry points (tests/test_gpu_overlap_pairs.py) share cases and pairs."""
import ctypes as C
from collections import namedtuple

import numpy as np

from gofindthem_amd import _lib

POISON = 0xA5
SELECT_ANY, SELECT_ALL, ROUTE_EVERY, ROUTE_REST, EXCERPT_WORDS = 0, 1, 1, 1, 2     # include/gft.h
SLOT, HOME = 256, 128          # range i lives at i * SLOT + HOME; [i * SLOT, i * SLOT + HOME) is free for an output moved in front

# data: an input's bytes (an output has none); step: its element size; space: "host" for what a device call takes in host memory;
# reset: the call clears it before any check, as it clears *n_selected and *total_bytes (the route's two host arrays, which
# include/gft.h says take their place): a refusal leaves zeros there and touches nothing else
Range = namedtuple("Range", "name role data nbytes step space reset")
Call = namedtuple("Call", "name ranges host device invoke")

DOCS = [b"alpha beta", b"gamma", b"delta eps"]
TEXT = np.frombuffer(b"".join(DOCS), np.uint8)
DOC_OFF = np.array([0, 10, 15, 24], np.uint64)
SPAN_OFF = np.array([0, 2, 3, 4], np.uint64)
SPAN_START = np.array([0, 6, 1, 0], np.uint32)
SPAN_LEN = np.array([5, 4, 3, 5], np.uint32)
N_DOCS, N_SPANS = 3, 4


def inp(name, a, space="dev"):
    a = np.ascontiguousarray(a)
    return Range(name, "in", a.view(np.uint8).copy(), a.nbytes, a.itemsize, space, False)


def out(name, nbytes, step, space="dev", reset=False):
    assert nbytes and nbytes % step == 0 and nbytes <= HOME
    return Range(name, "out", None, nbytes, step, space, reset)


def u64():
    return C.byref(C.c_uint64())


def span_inputs():
    return [inp("text", TEXT), inp("doc_off", DOC_OFF), inp("span_off", SPAN_OFF), inp("span_start", SPAN_START), inp("span_len", SPAN_LEN)]


def excerpt_call(snap):
    cap_bytes, cap_exc = 64, 4
    # out [cap_bytes]; exc_off, exc_span_off [cap_exc + 1] u64; exc_doc [cap_exc] u64; exc_start [cap_exc] u32; span_rel [n spans] u32;
    # doc_exc_off [n_docs + 1] u64
    ranges = span_inputs() + [out("out", cap_bytes, 1), out("exc_off", (cap_exc + 1) * 8, 8), out("exc_doc", cap_exc * 8, 8),
                              out("exc_start", cap_exc * 4, 4), out("exc_span_off", (cap_exc + 1) * 8, 8), out("span_rel", N_SPANS * 4, 4),
                              out("doc_exc_off", (N_DOCS + 1) * 8, 8)]

    def invoke(fn, p):
        flags = (EXCERPT_WORDS, 4) if snap else (0,)
        return fn(p["text"], p["doc_off"], N_DOCS, p["span_off"], p["span_start"], p["span_len"], 1, 1, *flags, p["out"], cap_bytes, p["exc_off"],
                  p["exc_doc"], p["exc_start"], p["exc_span_off"], cap_exc, p["span_rel"], p["doc_exc_off"], u64(), u64())
    if snap:
        return Call("excerpt_snap", ranges, "gft_debug_excerpt_spans_snap", "gft_excerpt_spans_snap_device", invoke)
    return Call("excerpt", ranges, "gft_debug_excerpt_spans", "gft_excerpt_spans_device", invoke)


def mark_call():
    cap_bytes = 64
    # out [cap_bytes]; out_off, doc_run_off [n_docs + 1] u64; span_new [n spans] u32
    ranges = span_inputs() + [out("out", cap_bytes, 1), out("out_off", (N_DOCS + 1) * 8, 8), out("span_new", N_SPANS * 4, 4),
                              out("doc_run_off", (N_DOCS + 1) * 8, 8)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["span_off"], p["span_start"], p["span_len"], b"<", 1, b">", 1, 0, p["out"], cap_bytes,
                  p["out_off"], p["span_new"], p["doc_run_off"], u64(), u64())
    return Call("mark", ranges, "gft_debug_mark_spans", "gft_mark_spans_device", invoke)


def replace_call():
    cap_bytes, cap_runs = 64, 4
    key_rep = np.array([1, 0], np.uint32)
    rep_bytes = np.frombuffer(b"XYZ", np.uint8).copy()
    rep_off = np.array([0, 1, 3], np.uint64)
    # span_key [n spans] u32 is an input; out [cap_bytes]; out_off, doc_run_off [n_docs + 1] u64; run_new, run_len, run_rep [cap_runs] u32
    ranges = span_inputs() + [inp("span_key", np.array([0, 1, 1, 0], np.uint32)), out("out", cap_bytes, 1), out("out_off", (N_DOCS + 1) * 8, 8),
                              out("doc_run_off", (N_DOCS + 1) * 8, 8), out("run_new", cap_runs * 4, 4), out("run_len", cap_runs * 4, 4),
                              out("run_rep", cap_runs * 4, 4)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["span_off"], p["span_start"], p["span_len"], p["span_key"], key_rep.ctypes.data, 2,
                  rep_bytes.ctypes.data, rep_off.ctypes.data, 2, 0, p["out"], cap_bytes, p["out_off"], p["doc_run_off"], p["run_new"], p["run_len"],
                  p["run_rep"], cap_runs, u64(), u64())
    return Call("replace", ranges, "gft_debug_replace_spans", "gft_replace_spans_device", invoke)


BITMAP = np.array([3, 1, 2], np.uint32)          # n_cols = 2: one word a row
ALSO = np.array([0, 1, 0], np.uint8)


def doc_inputs():
    return [inp("text", TEXT), inp("doc_off", DOC_OFF), inp("bitmap", BITMAP), inp("also", ALSO)]


def select_call():
    cap_bytes, cap_docs = 64, 3
    # bitmap [n_docs][ceil(n_cols / 32)] u32; also [n_docs] bytes; out [cap_bytes]; out_off [cap_docs + 1] u64; doc_idx [cap_docs] u64
    ranges = doc_inputs() + [out("out", cap_bytes, 1), out("out_off", (cap_docs + 1) * 8, 8), out("doc_idx", cap_docs * 8, 8)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["bitmap"], 2, None, SELECT_ANY, p["also"], p["out"], cap_bytes, p["out_off"],
                  p["doc_idx"], cap_docs, u64(), u64())
    return Call("select", ranges, "gft_debug_select_docs", "gft_select_docs_device", invoke)


def route_call():
    cap_bytes, cap_docs, n_buckets = 64, 6, 2
    B = n_buckets + 1                               # GFT_ROUTE_REST: one bucket more
    # masks [n_buckets][W] u32, bucket_doc and bucket_byte [B + 1] u64: host memory in the device call as well
    ranges = doc_inputs() + [inp("masks", np.array([1, 2], np.uint32), "host"), out("out", cap_bytes, 1), out("out_off", (cap_docs + 1) * 8, 8),
                             out("doc_idx", cap_docs * 8, 8), out("bucket_doc", (B + 1) * 8, 8, "host", True),
                             out("bucket_byte", (B + 1) * 8, 8, "host", True)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["bitmap"], 2, p["masks"], n_buckets, ROUTE_EVERY, ROUTE_REST, p["also"],
                  p["out"], cap_bytes, p["out_off"], p["doc_idx"], cap_docs, p["bucket_doc"], p["bucket_byte"])
    return Call("route", ranges, "gft_debug_route_docs", "gft_route_docs_device", invoke)


def context_call():
    cap_bytes, cap_docs, cap_groups = 64, 3, 2
    # fence [n_docs] bytes; kind [cap_docs] bytes; group_off [cap_groups + 1] u64
    ranges = doc_inputs() + [inp("fence", np.array([0, 0, 1], np.uint8)), out("out", cap_bytes, 1), out("out_off", (cap_docs + 1) * 8, 8),
                             out("doc_idx", cap_docs * 8, 8), out("kind", cap_docs, 1), out("group_off", (cap_groups + 1) * 8, 8)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["bitmap"], 2, None, SELECT_ALL, p["also"], 1, 1, p["fence"], p["out"], cap_bytes,
                  p["out_off"], p["doc_idx"], p["kind"], cap_docs, p["group_off"], cap_groups, u64(), u64(), u64(), u64())
    return Call("context", ranges, "gft_debug_context_docs", "gft_context_docs_device", invoke)


def words_call():
    cap = 4
    # the list: off [n_docs + 1] u64; pos, len, term [n entries] u32; the outputs: out_off [n_docs + 1] u64; out_pos, out_len, out_term [cap] u32
    ranges = [inp("text", TEXT), inp("doc_off", DOC_OFF), inp("off", SPAN_OFF), inp("pos", SPAN_START), inp("len", SPAN_LEN),
              inp("term", np.array([0, 1, 2, 3], np.uint32)), out("out_off", (N_DOCS + 1) * 8, 8), out("out_pos", cap * 4, 4), out("out_len", cap * 4, 4),
              out("out_term", cap * 4, 4)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["off"], p["pos"], p["len"], p["term"], None, 4, 0, p["out_off"], p["out_pos"], p["out_len"],
                  p["out_term"], cap, u64())
    return Call("words", ranges, "gft_debug_filter_word_matches", "gft_filter_word_matches_device", invoke)


def stats_call():
    n_terms = 2
    # off [n_docs + 1] u64; term [n entries] u32; occ, docs, first [n_terms] u64
    ranges = [inp("off", SPAN_OFF), inp("term", np.array([0, 1, 1, 0], np.uint32)), out("occ", n_terms * 8, 8), out("docs", n_terms * 8, 8),
              out("first", n_terms * 8, 8)]

    def invoke(fn, p):
        return fn(p["off"], p["term"], N_DOCS, n_terms, 0, 0, p["occ"], p["docs"], p["first"])
    return Call("term_stats", ranges, "gft_debug_term_stats", "gft_term_stats_device", invoke)


def columns_call():
    n_rows, n_cols = 4, 2
    # bitmap [n_rows][ceil(n_cols / 32)] u32 (no row_idx: the rows are the first n_rows); count [n_cols] u64
    ranges = [inp("bitmap", np.array([3, 1, 2, 3], np.uint32)), out("count", n_cols * 8, 8)]

    def invoke(fn, p):
        return fn(p["bitmap"], n_rows, n_cols, None, 0, p["count"])
    return Call("columns", ranges, "gft_debug_count_columns", "gft_count_columns_device", invoke)


def spans_call():
    cap, n_exprs = 4, 2
    term_len = np.array([5, 4], np.uint32)
    wit_off = np.array([0, 1, 2], np.uint64)          # term 0 is a witness of expression 0, term 1 of expression 1
    wit_expr = np.array([0, 1], np.uint32)
    # the walk behind the scan: match_off [n_docs + 1] u64; term_id, pos [n matches] u32; bitmap [n_docs][ceil(n_exprs / 32)] u32;
    # span_off [n_docs + 1] u64; span_start, span_len, span_term [cap] u32.  (the device call scans a text first: host walk only)
    ranges = [inp("match_off", SPAN_OFF), inp("term_id", np.array([0, 1, 0, 1], np.uint32)), inp("pos", SPAN_START), inp("bitmap", BITMAP),
              out("span_off", (N_DOCS + 1) * 8, 8), out("span_start", cap * 4, 4), out("span_len", cap * 4, 4), out("span_term", cap * 4, 4)]

    def invoke(fn, p):
        return fn(p["match_off"], p["term_id"], p["pos"], N_DOCS, term_len.ctypes.data, 0, wit_off.ctypes.data, wit_expr.ctypes.data, p["bitmap"],
                  n_exprs, None, None, p["span_off"], p["span_start"], p["span_len"], p["span_term"], cap, u64())
    return Call("hit_spans", ranges, "gft_debug_hit_spans", None, invoke)


def lower_call():
    cap = 64
    docs = ["Alpha BETA".encode(), "École À".encode(), "Édelta EPS".encode()]
    text = np.frombuffer(b"".join(docs), np.uint8)
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    # out [cap]; out_off [n_docs + 1] u64
    ranges = [inp("text", text), inp("doc_off", off), out("out", cap, 1), out("out_off", (N_DOCS + 1) * 8, 8)]

    def invoke(fn, p):
        return fn(p["text"], p["doc_off"], N_DOCS, p["out"], cap, p["out_off"], u64())
    return Call("to_lower", ranges, "gft_debug_emulate_to_lower", "gft_to_lower_device", invoke)


CALLS = [excerpt_call(False), excerpt_call(True), mark_call(), replace_call(), select_call(), route_call(), context_call(), words_call(),
         stats_call(), columns_call(), spans_call(), lower_call()]


# ---- where the ranges are, and what that means -----------------------------------------------------------------------------------
def homes(call):
    return {r.name: i * SLOT + HOME for i, r in enumerate(call.ranges)}


def arena_bytes(call):
    return (len(call.ranges) + 1) * SLOT


def meet(a0, an, b0, bn):
    return an > 0 and bn > 0 and a0 < b0 + bn and b0 < a0 + an


def expect_refused(call, at):
    """an output meets an input or another output: intervals [at, at + nbytes), nothing else"""
    outs = [r for r in call.ranges if r.role == "out"]
    return any(meet(at[o.name], o.nbytes, at[x.name], x.nbytes) for o in outs for x in call.ranges if x is not o)


def variants(call, spaces=None):
    """(label, at, refused) for every ordered pair (output O, other range X) and both moves of O.  spaces: the address spaces the
    ranges live in when there are two (a device call's host arguments): a pair across them cannot be made to meet"""
    for o in call.ranges:
        if o.role != "out":
            continue
        for x in call.ranges:
            if x is o or (spaces and spaces[o.name] != spaces[x.name]):
                continue
            for kind, back in (("a", o.nbytes - o.step), ("b", o.nbytes)):
                at = homes(call)
                at[o.name] = at[x.name] - back
                refused = expect_refused(call, at)
                # (a) shares O's last element with X's first and nothing else; (b) shares nothing and leaves no gap
                assert refused == (kind == "a") and at[o.name] % o.step == 0
                assert at[o.name] + o.nbytes == at[x.name] + (o.step if kind == "a" else 0)
                yield "%s: %s %s %s" % (call.name, o.name, "onto" if kind == "a" else "up to", x.name), at, refused


def n_pairs(call):
    outs = sum(r.role == "out" for r in call.ranges)
    return outs * (len(call.ranges) - 1)


def prepare(call, at, size):
    """the arena's bytes before the call: poison, then every input at its place"""
    a = np.full(size, POISON, np.uint8)
    for r in call.ranges:
        if r.role == "in":
            a[at[r.name]:at[r.name] + r.nbytes] = r.data
    return a


def outputs(call, at, after):
    return {r.name: after[at[r.name]:at[r.name] + r.nbytes].copy() for r in call.ranges if r.role == "out"}


def check(call, label, at, refused, rc, before, after, base):
    if refused:
        assert rc == _lib.GFT_E_INVALID, "%s: rc %d" % (label, rc)
        want = before.copy()
        for r in call.ranges:
            if r.reset:
                want[at[r.name]:at[r.name] + r.nbytes] = 0
        assert np.array_equal(want, after), "%s: a refused call wrote" % label
        return
    assert rc == 0, "%s: rc %d" % (label, rc)
    got = outputs(call, at, after)
    for name, want in base.items():
        assert np.array_equal(got[name], want), "%s: %s differs from the disjoint call's" % (label, name)
    for r in call.ranges:
        if r.role == "in":
            assert np.array_equal(after[at[r.name]:at[r.name] + r.nbytes], r.data), "%s: input %s changed" % (label, r.name)


def run_host(call, at):
    """the host walk on one numpy arena: (rc, bytes before, bytes after)"""
    before = prepare(call, at, arena_bytes(call))
    arena = before.copy()
    rc = call.invoke(getattr(_lib.load(), call.host), {n: arena.ctypes.data + o for n, o in at.items()})
    return rc, before, arena


def host_base(call):
    rc, before, after = run_host(call, homes(call))
    assert rc == 0, "%s: the disjoint call is refused: %d" % (call.name, rc)
    base = outputs(call, homes(call), after)
    assert any((v != POISON).any() for v in base.values()), "%s: the disjoint call wrote nothing" % call.name
    return base
