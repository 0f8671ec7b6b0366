"""A blob cut into line documents, the host half: gft_debug_split_lines -- the kernels' walk (csrc/gft_split_piece.hpp) tile by tile
on the host, with their carry resolution -- against the reference of split_lines.py on every fixed and random case in both modes,
the cap protocol, the refusals, and the group finder's JSON Lines call on a finder that takes the host route.  No GPU needed."""
import ctypes as C
import json

import numpy as np
import pytest

import split_lines as S
from gofindthem_amd import _lib, group
from gofindthem_amd.engine import GftError, split_lines_host, split_shape
from gofindthem_amd.finder import Finder, Match, SubstringEngine

GUARD = 0xA5A5A5A5A5A5A5A5
MODES = [S.AFTER_NL, S.JSON_LINES]


def test_symbols_and_shape():
    L = _lib.load()
    for name in ("gft_split_lines_device", "gft_debug_split_lines", "gft_debug_split_shape", "gft_finder_split_lines_device",
                 "gft_group_process_json_lines"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    T, K = split_shape()
    assert T >= 1024 and T % 1024 == 0 and K >= 2


def check(name, blob, mode, want):
    n, off = split_lines_host(blob, mode, guard=4)
    assert n == len(want) - 1, (name, mode)
    assert off[:n + 1].tolist() == want, (name, mode)
    assert (off[n + 1:] == GUARD).all(), (name, mode)


@pytest.mark.parametrize("mode", MODES)
def test_fixed_cases(mode):
    want = S.expected("fixed")
    for name, blob in S.fixed_cases():
        check(name, blob, mode, want[name, mode])


@pytest.mark.parametrize("mode", MODES)
def test_random_blobs(mode):
    want = S.expected("random")
    assert len(S.random_cases()) == 200
    for name, blob in S.random_cases():
        check(name, blob, mode, want[name, mode])


def test_the_reference_on_the_contract_examples():
    """the reference itself, on cases small enough to read"""
    assert S.reference(b"", 0) == [0] and S.reference(b"", 1) == [0]
    assert S.reference(b"a\nb", 0) == [0, 2, 3] and S.reference(b"a\nb\n", 0) == [0, 2, 4] and S.reference(b"\n\n", 0) == [0, 1, 2]
    assert S.reference(b" \n\t\r\n", 1) == [0]
    assert S.reference(b"\n \n{}\r\n\n  []\n \n", 1) == [0, 8, 15]
    assert S.documents(b"\n \n{}\r\n\n  []\n \n", 1) == [b"\n \n{}\r\n\n", b"  []\n \n"]
    assert S.sparse_reference(100, {10: 10, 20: ord("{"), 30: 10, 99: 10}, 0) == [0, 11, 31, 100]
    assert S.sparse_reference(100, {10: 10, 20: ord("{"), 30: 10, 50: ord("{"), 60: ord("{")}, 1) == [0, 31, 100]


@pytest.mark.parametrize("mode", MODES)
def test_cap_protocol(mode):
    blob = b'{"a":1}\n \n{"b":2}\r\n[]\n'
    want = S.reference(blob, mode)
    n = len(want) - 1
    assert split_lines_host(blob, mode, cap=0)[0] == n                     # count only
    got, off = split_lines_host(blob, mode, cap=n, guard=4)                # one short: entry n is not written
    assert got == n and off[:n].tolist() == want[:n] and (off[n:] == GUARD).all()
    got, off = split_lines_host(blob, mode, cap=1, guard=4)
    assert got == n and off[0] == 0 and (off[1:] == GUARD).all()
    got, off = split_lines_host(b" \n ", S.JSON_LINES, cap=3, guard=2)       # no document: entry 0 alone
    assert got == 0 and off[0] == 0 and (off[1:] == GUARD).all()


def test_refusals():
    L = _lib.load()
    n = C.c_uint64(7)
    a = np.frombuffer(b"abc\n", dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    assert L.gft_debug_split_lines(a.ctypes.data, 4, 2, out.ctypes.data, 4, C.byref(n)) == _lib.GFT_E_INVALID       # unknown mode
    assert L.gft_debug_split_lines(None, 4, 0, out.ctypes.data, 4, C.byref(n)) == _lib.GFT_E_INVALID                # no blob
    assert L.gft_debug_split_lines(a.ctypes.data, 4, 0, None, 4, C.byref(n)) == _lib.GFT_E_INVALID                  # a cap, no array
    assert L.gft_debug_split_lines(a.ctypes.data, 4, 0, out.ctypes.data, 4, None) == _lib.GFT_E_INVALID
    both = np.zeros(64, dtype=np.uint8)                                                                               # output over the input
    assert L.gft_debug_split_lines(both.ctypes.data, 64, 0, both.ctypes.data + 8, 4, C.byref(n)) == _lib.GFT_E_INVALID
    assert L.gft_debug_split_lines(a.ctypes.data, 4, 0, out.ctypes.data, 4, C.byref(n)) == 0 and n.value == 1
    with pytest.raises(GftError):
        split_lines_host(b"x", 5)


# ---- the callers on a finder that takes the host route ------------------------------------------------------------------------
class NaiveEngine(SubstringEngine):
    """an injected substring engine: the group finder then walks and splits on the host"""

    def BuildEngine(self, keywords, caseSensitive):
        self.keywords = list(keywords)

    def FindSubstrings(self, text):
        out = []
        for k in self.keywords:
            at = text.find(k)
            while at >= 0:
                out.append(Match(len(text[:at].encode("utf-8", "surrogateescape")), k))
                at = text.find(k, at + 1)
        return out


LINES = (b'\n  \r\n{"title": "alpha beta", "n": 1}\r\n\n   {"title": "gamma", "body": {"text": "beta"}}\n{"title": \n'
         b'\t[1, 2, {"title": "alpha"}]\n \n{"n": [5, null]}\n"beta"')
RULES = {"ab": ['"t1" and "t2"'], "only a": ['"t1" and not "t2"'], "none": ['not "t1"']}


def host_group(schema=None):
    f = Finder(NaiveEngine(), None, False, allow_no_device=True)
    f.AddExpressionWithTag('"alpha"', "t1")
    f.AddExpressionWithTag('"beta"', "t2")
    g = group.NewFinderWithRules(f, RULES)
    if schema is not None:
        g.SetSchema(schema)
    return g


def test_process_json_lines_on_the_host_route():
    docs = S.documents(LINES, S.JSON_LINES)
    assert len(docs) == 6 and b"".join(docs) == LINES
    g = host_group()
    want = g.ProcessJsons(docs)
    assert g.ProcessJsonLines(LINES) == want
    assert g.json_last() == (0, 6)
    # (a document with string values needs the device for its leaves: without one it is an error on both sides)
    assert "error" in want[2] and want[4] == {"rules": {"none": ['not "t1"']}}
    assert g.ProcessJsonLines(LINES, ["title"], None) == g.ProcessJsons(docs, ["title"], None)
    assert g.ProcessJsonLines(b"") == [] and g.ProcessJsonLines(b" \n\r\n") == []
    assert json.loads(json.dumps(g.ProcessJsonLines(b"{}"))) == [{"rules": {"none": ['not "t1"']}}]


def test_process_json_lines_with_a_schema_on_the_host_route():
    g = host_group(["title", "body.text"])
    docs = S.documents(LINES, S.JSON_LINES)
    assert g.ProcessJsonLines(LINES) == g.ProcessJsons(docs)
    with pytest.raises(group.GroupFinderError) as e:
        g.ProcessJsonLines(LINES, ["title"], None)
    assert e.value.code == _lib.GFT_E_INVALID
    assert g.ProcessJsonLines(LINES) == g.ProcessJsons(docs)             # the handle goes on answering
