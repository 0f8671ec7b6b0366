"""The host walks of the three document-gather calls (gft_debug_select_docs, gft_debug_context_docs, gft_debug_route_docs) over the
rows of row_widths.py: every width the device walk treats differently, every word position deciding some document's verdict, against
the references of the calls' own case modules.  No device needed.  All comparisons are exact."""
import row_widths as RW
from gofindthem_amd.engine import context_docs_host, route_docs_host, select_docs_host


def test_the_cases_are_not_vacuous():
    assert RW.assert_not_vacuous() > 1000


def test_select_host_walk():
    for c in RW.select_cases():
        data, off, idx = RW.expected()[("select", c.name)]
        m, total, out, out_off, doc_idx = select_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode)
        assert (m, total) == (len(idx), len(data)), c.name
        assert out[:total].tobytes() == data and out_off[:m + 1].tolist() == off and doc_idx[:m].tolist() == idx, c.name


def test_context_host_walk():
    for c in RW.context_cases():
        data, off, idx, kind, group_off = RW.expected()[("context", c.name)]
        m, hits, groups, total, out, out_off, doc_idx, knd, goff = context_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.want, c.mode, None, 1, 1)
        assert (m, hits, groups, total) == (len(idx), sum(kind), len(group_off) - 1, len(data)), c.name
        assert out[:total].tobytes() == data and out_off[:m + 1].tolist() == off and doc_idx[:m].tolist() == idx, c.name
        assert knd[:m].tolist() == kind and goff[:groups + 1].tolist() == group_off, c.name


def test_route_host_walk():
    for c in RW.route_cases():
        data, off, idx, bucket_doc, bucket_byte = RW.expected()[("route", c.name)]
        bd, bb, out, out_off, doc_idx = route_docs_host(c.blob, c.doc_off, c.rows, c.n_cols, c.masks, c.mode, c.rest)
        m = len(idx)
        assert bd.tolist() == bucket_doc and bb.tolist() == bucket_byte, c.name
        assert out[:len(data)].tobytes() == data and out_off[:m + 1].tolist() == off and doc_idx[:m].tolist() == idx, c.name
