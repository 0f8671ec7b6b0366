"""The row walk of the three document-gather calls on the device (join_bit_rows of csrc/gft_bitrows_dev.hpp under k_select_mark and
k_route_mark; the context call runs the select's mark pass) over the rows of row_widths.py: every segment width of the W <= 64 path
with and without idle lanes, both sides of the 64-word border, rows of two and three steps, a last group that is always partial, and
every word position deciding some document's verdict -- against the references of the calls' own case modules.  All comparisons
are exact."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libgft.so is loaded: one HIP runtime)

import row_widths as RW
from gofindthem_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def on_device(c):
    """(text with its 64 bytes of slack, doc_off, rows) of a case"""
    text = torch.zeros(len(c.blob) + 64, dtype=torch.uint8, device="cuda")
    if len(c.blob):
        text[:len(c.blob)] = torch.from_numpy(c.blob).cuda()
    return text, torch.from_numpy(c.doc_off.astype(np.int64)).cuda(), torch.from_numpy(c.rows.view(np.int32).copy()).cuda()


def test_the_cases_are_not_vacuous():
    assert RW.assert_not_vacuous() > 1000


def test_select_at_every_width(eng):
    for c in RW.select_cases():
        data, off, idx = RW.expected()[("select", c.name)]
        out, out_off, doc_idx = eng.select_docs_device(*on_device(c), c.n_cols, c.want, c.mode)
        assert doc_idx.cpu().tolist() == idx and out_off.cpu().tolist() == off and out.cpu().numpy().tobytes() == data, c.name


def test_context_at_every_width(eng):
    for c in RW.context_cases():
        data, off, idx, kind, group_off = RW.expected()[("context", c.name)]
        out, out_off, doc_idx, knd, goff = eng.context_docs_device(*on_device(c), c.n_cols, c.want, c.mode, None, 1, 1)
        assert doc_idx.cpu().tolist() == idx and knd.cpu().tolist() == kind and goff.cpu().tolist() == group_off, c.name
        assert out_off.cpu().tolist() == off and out.cpu().numpy().tobytes() == data, c.name


def test_route_at_every_width(eng):
    for c in RW.route_cases():
        data, off, idx, bucket_doc, bucket_byte = RW.expected()[("route", c.name)]
        out, out_off, doc_idx, bd, bb = eng.route_docs_device(*on_device(c), c.n_cols, c.masks, c.mode, c.rest)
        assert doc_idx.cpu().tolist() == idx and bd.tolist() == bucket_doc and bb.tolist() == bucket_byte, c.name
        assert out_off.cpu().tolist() == off and out.cpu().numpy().tobytes() == data, c.name
