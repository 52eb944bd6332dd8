"""The task lists pcodec_amd.paged builds for an index with histories (include/pco_gfx.h section 4j), under the stand-ins for torch and the library of
tests/paged_plan_util.py: index_pages(history=True) is ONE pco_gfx_index_pages_hist call with a [k, stride] tensor per page of a chunk under Lookback,
and decompress_chunks_from / decompress_rows_from with histories= are ONE pco_gfx_decompress_page_reads_hist call whose segment s starts from cursor
s - 1 AND history s - 1, with to == NULL.  What the ChunkMeta says (the one read from the device) is given here: chunk 0 and chunk 2 are under Lookback."""
import sys

import pytest

import paged_plan_util as U
from pcodec_amd import _lib as G
from pcodec_amd import build as B

HISTORY_BYTES = {0: 64 + 4 * 16, 1: 0, 2: 64 + 2 * 2 + 2}   # chunk 2's is no multiple of 8: the stride is rounded up
STRIDE = {c: (b + 7) // 8 * 8 for c, b in HISTORY_BYTES.items()}
EVERY = 256


@pytest.fixture()
def stand_ins(monkeypatch):
    if B.needs_build():
        B.build()
    from pcodec_amd import paged
    G.lib()
    real_torch = sys.modules.get("torch")
    torch = sys.modules["torch"] = U.FakeTorch()
    lib = U.FakeLib(G)
    monkeypatch.setattr(paged, "_require_device", lambda: lib)
    monkeypatch.setattr(paged._BlobPages, "history_bytes", lambda self, L, blob, c: HISTORY_BYTES[c])
    pieces, total = U.directory(0)
    blob = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    try:
        yield paged, lib, blob, pieces
    finally:
        if real_torch is None:
            sys.modules.pop("torch", None)
        else:
            sys.modules["torch"] = real_torch


def pages():
    """(chunk, page index, page_n, k) in the index's order"""
    return [(c, i, n, max((n - 1) // EVERY, 0)) for c, ns in enumerate(U.PAGE_NS) for i, n in enumerate(ns)]


def names(struct):
    return [n for n, _ in struct._fields_]


def test_index_pages_with_histories_is_one_call_with_a_tensor_per_lookback_page(stand_ins):
    paged, lib, blob, pieces = stand_ins
    idx = paged.index_pages(blob, pieces, U.DTYPES, EVERY, history=True)
    assert [c["fn"] for c in lib.calls] == ["pco_gfx_index_pages_hist"] and lib.calls[0]["n_tasks"] == len(pages()) == len(idx) == len(idx.histories)
    assert lib.calls[0]["args"][0] == 0 and lib.calls[0]["args"][1] is None and lib.calls[0]["args"][2] == idx.results.data_ptr()   # flags, no host results, d_results
    f = names(G.PageIndexHistTask)
    for (c, i, n, k), pc, h, task in zip(pages(), idx, idx.histories, lib.calls[0]["tasks"]):
        t = dict(zip(f, task))
        assert (pc.chunk, pc.piece, pc.every_rows, pc.cursors.shape) == (c, i + 1, EVERY, (k, 256)) and len(pc) == 4
        assert (t["page_n"], t["every_rows"], t["cursors"]) == (n, EVERY, pc.cursors.data_ptr() if k else None)
        if STRIDE[c]:
            assert h.shape == (k, STRIDE[c]) and (t["histories"], t["history_stride"]) == ((h.data_ptr(), STRIDE[c]) if k else (None, 0))
        else:
            assert h is None and (t["histories"], t["history_stride"]) == (None, 0)
    lib.calls.clear()
    paged.index_pages(blob, pieces, U.DTYPES, EVERY, general=True, history=True)
    assert lib.calls[0]["fn"] == "pco_gfx_index_pages_hist" and lib.calls[0]["args"][0] == G.CURSOR_GENERAL
    lib.calls.clear()
    assert paged.index_pages(blob, pieces, U.DTYPES, EVERY).histories is None and lib.calls[0]["fn"] == "pco_gfx_index_pages"


def test_segments_start_from_cursor_and_history_s_minus_1_and_leave_the_pair(stand_ins):
    paged, lib, blob, pieces = stand_ins
    idx = paged.index_pages(blob, pieces, U.DTYPES, EVERY, history=True)
    lib.calls.clear()
    outs = paged.decompress_chunks_from(blob, pieces, U.DTYPES, idx, histories=idx.histories)
    assert [c["fn"] for c in lib.calls] == ["pco_gfx_decompress_page_reads_hist"] and lib.calls[0]["args"][0] == 0 and lib.calls[0]["args"][1] == "host"
    f = names(G.PageReadHistTask)
    tasks = [dict(zip(f, t)) for t in lib.calls[0]["tasks"]]
    at = 0
    for (c, i, n, k), pc, h in zip(pages(), idx, idx.histories):
        for s, row in enumerate(range(0, n, EVERY)):
            t = tasks[at]; at += 1
            assert (t["page_n"], t["first"], t["count"], t["to"]) == (n, row, min(EVERY, n - row), None)
            assert t["from_"] == (pc.cursors.data_ptr() + (s - 1) * 256 if s else None)
            assert (t["history"], t["history_len"]) == ((h.data_ptr() + (s - 1) * STRIDE[c], STRIDE[c]) if s and h is not None else (None, 0)), (c, i, s)
    assert at == len(tasks) and [o.shape[0] for o in outs] == [sum(ns) for ns in U.PAGE_NS]
    # rows: one task per page the interval touches, from the last pair at or in front of its first row
    lib.calls.clear()
    paged.decompress_rows_from(blob, pieces, U.DTYPES, idx, [(990, 2100), None, (0, 1)], histories=idx.histories)
    assert [c["fn"] for c in lib.calls] == ["pco_gfx_decompress_page_reads_hist"]
    got = [(t["page_n"], t["first"], t["count"], t["from_"], t["to"], t["history"], t["history_len"]) for t in (dict(zip(f, x)) for x in lib.calls[0]["tasks"])]
    c0, h0 = [pc.cursors.data_ptr() for pc in idx[:3]], [h.data_ptr() for h in idx.histories[:3]]
    assert got == [(1000, 990, 10, c0[0] + 2 * 256, None, h0[0] + 2 * STRIDE[0], STRIDE[0]), (999, 0, 999, None, None, None, 0),
                   (257, 0, 101, None, None, None, 0), (1, 0, 1, None, None, None, 0)]
    # without histories= the calls are what they were
    lib.calls.clear()
    paged.decompress_chunks_from(blob, pieces, U.DTYPES, idx)
    assert [c["fn"] for c in lib.calls] == ["pco_gfx_decompress_page_reads"]
    with pytest.raises(ValueError):
        paged.decompress_chunks_from(blob, pieces, U.DTYPES, idx, histories=idx.histories[:2])
