"""pco_gfx_decompress_page_ranges without a device: the task struct of the ctypes binding against the header, the argument checks (made before
anything is launched, and before a device is asked for), and the interval-to-page mapping of paged.decompress_rows as a pure function."""
import ctypes as C
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402

HEADER = os.path.join(HERE, "..", "include", "pco_gfx.h")
C_TYPES = {"const void*": C.c_void_p, "void*": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}


def header_fields():
    text = open(HEADER).read()
    body = re.search(r"typedef struct PcoGfxPageRangeTask \{(.*?)\} PcoGfxPageRangeTask;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const void\*|void\*|uint64_t|uint32_t)\s+(.*)", decl)
        assert m, decl
        for name in m.group(2).split(","):
            out.append((name.strip(), C_TYPES[m.group(1)]))
    return out


def test_the_binding_lays_the_task_out_as_the_header_does():
    want = header_fields()
    assert [n for n, _ in want] == ["meta", "meta_len", "page", "page_len", "dst", "page_n", "first", "count", "dtype", "format_major"]
    assert [(n, t) for n, t in G.PageRangeTask._fields_] == want
    assert C.sizeof(G.PageRangeTask) == 72
    offs = {n: getattr(G.PageRangeTask, n).offset for n, _ in want}
    assert offs == {"meta": 0, "meta_len": 8, "page": 16, "page_len": 24, "dst": 32, "page_n": 40, "first": 48, "count": 56, "dtype": 64, "format_major": 68}


def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    assert re.search(r"enum PcoError pco_gfx_decompress_page_ranges\(size_t n_tasks, const PcoGfxPageRangeTask\* tasks", open(HEADER).read())
    assert hasattr(G.lib(), "pco_gfx_decompress_page_ranges")


def call(task):
    L = G.lib()
    arr = (G.PageRangeTask * 1)(task); res = (G.TaskResult * 1)()
    res[0].n_out = 77; res[0].status = 99
    code = L.pco_gfx_decompress_page_ranges(1, arr, res, None, None)
    return code, L.pco_gfx_last_status(), res[0]


P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)


@pytest.mark.parametrize("task,status", [
    (dict(first=5, count=6, page_n=10), G.ST_INVALID_ARGUMENT),            # first + count > page_n
    (dict(first=11, count=0, page_n=10), G.ST_INVALID_ARGUMENT),
    (dict(first=(1 << 64) - 1, count=2, page_n=10), G.ST_INVALID_ARGUMENT),  # the sum wraps
    (dict(page_n=0, first=0, count=0), G.ST_INVALID_ARGUMENT),
    (dict(page_n=(1 << 24) + 1), G.ST_INVALID_ARGUMENT),
    (dict(meta=None), G.ST_INVALID_ARGUMENT),
    (dict(page=None), G.ST_INVALID_ARGUMENT),
    (dict(dst=None, count=1), G.ST_INVALID_ARGUMENT),
    (dict(dtype=0), G.ST_INVALID_ARGUMENT),
    (dict(format_major=5), G.ST_CORRUPTION),
])
def test_argument_checks_come_before_anything_else(task, status):
    kw = dict(meta=P, meta_len=10, page=P, page_len=10, dst=P, page_n=10, first=0, count=1, dtype=1, format_major=4)
    kw.update(task)
    code, st, res = call(G.PageRangeTask(**kw))
    assert code == G.PcoDecompressionError and st == status
    assert res.n_out == 77 and res.status == 99   # nothing was written


def test_no_tasks_is_a_success_without_a_device():
    assert G.lib().pco_gfx_decompress_page_ranges(0, None, None, None, None) == G.PcoSuccess


def test_rows_map_onto_the_pages_they_touch():
    ns = [1000, 3000, 500]
    m = paged.map_rows_to_pages
    assert m(ns, 10, 20) == [(0, 10, 10, 0)]                                  # inside one page
    assert m(ns, 990, 1010) == [(0, 990, 10, 0), (1, 0, 10, 10)]              # across two
    assert m(ns, 999, 4001) == [(0, 999, 1, 0), (1, 0, 3000, 1), (2, 0, 1, 3001)]   # across three
    assert m(ns, 1000, 1001) == [(1, 0, 1, 0)]                                # starting exactly at a page boundary
    assert m(ns, 0, 1000) == [(0, 0, 1000, 0)]                                # ending exactly at one: the next page gets no task
    assert m(ns, 0, 4500) == [(0, 0, 1000, 0), (1, 0, 3000, 1000), (2, 0, 500, 4000)]
    assert m(ns, 1234, 1234) == [] and m(ns, 4500, 4500) == [] and m([], 0, 0) == []
    for bad in ((5, 4), (0, 4501), (-1, 3)):
        with pytest.raises(ValueError):
            m(ns, *bad)
