"""pco_gfx_index_pages (include/pco_gfx.h section 4g) without a device: the struct of the ctypes binding against the header, the two exports,
pco_gfx_page_index_len against its one-line definition, the argument checks (made before anything is launched, and before a device is asked
for), and the slot arithmetic of pcodec_amd/csrc/pco_index.h compiled on its own with g++ (the same lines the index walker and expander run
per batch) against a plain Python restatement."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import test_page_reads_abi as A  # noqa: E402  (header_fields: a struct's fields as the header declares them)
from pcodec_amd import _lib as G  # noqa: E402

NO_SLOT = 0xFFFFFFFF


def restated_len(page_n, every_rows):
    """k = (page_n - 1) / every_rows; 0 for page_n == 0 or > 2^24, every_rows == 0 or not a multiple of 256"""
    if page_n == 0 or page_n > 1 << 24 or every_rows == 0 or every_rows % 256:
        return 0
    return (page_n - 1) // every_rows


def restated_slot(batches_done, every_batches, k):
    """cursor i stands behind (i + 1) * every_batches batches, for i < k"""
    for i in range(k):
        if batches_done == (i + 1) * every_batches:
            return i
    return NO_SLOT


# ---------------------------------------------------------------------------------------------------------------------------------------
# the struct and the exports
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_lays_the_index_task_out_as_the_header_does():
    want = A.header_fields("PcoGfxPageIndexTask")
    assert [n for n, _ in want] == ["meta", "meta_len", "page", "page_len", "cursors", "page_n", "every_rows", "dtype", "format_major"]
    assert G.PageIndexTask._fields_ == want
    assert C.sizeof(G.PageIndexTask) == 64
    at = 0
    for n, t in G.PageIndexTask._fields_:
        assert getattr(G.PageIndexTask, n).offset == at, n
        at += C.sizeof(t)
    assert at == 64
    assert [getattr(G.PageIndexTask, n).offset for n, _ in G.PageIndexTask._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60]


def test_the_header_declares_both_functions_and_the_library_exports_them():
    text = open(A.HEADER).read()
    assert re.search(r"size_t pco_gfx_page_index_len\(uint64_t page_n, uint64_t every_rows\);", text)
    assert re.search(r"enum PcoError pco_gfx_index_pages\(size_t n_tasks, const PcoGfxPageIndexTask\* tasks, PcoGfxTaskResult\* results, PcoGfxTaskResult\* d_results,\s+void\* stream\);", text)
    L = G.lib()
    assert hasattr(L, "pco_gfx_page_index_len") and hasattr(L, "pco_gfx_index_pages")


@pytest.mark.parametrize("every_rows", [0, 100, 256, 512, 1 << 24])
def test_index_len_is_its_definition(every_rows):
    L = G.lib()
    for page_n in (0, 1, 255, 256, 257, 512, 513, 1 << 24, (1 << 24) + 1):
        assert L.pco_gfx_page_index_len(page_n, every_rows) == restated_len(page_n, every_rows), (page_n, every_rows)
    assert [restated_len(n, 256) for n in (0, 1, 255, 256, 257, 512, 513, 1 << 24, (1 << 24) + 1)] == [0, 0, 0, 0, 1, 1, 2, 65535, 0]   # (the restatement, written out once)


# ---------------------------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
GOOD_TASK = dict(meta=P, meta_len=10, page=P, page_len=10, cursors=P, page_n=1000, every_rows=256, dtype=1, format_major=4)


def call(task=None, no_tasks=False, no_results=False):
    L = G.lib()
    kw = dict(GOOD_TASK); kw.update(task or {})
    arr = (G.PageIndexTask * 1)(G.PageIndexTask(**kw))
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    code = L.pco_gfx_index_pages(1, None if no_tasks else arr, None if no_results else res, None, None)
    return code, L.pco_gfx_last_status(), res[0]


CHECKS = [
    (dict(no_tasks=True), G.ST_INVALID_ARGUMENT),
    (dict(no_results=True), G.ST_INVALID_ARGUMENT),                                   # results and d_results both NULL
    (dict(task=dict(meta=None)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page=None)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(dtype=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(dtype=12)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_n=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_n=(1 << 24) + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=100)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=257)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=(1 << 64) - 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=100, page_n=50, cursors=None)), G.ST_INVALID_ARGUMENT),   # a bad every_rows is refused whatever k would be
    (dict(task=dict(cursors=None)), G.ST_INVALID_ARGUMENT),                           # k = 3
    (dict(task=dict(cursors=P + 4)), G.ST_INVALID_ARGUMENT),                          # misaligned
    (dict(task=dict(cursors=P + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(format_major=5)), G.ST_CORRUPTION),
]


@pytest.mark.parametrize("kw,status", CHECKS)
def test_argument_checks_come_before_anything_else(kw, status):
    code, st, res = call(**kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)   # nothing was written


def test_no_tasks_is_a_success_without_a_device():
    res = (G.TaskResult * 1)(); res[0].status = 99
    assert G.lib().pco_gfx_index_pages(0, None, res, None, None) == G.PcoSuccess
    assert G.lib().pco_gfx_index_pages(0, None, None, None, None) == G.PcoSuccess
    assert res[0].status == 99


# ---------------------------------------------------------------------------------------------------------------------------------------
# the slot arithmetic, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def index_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pageindex")
    src = d / "index.cpp"
    src.write_text(f'''
#include "{A.CSRC}/pco_index.h"
extern "C" uint64_t len(uint64_t page_n, uint64_t every_rows) {{ return pcogfx::index_len(page_n, every_rows); }}
extern "C" uint32_t slot(uint32_t batches_done, uint32_t every_batches, uint32_t k) {{ return pcogfx::index_slot(batches_done, every_batches, k); }}
''')
    out = d / "libindex.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.len.argtypes = [C.c_uint64, C.c_uint64]; lib.len.restype = C.c_uint64
    lib.slot.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]; lib.slot.restype = C.c_uint32
    return lib


def test_the_header_includes_no_device_header():
    text = open(os.path.join(A.CSRC, "pco_index.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["stdint.h"]
    assert "index_len" in text and "index_slot" in text


def test_index_len_of_the_header_against_the_restatement_and_the_export(index_lib):
    L = G.lib()
    for every_rows in (0, 100, 256, 512, 768, 1 << 16, 1 << 24, 1 << 40, (1 << 64) - 256):
        for page_n in (0, 1, 255, 256, 257, 512, 513, 768, 769, 2000, 65793, 1 << 24, (1 << 24) + 1, 1 << 40):
            want = restated_len(page_n, every_rows)
            assert index_lib.len(page_n, every_rows) == want == L.pco_gfx_page_index_len(page_n, every_rows), (page_n, every_rows)


@pytest.mark.parametrize("every_rows", [256, 512, 768])
def test_index_slot_exhaustively_over_small_pages(index_lib, every_rows):
    """Every page_n <= 2000: after each batch of the page the C function names the slot the restatement names, and over the batches the index
    call walks -- [0, k * every_rows / 256) -- the slots hit are 0 .. k - 1, each once, in order.  Batches behind the walk hit none."""
    eb = every_rows // 256
    for page_n in range(1, 2001):
        k = restated_len(page_n, every_rows)
        assert index_lib.len(page_n, every_rows) == k
        n_batches = (page_n + 255) // 256
        got = [index_lib.slot(done, eb, k) for done in range(0, n_batches + 1)]
        assert got == [restated_slot(done, eb, k) for done in range(0, n_batches + 1)], page_n
        walked = [s for s in got[1: k * eb + 1] if s != NO_SLOT]
        assert walked == list(range(k)), page_n
        assert got[0] == NO_SLOT and all(s == NO_SLOT for s in got[k * eb + 1:]), page_n
        assert k * eb < n_batches, page_n   # the walk never reaches the page's last batch


def test_index_slot_at_its_edges(index_lib):
    assert index_lib.slot(5, 0, 3) == NO_SLOT            # (k == 0 tasks carry every_batches 0)
    assert index_lib.slot(0, 1, 3) == NO_SLOT
    assert index_lib.slot(257, 1, 257) == 256 and index_lib.slot(258, 1, 257) == NO_SLOT   # k beyond a block's 256 threads
    assert index_lib.slot(65535, 1, 65535) == 65534 and index_lib.slot(65536, 65536, 1) == 0
    assert index_lib.slot(0xFFFFFFFF, 1, 0xFFFFFFFF) == 0xFFFFFFFE
