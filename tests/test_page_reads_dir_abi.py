"""CPU: the ABI of pco_gfx_decompress_page_reads_dir / pco_gfx_index_pages_dir / pco_gfx_lookback_window_n_log (include/pco_gfx.h section 4k) -- the two
task structs against the header and against a g++ offsetof probe, every host check of both entry points answered without a device in both forms and
under both flag values, and the task lists pcodec_amd.paged builds from a device directory (_DirPages) against the ones it builds from the host
directory (_BlobPages) for the same chunks, under the stand-ins of tests/paged_plan_util.py: field for field the same, apart from the addressing."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import paged_plan_util as U  # noqa: E402
import test_page_reads_abi as A  # noqa: E402  (header_fields, HEADER)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import build as B  # noqa: E402

FLAG = 1   # PCO_GFX_CURSOR_GENERAL
READ_FIELDS = ["dst", "page_n", "first", "count", "meta_piece", "page_piece", "dtype", "format_major", "from", "to", "history", "history_len"]
INDEX_FIELDS = ["cursors", "page_n", "every_rows", "meta_piece", "page_piece", "dtype", "format_major", "histories", "history_stride"]
STRUCTS = [("PcoGfxDirPageReadTask", "DirPageReadTask", 80, READ_FIELDS, [0, 8, 16, 24, 32, 36, 40, 44, 48, 56, 64, 72]),
           ("PcoGfxDirPageIndexTask", "DirPageIndexTask", 56, INDEX_FIELDS, [0, 8, 16, 24, 28, 32, 36, 40, 48])]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the structs and the exports
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("struct,binding,size,names,offsets", STRUCTS)
def test_the_binding_lays_the_structs_out_as_the_header_does(tmp_path, struct, binding, size, names, offsets):
    bound = getattr(G, binding)
    want = A.header_fields(struct)
    assert [n for n, _ in want] == names
    assert [(n.rstrip("_"), t) for n, t in bound._fields_] == want and C.sizeof(bound) == size   # (`from` is from_ in Python)
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "%s"\nint main() { printf("%%zu", sizeof(%s));\n%s\nreturn 0; }\n' % (
        os.path.abspath(A.HEADER), struct, "\n".join('printf(" %%zu", offsetof(%s, %s));' % (struct, f) for f in names)))
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    got_size, *got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got_size == size and got == [getattr(bound, n).offset for n, _ in bound._fields_] == offsets


def test_the_read_task_is_the_range_task_then_the_history_read_task_s_last_four():
    assert G.DirPageReadTask._fields_[:8] == G.DirPageRangeTask._fields_ and G.DirPageReadTask._fields_[8:] == G.PageReadHistTask._fields_[-4:]
    assert G.DirPageIndexTask._fields_[-2:] == G.PageIndexHistTask._fields_[-2:]


def test_the_header_declares_the_three_functions_and_the_library_exports_them():
    text = open(A.HEADER).read()
    tail = r"const PcoGfxDirectory\* dir, uint32_t flags,\s*PcoGfxTaskResult\* results, PcoGfxTaskResult\* d_results, void\* stream\);"
    assert re.search(r"enum PcoError pco_gfx_decompress_page_reads_dir\(size_t n_tasks, const PcoGfxDirPageReadTask\* tasks, " + tail, text)
    assert re.search(r"enum PcoError pco_gfx_index_pages_dir\(size_t n_tasks, const PcoGfxDirPageIndexTask\* tasks, " + tail, text)
    assert re.search(r"^int pco_gfx_lookback_window_n_log\(uint64_t n\);", text, re.M) and G.SIGNATURES["pco_gfx_lookback_window_n_log"] == (C.c_int, (C.c_uint64,))
    for name in ("pco_gfx_decompress_page_reads_dir", "pco_gfx_index_pages_dir", "pco_gfx_lookback_window_n_log"):
        assert hasattr(G.lib(), name) and name in G.SIGNATURES


@pytest.mark.parametrize("n", [1, 2, 16, 17, 1 << 15, (1 << 15) + 1, 1 << 24])
def test_the_window_of_a_lookback_chunk(n):
    assert G.lib().pco_gfx_lookback_window_n_log(n) == min(max((n - 1).bit_length(), 4), 15)


def test_the_window_of_no_chunk_is_zero():
    assert G.lib().pco_gfx_lookback_window_n_log(0) == 0 and G.lib().pco_gfx_lookback_window_n_log((1 << 24) + 1) == 0
    assert G.lib().pco_gfx_lookback_window_n_log(1 << 63) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
ALL_ONES = (1 << 64) - 1
GOOD_DIR = dict(d_blob=P, blob_len=100, d_offsets=P, n_pieces=8, gap=0, reserved=0)
GOOD_READ = dict(dst=P, page_n=10, first=0, count=1, meta_piece=0, page_piece=1, dtype=1, format_major=4, from_=P, to=P, history=P, history_len=80)
GOOD_INDEX = dict(cursors=P, page_n=1000, every_rows=256, meta_piece=0, page_piece=1, dtype=1, format_major=4, histories=P, history_stride=80)
KINDS = {"read": (G.DirPageReadTask, GOOD_READ, "pco_gfx_decompress_page_reads_dir"), "index": (G.DirPageIndexTask, GOOD_INDEX, "pco_gfx_index_pages_dir")}

# section 4e's list, then the fields both task kinds share
COMMON = [
    (dict(no_tasks=True), G.ST_INVALID_ARGUMENT),
    (dict(no_dir=True), G.ST_INVALID_ARGUMENT),
    (dict(directory=dict(d_blob=None)), G.ST_INVALID_ARGUMENT),
    (dict(directory=dict(d_offsets=None)), G.ST_INVALID_ARGUMENT),
    (dict(no_results=True), G.ST_INVALID_ARGUMENT),                                   # results and d_results both NULL
    (dict(directory=dict(n_pieces=1 << 31)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(meta_piece=8)), G.ST_INVALID_ARGUMENT),                           # a piece index >= n_pieces
    (dict(task=dict(page_piece=8)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_piece=0xFFFFFFFF)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(meta_piece=3, page_piece=3)), G.ST_INVALID_ARGUMENT),             # one piece cannot be both
    (dict(task=dict(dtype=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(dtype=12)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_n=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_n=(1 << 24) + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(format_major=5)), G.ST_CORRUPTION),
    (dict(task=dict(format_major=5, meta_piece=8)), G.ST_CORRUPTION),                 # check_partial_task's order: the version first
]
READ_ONLY = [   # sections 4f and 4i
    (dict(task=dict(dst=None)), G.ST_INVALID_ARGUMENT),                               # with count > 0
    (dict(task=dict(first=5, count=6)), G.ST_INVALID_ARGUMENT),                       # first + count > page_n
    (dict(task=dict(first=10, count=1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(first=11, count=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(first=ALL_ONES, count=2)), G.ST_INVALID_ARGUMENT),                # the sum wraps
    (dict(task=dict(page_n=0, first=0, count=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history=P, history_len=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history=None, history_len=80)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history=P + 4)), G.ST_INVALID_ARGUMENT),                          # misaligned
    (dict(task=dict(history=P + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history=P, history_len=0, count=0)), G.ST_INVALID_ARGUMENT),      # the pair is judged whatever the count is
]
INDEX_ONLY = [   # sections 4g and 4j
    (dict(task=dict(every_rows=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=100)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=257)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=ALL_ONES)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=100, page_n=50, cursors=None)), G.ST_INVALID_ARGUMENT),   # a bad every_rows is refused whatever k would be
    (dict(task=dict(cursors=None)), G.ST_INVALID_ARGUMENT),                           # k = 3
    (dict(task=dict(cursors=P + 4)), G.ST_INVALID_ARGUMENT),                          # misaligned
    (dict(task=dict(cursors=P + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(histories=P, history_stride=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(histories=None, history_stride=80)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history_stride=84)), G.ST_INVALID_ARGUMENT),                      # no multiple of 8
    (dict(task=dict(history_stride=81)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(histories=P + 4)), G.ST_INVALID_ARGUMENT),                        # misaligned
    (dict(task=dict(histories=P, history_stride=0, page_n=50)), G.ST_INVALID_ARGUMENT),   # the pair is judged whatever k is
]
CASES = [("read", kw, st) for kw, st in COMMON + READ_ONLY] + [("index", kw, st) for kw, st in COMMON + INDEX_ONLY]


def call(kind, flags=0, form="sync", task=None, directory=None, no_tasks=False, no_dir=False, no_results=False, n_tasks=1):
    struct, good, name = KINDS[kind]
    kw = dict(good); kw.update(task or {})
    arr = (struct * 1)(struct(**kw))
    dkw = dict(GOOD_DIR); dkw.update(directory or {})
    d = G.Directory(**dkw)
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    host, dev = (None if no_results else res, None) if form == "sync" else (None, None if no_results else P)   # (d_results: a device pointer the refused call never touches)
    code = getattr(G.lib(), name)(n_tasks, None if no_tasks else arr, None if no_dir else C.addressof(d), flags, host, dev, None)
    return code, G.lib().pco_gfx_last_status(), res[0]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags", [0, FLAG])
@pytest.mark.parametrize("kind,kw,status", CASES)
def test_every_host_check_comes_before_a_device_is_asked_for(kind, kw, status, flags, form):
    code, st, res = call(kind, flags, form, **kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)   # nothing was written


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("kind", ["read", "index"])
@pytest.mark.parametrize("flags", [2, 3, 4, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF])
def test_an_unknown_flag_bit_is_refused_before_anything_else(flags, kind, form):
    for kw in ({}, dict(no_dir=True), dict(no_tasks=True)):
        code, st, res = call(kind, flags, form, **kw)
        assert code == G.PcoDecompressionError and st == G.ST_INVALID_ARGUMENT
        assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)


@pytest.mark.parametrize("kind", ["read", "index"])
@pytest.mark.parametrize("flags", [0, FLAG])
def test_no_tasks_is_a_success_without_a_device_given_a_directory_and_results(kind, flags):
    assert call(kind, flags, n_tasks=0, no_tasks=True)[0] == G.PcoSuccess and call(kind, flags, "async", n_tasks=0, no_tasks=True)[0] == G.PcoSuccess
    # section 4e's rule: a call without results, or without a directory, is refused even when it has no tasks
    assert call(kind, flags, n_tasks=0, no_results=True)[:2] == (G.PcoDecompressionError, G.ST_INVALID_ARGUMENT)
    assert call(kind, flags, n_tasks=0, no_dir=True)[:2] == (G.PcoDecompressionError, G.ST_INVALID_ARGUMENT)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the planners: _DirPages builds what _BlobPages builds, apart from the addressing
# ---------------------------------------------------------------------------------------------------------------------------------------
EVERY = 256
WINDOW_BYTES = {c: 64 + U.WIDTHS[name] * (1 << min(max((sum(ns) - 1).bit_length(), 4), 15)) for c, (name, ns) in enumerate(zip(U.DTYPES, U.PAGE_NS))}
STRIDE = {c: (b + 7) // 8 * 8 for c, b in WINDOW_BYTES.items()}


class Lib(U.FakeLib):
    FORWARDED = U.FakeLib.FORWARDED + ("pco_gfx_lookback_window_n_log", "pco_gfx_lookback_history_bytes")
    DIR_FORMS = U.FakeLib.DIR_FORMS + ("pco_gfx_decompress_page_reads_dir", "pco_gfx_index_pages_dir")


@pytest.fixture()
def stand_ins(monkeypatch):
    if B.needs_build():
        B.build()
    from pcodec_amd import ChunkConfig, PagingSpec, paged
    G.lib()
    real_torch = sys.modules.get("torch")
    torch = sys.modules["torch"] = U.FakeTorch()
    lib = Lib(G)
    monkeypatch.setattr(paged, "_require_device", lambda: lib)
    monkeypatch.setattr(paged._BlobPages, "history_bytes", lambda self, L, blob, c: WINDOW_BYTES[c])   # every chunk under Lookback, as the device form must assume
    try:
        tensors = [torch.tensor_of(sum(ns), name) for ns, name in zip(U.PAGE_NS, U.DTYPES)]
        cc = paged.compress_chunks(tensors, ChunkConfig(paging_spec=PagingSpec.equal_pages_up_to(1000)), page_sizes=U.PAGE_NS, gap=4)
        pieces, total = U.directory(4)
        lib.calls.clear()
        yield paged, lib, cc, pieces
    finally:
        if real_torch is None:
            sys.modules.pop("torch", None)
        else:
            sys.modules["torch"] = real_torch


def rows_of(struct, call_):
    return [dict(zip([n for n, _ in struct._fields_], t)) for t in call_["tasks"]]


ADDRESSING = ("meta", "meta_len", "page", "page_len", "meta_piece", "page_piece")
POINTERS = ("dst", "from_", "to", "history", "cursors", "histories")


def same_apart_from_addressing(dir_tasks, blob_tasks, dir_base, blob_base):
    """field for field; a pointer into an output, a cursor tensor or a history tensor is compared as an offset from its call's first allocation"""
    assert len(dir_tasks) == len(blob_tasks)
    for d, b in zip(dir_tasks, blob_tasks):
        assert {k for k in d if k not in ADDRESSING} == {k for k in b if k not in ADDRESSING}
        for k in d:
            if k in ADDRESSING:
                continue
            if k in POINTERS:
                assert (d[k] is None) == (b[k] is None) and (d[k] is None or d[k] - dir_base == b[k] - blob_base), k
            else:
                assert d[k] == b[k], k


def pieces_of(tasks):
    first = [0, 4, 6]   # chunk c's ChunkMeta piece under U.PAGE_NS
    want = [(first[c], first[c] + 1 + i) for c, ns in enumerate(U.PAGE_NS) for i in range(len(ns))]
    return want, sorted({(t["meta_piece"], t["page_piece"]) for t in tasks})


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("history", [False, True])
def test_the_index_from_either_directory_is_the_same_tasks_keys_and_tensors(stand_ins, history, general):
    paged, lib, cc, pieces = stand_ins
    torch = sys.modules["torch"]
    base_d = torch._next
    idx_d = paged.index_pages_async(cc, EVERY, general=general, history=history)
    base_b = torch._next
    idx_b = paged.index_pages(cc.blob, pieces, U.DTYPES, EVERY, general=general, history=history)
    assert cc._dir is None
    d, b = lib.calls
    assert d["fn"] == "pco_gfx_index_pages_dir" and b["fn"] == ("pco_gfx_index_pages_hist" if history else "pco_gfx_index_pages_ex" if general else "pco_gfx_index_pages")
    assert d["dir"] == [cc.blob.data_ptr(), cc.blob.numel() - 64, cc.offsets.data_ptr(), 8, 4, 0]
    assert d["args"] == [FLAG if general else 0, None, idx_d.results.data_ptr(), U.STREAM_HANDLE]
    dt = rows_of(G.DirPageIndexTask, d)
    bt = rows_of(G.PageIndexHistTask if history else G.PageIndexTask, b)
    if not history:
        assert all((t.pop("histories"), t.pop("history_stride")) == (None, 0) for t in dt)
    same_apart_from_addressing(dt, bt, base_d, base_b)
    want, got = pieces_of(dt)
    assert got == want and [(t["meta_piece"], t["page_piece"]) for t in dt] == want
    assert [(p.chunk, p.piece, p.every_rows, p.cursors.shape) for p in idx_d] == [(p.chunk, p.piece, p.every_rows, p.cursors.shape) for p in idx_b]
    if history:
        assert [h.shape for h in idx_d.histories] == [h.shape for h in idx_b.histories]
        assert [h.shape[1] for h in idx_d.histories] == [STRIDE[p.chunk] for p in idx_d]
    else:
        assert idx_d.histories is None


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("history", [False, True])
def test_segments_and_rows_from_either_directory_are_the_same_tasks(stand_ins, history, general):
    paged, lib, cc, pieces = stand_ins
    torch = sys.modules["torch"]
    idx = paged.index_pages_async(cc, EVERY, general=general, history=history)
    rows = [(990, 2100), None, (0, 1)]
    for run_d, run_b in ((lambda: paged.decompress_chunks_from_async(cc, idx, general=general),
                          lambda: paged.decompress_chunks_from(cc.blob, pieces, U.DTYPES, idx, general=general, histories=idx.histories)),
                         (lambda: paged.decompress_rows_from_async(cc, idx, rows, general=general),
                          lambda: paged.decompress_rows_from(cc.blob, pieces, U.DTYPES, idx, rows, general=general, histories=idx.histories))):
        lib.calls.clear()
        base_d = torch._next
        outs_d, results = run_d()
        base_b = torch._next
        outs_b = run_b()
        assert cc._dir is None
        d, b = lib.calls
        assert d["fn"] == "pco_gfx_decompress_page_reads_dir"
        assert b["fn"] == ("pco_gfx_decompress_page_reads_hist" if history else "pco_gfx_decompress_page_reads_ex" if general else "pco_gfx_decompress_page_reads")
        assert d["args"] == [FLAG if general else 0, None, results.data_ptr(), U.STREAM_HANDLE] and d["dir"][3:5] == [8, 4]
        dt = rows_of(G.DirPageReadTask, d)
        bt = rows_of(G.PageReadHistTask if history else G.PageReadTask, b)
        if not history:
            assert all((t.pop("history"), t.pop("history_len")) == (None, 0) for t in dt)
        # cursors and histories are the index's own tensors in both calls: compared as they are, outputs as offsets
        for t in dt + bt:
            for k in ("from_", "history"):
                if t.get(k) is not None:
                    t[k] = ("index", t[k])
        for d_, b_ in zip(dt, bt):
            assert d_.get("from_") == b_.get("from_") and d_.get("history") == b_.get("history")
            d_.pop("from_"), b_.pop("from_"), d_.pop("history", None), b_.pop("history", None)
        same_apart_from_addressing(dt, bt, base_d, base_b)
        assert [o.shape for o in outs_d] == [o.shape for o in outs_b] and results.shape == (len(dt) * 24,)
        assert set(pieces_of(dt)[1]) <= set(pieces_of(dt)[0]) and all(t["to"] is None for t in dt)
        if history:
            assert any(t["history_len"] for t in dt)
