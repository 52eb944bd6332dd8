"""pco_gfx_decompress_pages_dir / pco_gfx_decompress_page_ranges_dir (include/pco_gfx.h section 4e) without a device: the three structs of the
ctypes binding against the header, the argument checks (made before anything is launched, and before a device is asked for), the directory
verdict of pcodec_amd/csrc/pco_dir.h compiled on its own with g++ (the same lines dir_resolve_kernel runs per task) against a plain Python
restatement, and CompressedChunks.page_ns' arithmetic."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402

HEADER = os.path.join(HERE, "..", "include", "pco_gfx.h")
CSRC = os.path.abspath(os.path.join(HERE, "..", "pcodec_amd", "csrc"))
C_TYPES = {"const void*": C.c_void_p, "void*": C.c_void_p, "const uint64_t*": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
ALL_ONES = (1 << 64) - 1


def header_fields(struct):
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const void\*|void\*|const uint64_t\*|uint64_t|uint32_t)\s+(.*)", decl)
        assert m, decl
        for name in m.group(2).split(","):
            out.append((name.strip(), C_TYPES[m.group(1)]))
    return out


@pytest.mark.parametrize("struct,binding,size,names", [
    ("PcoGfxDirectory", "Directory", 40, ["d_blob", "blob_len", "d_offsets", "n_pieces", "gap", "reserved"]),
    ("PcoGfxDirPageTask", "DirPageTask", 32, ["dst", "page_n", "meta_piece", "page_piece", "dtype", "format_major"]),
    ("PcoGfxDirPageRangeTask", "DirPageRangeTask", 48, ["dst", "page_n", "first", "count", "meta_piece", "page_piece", "dtype", "format_major"]),
])
def test_the_binding_lays_the_structs_out_as_the_header_does(struct, binding, size, names):
    want = header_fields(struct)
    cls = getattr(G, binding)
    assert [n for n, _ in want] == names
    assert [(n, t) for n, t in cls._fields_] == want
    assert C.sizeof(cls) == size
    at = 0   # natural alignment without padding: every field starts where the one before ended
    for n, t in want:
        assert getattr(cls, n).offset == at, n
        at += C.sizeof(t)
    assert at == size


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(HEADER).read()
    assert re.search(r"enum PcoError pco_gfx_decompress_pages_dir\(size_t n_tasks, const PcoGfxDirPageTask\* tasks, const PcoGfxDirectory\* dir,", text)
    assert re.search(r"enum PcoError pco_gfx_decompress_page_ranges_dir\(size_t n_tasks, const PcoGfxDirPageRangeTask\* tasks, const PcoGfxDirectory\* dir,", text)
    assert hasattr(G.lib(), "pco_gfx_decompress_pages_dir") and hasattr(G.lib(), "pco_gfx_decompress_page_ranges_dir")


P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
GOOD_DIR = dict(d_blob=P, blob_len=100, d_offsets=P, n_pieces=8, gap=0, reserved=0)
GOOD_TASK = dict(dst=P, page_n=10, meta_piece=0, page_piece=1, dtype=1, format_major=4)


def call(ranges, task=None, directory=None, no_tasks=False, no_dir=False, no_results=False):
    L = G.lib()
    kw = dict(GOOD_TASK); kw.update(dict(first=0, count=1) if ranges else {}); kw.update(task or {})
    arr = ((G.DirPageRangeTask if ranges else G.DirPageTask) * 1)((G.DirPageRangeTask if ranges else G.DirPageTask)(**kw))
    dkw = dict(GOOD_DIR); dkw.update(directory or {})
    d = G.Directory(**dkw)
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    fn = L.pco_gfx_decompress_page_ranges_dir if ranges else L.pco_gfx_decompress_pages_dir
    code = fn(1, None if no_tasks else arr, None if no_dir else C.addressof(d), None if no_results else res, None, None)
    return code, L.pco_gfx_last_status(), res[0]


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
    (dict(task=dict(dst=None)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(format_major=5)), G.ST_CORRUPTION),
]
RANGES_ONLY = [
    (dict(task=dict(first=5, count=6)), G.ST_INVALID_ARGUMENT),                       # first + count > page_n
    (dict(task=dict(first=11, count=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(first=ALL_ONES, count=2)), G.ST_INVALID_ARGUMENT),                # the sum wraps
    (dict(task=dict(page_n=0, first=0, count=0)), G.ST_INVALID_ARGUMENT),
]


@pytest.mark.parametrize("ranges,kw,status", [(False, kw, st) for kw, st in COMMON] + [(True, kw, st) for kw, st in COMMON + RANGES_ONLY])
def test_argument_checks_come_before_anything_else(ranges, kw, status):
    code, st, res = call(ranges, **kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)   # nothing was written


def test_no_tasks_is_a_success_without_a_device():
    d = G.Directory(**GOOD_DIR); res = (G.TaskResult * 1)()
    assert G.lib().pco_gfx_decompress_pages_dir(0, None, C.addressof(d), res, None, None) == G.PcoSuccess
    assert G.lib().pco_gfx_decompress_page_ranges_dir(0, None, C.addressof(d), res, None, None) == G.PcoSuccess


# ---------------------------------------------------------------------------------------------------------------------------------------
# the verdict function, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdict(tmp_path_factory):
    d = tmp_path_factory.mktemp("dirverdict")
    src = d / "verdict.cpp"
    src.write_text(f'''
#include "{CSRC}/pco_dir.h"
extern "C" void verdict(uint64_t blob, uint64_t blob_len, uint32_t gap, const uint64_t* offs, uint64_t n_pieces, uint32_t meta_piece, uint32_t page_piece, uint64_t* out) {{
  const pcogfx::DirVerdict v = pcogfx::dir_verdict((const uint8_t*)blob, blob_len, gap, offs[n_pieces], offs[meta_piece], offs[meta_piece + 1], offs[page_piece], offs[page_piece + 1]);
  out[0] = (uint64_t)v.meta; out[1] = v.meta_len; out[2] = (uint64_t)v.page; out[3] = v.page_len; out[4] = v.status;
}}
''')
    out = d / "libverdict.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.verdict.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.verdict.restype = None

    def run(blob, blob_len, gap, offs, mp, pp):
        a = (C.c_uint64 * len(offs))(*offs); o = (C.c_uint64 * 5)()
        lib.verdict(blob, blob_len, gap, a, len(offs) - 1, mp, pp, o)
        return tuple(int(x) for x in o)
    return run


def restated(blob, blob_len, gap, offs, mp, pp):
    """include/pco_gfx.h section 4e's table, top to bottom; a refused task points at the blob's first byte with lengths of 0"""
    refuse = lambda status: (blob, 0, blob, 0, status)   # noqa: E731
    if offs[-1] == ALL_ONES:
        return refuse(G.ST_INVALID_ARGUMENT)
    for k in (mp, pp):
        if offs[k] > offs[k + 1] or offs[k + 1] > blob_len:
            return refuse(G.ST_INVALID_ARGUMENT)
    if offs[mp + 1] == offs[mp]:
        return refuse(G.ST_INSUFFICIENT_DATA)
    if offs[mp + 1] - offs[mp] < gap or offs[pp + 1] - offs[pp] < gap:
        return refuse(G.ST_INVALID_ARGUMENT)
    return (blob + offs[mp] + gap, offs[mp + 1] - offs[mp] - gap, blob + offs[pp] + gap, offs[pp + 1] - offs[pp] - gap, G.ST_OK)


BLOB = 0x7F0000001000
# (name, blob_len, gap, offsets, meta_piece, page_piece, the status expected -- written down here, not taken from either implementation)
ROWS = [
    ("a normal pair, gap 0", 100, 0, [5, 14, 60, 100], 0, 1, G.ST_OK),
    ("a normal pair, gap 4", 100, 4, [5, 18, 60, 100], 0, 2, G.ST_OK),
    ("a page of 0 bytes, gap 0", 100, 0, [0, 9, 9, 9, 9], 0, 2, G.ST_OK),
    ("a page of 0 bytes, gap 4", 100, 4, [0, 13, 17, 21, 25], 0, 3, G.ST_OK),
    ("a ChunkMeta of 1 byte, gap 4", 100, 4, [0, 5, 9], 0, 1, G.ST_OK),
    ("a dropped chunk, gap 0", 100, 0, [0, 9, 9, 9, 20], 1, 2, G.ST_INSUFFICIENT_DATA),
    ("a dropped chunk, gap 4", 100, 4, [0, 13, 13, 13, 30], 1, 2, G.ST_INSUFFICIENT_DATA),
    ("the sentinel", 100, 0, [5, 14, 60, ALL_ONES], 0, 1, G.ST_INVALID_ARGUMENT),
    ("the sentinel, itself the page's end", 100, 0, [5, 14, ALL_ONES], 0, 1, G.ST_INVALID_ARGUMENT),
    ("a descending ChunkMeta", 100, 0, [14, 5, 60, 100], 0, 2, G.ST_INVALID_ARGUMENT),
    ("a descending page", 100, 0, [5, 14, 60, 50, 100], 0, 2, G.ST_INVALID_ARGUMENT),
    ("a page that ends beyond blob_len", 99, 0, [5, 14, 60, 100], 0, 2, G.ST_INVALID_ARGUMENT),
    ("a ChunkMeta that ends beyond blob_len", 13, 0, [5, 14, 14, 100], 0, 1, G.ST_INVALID_ARGUMENT),
    ("an end exactly at blob_len", 100, 0, [5, 14, 60, 100], 0, 2, G.ST_OK),
    ("a page extent of gap - 1", 100, 4, [0, 13, 16, 30], 0, 1, G.ST_INVALID_ARGUMENT),
    ("a ChunkMeta extent of gap - 1", 100, 4, [0, 3, 16, 30], 0, 1, G.ST_INVALID_ARGUMENT),
    ("dropped comes before the gap check", 100, 4, [7, 7, 7, 30], 0, 1, G.ST_INSUFFICIENT_DATA),
    ("the page in front of its ChunkMeta", 100, 4, [0, 30, 43, 43], 1, 0, G.ST_OK),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_the_verdict_function_against_its_restatement(verdict, row):
    _, blob_len, gap, offs, mp, pp, status = row
    want = restated(BLOB, blob_len, gap, offs, mp, pp)
    assert want[4] == status
    assert verdict(BLOB, blob_len, gap, offs, mp, pp) == want
    if status != G.ST_OK:
        assert want[:4] == (BLOB, 0, BLOB, 0)
    else:
        assert want[0] != 0 and want[2] != 0


def test_the_verdict_function_over_every_small_directory(verdict):
    """all offset triples over {0, 1, 3, 4, 5, 9, ~0} x gaps {0, 1, 4} x blob_len {4, 9}: 7^3 * 6 directories of two pieces"""
    vals = [0, 1, 3, 4, 5, 9, ALL_ONES]
    for a in vals:
        for b in vals:
            for c in vals:
                for gap in (0, 1, 4):
                    for blob_len in (4, 9):
                        got = verdict(BLOB, blob_len, gap, [a, b, c], 0, 1)
                        assert got == restated(BLOB, blob_len, gap, [a, b, c], 0, 1), (a, b, c, gap, blob_len)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CompressedChunks.page_ns
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
@pytest.mark.parametrize("max_page_n", [1, 256, 1000, 1 << 18])
def test_page_ns_arithmetic_is_equal_pages_up_to(n, max_page_n):
    L = G.lib()   # (host arithmetic only: the library loads without a device)
    got = paged.equal_pages(n, max_page_n)
    k = -(-n // max_page_n)   # chunk_config.rs:145-161: as few pages as fit, the first n % k one number longer
    assert len(got) == k == L.pco_gfx_wrapped_n_pages(n, max_page_n)
    assert got == [n // k + (1 if i < n % k else 0) for i in range(k)]
    assert sum(got) == n and max(got) <= max_page_n and max(got) - min(got) <= 1


def test_page_ns_default_page_size_and_the_record():
    assert paged.equal_pages(1 << 18, 0) == [1 << 18] and paged.equal_pages((1 << 18) + 1, 0) == [(1 << 17) + 1, 1 << 17] and paged.equal_pages(0, 7) == []
    cc = paged.CompressedChunks(None, None, None, [3], ["uint32"], 4, None, None, [[5, 4]])
    assert cc.page_ns == [[5, 4]] and cc._dir is None
