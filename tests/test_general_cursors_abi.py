"""PCO_GFX_CURSOR_GENERAL (include/pco_gfx.h section 4h) without a device: the two _ex exports, their flag and host checks (made before anything
is launched, and before a device is asked for), the kind-3 verdict and word writer of pcodec_amd/csrc/pco_cursor.h compiled on their own with g++
(the same lines the general kernel runs per task) against a plain Python restatement, the packing of Conv1 residuals, and the tANS model stepped
batch by batch over a page with more than 256 bins: the expected cursor fields of tests/test_gpu_general_cursors.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import tans_model as TM  # noqa: E402
import test_page_reads_abi as A  # noqa: E402  (the cursor's layout restated, the stepped tANS model, the read checks)
from pcodec_amd import _lib as G  # noqa: E402

HEADER = A.HEADER
CSRC = A.CSRC
ALL_ONES = A.ALL_ONES
GENERAL = 3     # the kind
FLAG = 1        # PCO_GFX_CURSOR_GENERAL


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kind-3 layout, restated: used here and by the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def pack_residuals(residuals):
    """words 10 .. 25 under Conv1: residual i in bits 32 (i % 2) .. of word 10 + i / 2"""
    assert len(residuals) <= 32
    tail = [0] * 16
    for i, r in enumerate(residuals):
        tail[i // 2] |= (int(r) & 0xFFFFFFFF) << (32 * (i % 2))
    return tail


def unpack_residuals(w, order):
    return [(int(w[10 + i // 2]) >> (32 * (i % 2))) & 0xFFFFFFFF for i in range(order)]


def pack_general(row, bit, page_n, dtype, states=None, moments=None, residuals=None, version=A.VERSION, kind=GENERAL):
    """The 32 words of a kind-3 cursor: A.pack_cursor's, with the residuals in the moments' place under Conv1."""
    w = A.pack_cursor(kind, row, bit, page_n, dtype, states, moments, version)
    if residuals is not None:
        assert moments is None
        w[10:26] = pack_residuals(residuals)
    return w


def restated_verdict_general(w, page_n, dtype, first, body_first_bit, page_bits, asl, end_batch, walk_cap):
    """include/pco_gfx.h section 4h's list of refusals"""
    c = A.unpack_cursor(w)
    if c["version"] != A.VERSION or c["kind"] != GENERAL:
        return G.ST_INVALID_ARGUMENT
    if c["page_n"] != page_n or c["dtype"] != dtype:
        return G.ST_INVALID_ARGUMENT
    if c["row"] > first or (c["row"] % 256 != 0 and c["row"] != page_n):
        return G.ST_INVALID_ARGUMENT
    if c["bit"] < body_first_bit or c["bit"] > page_bits:
        return G.ST_INVALID_ARGUMENT
    if any(c["states"][v][j] >= 1 << asl[v] for v in range(3) for j in range(4)):
        return G.ST_INVALID_ARGUMENT
    if end_batch - c["row"] // 256 > walk_cap or end_batch < c["row"] // 256:
        return G.ST_INVALID_ARGUMENT
    return G.ST_OK


# ---------------------------------------------------------------------------------------------------------------------------------------
# the exports and the constants
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(HEADER).read()
    assert re.search(r"#define PCO_GFX_CURSOR_GENERAL 1u", text)
    assert re.search(r"enum PcoError pco_gfx_decompress_page_reads_ex\(size_t n_tasks, const PcoGfxPageReadTask\* tasks, uint32_t flags, PcoGfxTaskResult\* results,", text)
    assert re.search(r"enum PcoError pco_gfx_index_pages_ex\(size_t n_tasks, const PcoGfxPageIndexTask\* tasks, uint32_t flags, PcoGfxTaskResult\* results,", text)
    assert hasattr(G.lib(), "pco_gfx_decompress_page_reads_ex") and hasattr(G.lib(), "pco_gfx_index_pages_ex")
    assert (G.CURSOR_GENERAL, G.CURSOR_GENERAL_KIND) == (FLAG, GENERAL)
    cur = open(os.path.join(CSRC, "pco_cursor.h")).read()
    assert re.search(r"kCursorGeneral = 3;", cur) and re.search(r"kCursorFull = 1, kCursorPosition = 2;", cur)


# ---------------------------------------------------------------------------------------------------------------------------------------
# host checks through the _ex forms
# ---------------------------------------------------------------------------------------------------------------------------------------
def call_reads(flags, task=None, no_tasks=False, no_results=False):
    L = G.lib()
    kw = dict(A.GOOD_TASK); kw.update(task or {})
    arr = (G.PageReadTask * 1)(G.PageReadTask(**kw))
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    code = L.pco_gfx_decompress_page_reads_ex(1, None if no_tasks else arr, flags, None if no_results else res, None, None)
    return code, L.pco_gfx_last_status(), res[0]


INDEX_GOOD = dict(meta=A.P, meta_len=10, page=A.P, page_len=10, cursors=A.P, page_n=1000, every_rows=256, dtype=1, format_major=4)
INDEX_CHECKS = [
    (dict(no_tasks=True), G.ST_INVALID_ARGUMENT),
    (dict(no_results=True), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(meta=None)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page=None)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(dtype=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_n=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(page_n=(1 << 24) + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(every_rows=100)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(cursors=None)), G.ST_INVALID_ARGUMENT),            # k = 3 > 0
    (dict(task=dict(cursors=A.P + 4)), G.ST_INVALID_ARGUMENT),        # misaligned
    (dict(task=dict(format_major=5)), G.ST_CORRUPTION),
]


def call_index(flags, task=None, no_tasks=False, no_results=False):
    L = G.lib()
    kw = dict(INDEX_GOOD); kw.update(task or {})
    arr = (G.PageIndexTask * 1)(G.PageIndexTask(**kw))
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    code = L.pco_gfx_index_pages_ex(1, None if no_tasks else arr, flags, None if no_results else res, None, None)
    return code, L.pco_gfx_last_status(), res[0]


@pytest.mark.parametrize("flags", [2, 3, 4, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF])
@pytest.mark.parametrize("call", [call_reads, call_index])
def test_an_unknown_flag_bit_is_refused_before_anything_else(call, flags):
    code, st, res = call(flags)   # (every other argument is fine, and nothing is dereferenced: the refusal comes first)
    assert code == G.PcoDecompressionError and st == G.ST_INVALID_ARGUMENT
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)


@pytest.mark.parametrize("flags", [0, FLAG])
@pytest.mark.parametrize("kw,status", A.CHECKS)
def test_the_read_checks_through_the_ex_form(kw, status, flags):
    code, st, res = call_reads(flags, **kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)


@pytest.mark.parametrize("flags", [0, FLAG])
@pytest.mark.parametrize("kw,status", INDEX_CHECKS)
def test_the_index_checks_through_the_ex_form(kw, status, flags):
    code, st, res = call_index(flags, **kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)


def test_the_index_checks_here_are_the_ones_the_unflagged_entry_point_makes():
    """the list above, through pco_gfx_index_pages itself: the same refusals"""
    L = G.lib()
    for kw, status in INDEX_CHECKS:
        t = dict(INDEX_GOOD); t.update(kw.get("task") or {})
        arr = (G.PageIndexTask * 1)(G.PageIndexTask(**t))
        res = (G.TaskResult * 1)()
        code = L.pco_gfx_index_pages(1, None if kw.get("no_tasks") else arr, None if kw.get("no_results") else res, None, None)
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == status, kw


@pytest.mark.parametrize("flags", [0, FLAG])
def test_no_tasks_is_a_success_without_a_device(flags):
    res = (G.TaskResult * 1)()
    assert G.lib().pco_gfx_decompress_page_reads_ex(0, None, flags, res, None, None) == G.PcoSuccess
    assert G.lib().pco_gfx_index_pages_ex(0, None, flags, res, None, None) == G.PcoSuccess


# ---------------------------------------------------------------------------------------------------------------------------------------
# the verdict and the word writer, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cursor_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("generalverdict")
    src = d / "verdict.cpp"
    src.write_text(f'''
#include "{CSRC}/pco_cursor.h"
using namespace pcogfx;
extern "C" uint32_t verdict(const uint64_t* w, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits, const uint32_t* asl,
                            uint64_t end_batch, uint64_t walk_cap) {{
  return cursor_verdict_general(w, page_n, dtype, first, body_first_bit, page_bits, asl, end_batch, walk_cap);
}}
// the words as the kernel forms them: a state pair per word 4 .. 9, a tail word per word 10 .. 25
extern "C" void words(uint64_t row, uint64_t bit, uint64_t page_n, uint32_t dtype, const uint32_t* states, const uint64_t* tail, uint64_t* out) {{
  for (uint32_t i = 0; i < kCursorWords; i++) {{
    const uint32_t s = i >= kCursorStateWord && i < kCursorMomentWord ? 2 * (i - kCursorStateWord) : 0;
    const uint32_t t = i >= kCursorMomentWord && i < kCursorMomentWord + 16 ? i - kCursorMomentWord : 0;
    out[i] = cursor_word_general(i, row, bit, page_n, dtype, (uint64_t)states[s] | ((uint64_t)states[s + 1] << 32), tail[t]);
  }}
}}
extern "C" void pack(const uint32_t* residuals, uint32_t order, uint64_t* tail) {{ cursor_conv1_pack(residuals, order, tail); }}
extern "C" uint32_t residual(const uint64_t* w, uint32_t i) {{ return cursor_conv1_residual(w, i); }}
extern "C" uint32_t old_verdict(const uint64_t* w, uint32_t want_kind, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits, const uint32_t* asl) {{
  return cursor_verdict(w, want_kind, page_n, dtype, first, body_first_bit, page_bits, asl);
}}
''')
    out = d / "libgeneralcursor.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.verdict.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]
    lib.verdict.restype = C.c_uint32
    lib.words.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.words.restype = None
    lib.pack.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]; lib.pack.restype = None
    lib.residual.argtypes = [C.c_void_p, C.c_uint32]; lib.residual.restype = C.c_uint32
    lib.old_verdict.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.old_verdict.restype = C.c_uint32
    return lib


def run_verdict(lib, w, page_n, dtype, first, body_first_bit, page_bits, asl, end_batch, walk_cap):
    return lib.verdict((C.c_uint64 * 32)(*w), page_n, dtype, first, body_first_bit, page_bits, (C.c_uint32 * 3)(*asl), end_batch, walk_cap)


ASL = [0, 14, 2]
STATES = [[0, 0, 0, 0], [5, 6, 7, (1 << 14) - 1], [1, 2, 3, 3]]
SCENE = dict(page_n=3000, dtype=1, first=600, body_first_bit=40, page_bits=8000, end_batch=4, walk_cap=2)   # rows [600, 1000): batches 2 and 3 from a cursor at 512


def good(**kw):
    d = dict(row=512, bit=1000, page_n=3000, dtype=1, states=[list(s) for s in STATES], moments=[[7] * 8, [9] * 8])
    d.update(kw)
    return pack_general(**d)


def with_state(v, j, x):
    s = [list(r) for r in STATES]; s[v][j] = x
    return good(states=s)


# (name, cursor words, what differs from SCENE, the status expected -- written down here, not taken from either implementation)
ROWS = [
    ("a cursor that passes", good(), {}, G.ST_OK),
    ("a wrong version", good(version=2), {}, G.ST_INVALID_ARGUMENT),
    ("version 0", good(version=0), {}, G.ST_INVALID_ARGUMENT),
    ("kind 1", good(kind=A.FULL), {}, G.ST_INVALID_ARGUMENT),
    ("kind 2", good(kind=A.POSITION), {}, G.ST_INVALID_ARGUMENT),
    ("kind 4", good(kind=4), {}, G.ST_INVALID_ARGUMENT),
    ("another page_n", good(page_n=2999), {}, G.ST_INVALID_ARGUMENT),
    ("another dtype", good(dtype=3), {}, G.ST_INVALID_ARGUMENT),
    ("at > first", good(row=768), {}, G.ST_INVALID_ARGUMENT),
    ("at == first", good(), dict(first=512), G.ST_OK),
    ("first one row in front of at", good(), dict(first=511), G.ST_INVALID_ARGUMENT),
    ("at neither a multiple of 256 nor page_n", good(row=300), {}, G.ST_INVALID_ARGUMENT),
    ("at == page_n", good(row=3000), dict(first=3000, end_batch=12, walk_cap=1), G.ST_OK),
    ("at == page_n but first in front of it", good(row=3000), dict(first=2999, end_batch=12, walk_cap=1), G.ST_INVALID_ARGUMENT),
    ("the body's first bit", good(bit=40), {}, G.ST_OK),
    ("one bit in front of the body", good(bit=39), {}, G.ST_INVALID_ARGUMENT),
    ("the page's last bit position", good(bit=8000), {}, G.ST_OK),
    ("one bit beyond the page", good(bit=8001), {}, G.ST_INVALID_ARGUMENT),
    ("a bit position of all ones", good(bit=ALL_ONES), {}, G.ST_INVALID_ARGUMENT),
    ("the primary's state 2^asl - 1", with_state(1, 0, (1 << 14) - 1), {}, G.ST_OK),
    ("the primary's state 2^asl", with_state(1, 0, 1 << 14), {}, G.ST_INVALID_ARGUMENT),
    ("the secondary's state 2^asl - 1", with_state(2, 3, 3), {}, G.ST_OK),
    ("the secondary's state 2^asl", with_state(2, 3, 4), {}, G.ST_INVALID_ARGUMENT),
    ("a state of all ones", with_state(1, 2, 0xFFFFFFFF), {}, G.ST_INVALID_ARGUMENT),
    ("a state for a variable the page does not have", with_state(0, 1, 1), {}, G.ST_INVALID_ARGUMENT),
    ("exactly the batches the host gave scratch for", good(), dict(walk_cap=2), G.ST_OK),
    ("one batch more than the host gave scratch for", good(), dict(walk_cap=1), G.ST_INVALID_ARGUMENT),
    ("a cursor at row 0 walks every batch to the end", good(row=0), dict(walk_cap=3), G.ST_INVALID_ARGUMENT),
    ("... and passes with that many", good(row=0), dict(walk_cap=4), G.ST_OK),
    ("moments of all ones", good(moments=[[ALL_ONES] * 8, [ALL_ONES] * 8]), {}, G.ST_OK),
    ("Conv1 residuals of 0xFFFFFFFF", good(moments=None, residuals=[0xFFFFFFFF] * 32), {}, G.ST_OK),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_the_general_verdict_against_its_restatement(cursor_lib, row):
    _, w, diff, status = row
    scene = dict(SCENE); scene.update(diff)
    assert restated_verdict_general(w, asl=ASL, **scene) == status
    assert run_verdict(cursor_lib, w, asl=ASL, **scene) == status


def test_the_general_verdict_over_a_small_grid(cursor_lib):
    """version x kind x row x first x the cursor's page_n x bit position x one state x walk_cap: 3 * 4 * 5 * 4 * 2 * 4 * 3 * 3 cursors"""
    n = 0
    for version in (0, 1, 2):
        for kind in (1, 2, 3, 4):
            for row in (0, 256, 300, 512, 3000):
                for first in (0, 256, 511, 3000):
                    for page_n in (3000, 2999):
                        for bit in (39, 40, 8000, 8001):
                            for st in (0, 3, 4):
                                for cap in (0, 1, 12):
                                    s = [list(r) for r in STATES]; s[2][1] = st
                                    w = pack_general(row, bit, page_n, 1, s, None, None, version, kind)
                                    args = dict(page_n=3000, dtype=1, first=first, body_first_bit=40, page_bits=8000, asl=ASL, end_batch=(first + 1 + 255) // 256, walk_cap=cap)
                                    assert run_verdict(cursor_lib, w, **args) == restated_verdict_general(w, **args), (version, kind, row, first, page_n, bit, st, cap)
                                    n += 1
    assert n == 17280


def test_the_two_older_kinds_refuse_a_kind_3_cursor_and_it_refuses_them(cursor_lib):
    asl = (C.c_uint32 * 3)(*ASL)
    w3 = (C.c_uint64 * 32)(*good())
    for want in (A.FULL, A.POSITION):
        assert cursor_lib.old_verdict(w3, want, 3000, 1, 600, 40, 8000, asl) == G.ST_INVALID_ARGUMENT
    for kind in (A.FULL, A.POSITION):
        assert run_verdict(cursor_lib, A.pack_cursor(kind, 512, 1000, 3000, 1, STATES), asl=ASL, **SCENE) == G.ST_INVALID_ARGUMENT


def test_the_word_writer_is_the_documented_layout(cursor_lib):
    st = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]; mom = [(1 << 63) + i * 977 for i in range(16)]
    out = (C.c_uint64 * 32)()
    cursor_lib.words(768, 12345, 3000, 6, (C.c_uint32 * 12)(*st), (C.c_uint64 * 16)(*mom), out)
    want = pack_general(768, 12345, 3000, 6, [st[0:4], st[4:8], st[8:12]], [mom[:8], mom[8:]])
    assert list(out) == want and list(out)[26:] == [0] * 6
    c = A.unpack_cursor(out)
    assert (c["version"], c["kind"], c["row"], c["bit"], c["page_n"], c["dtype"]) == (1, GENERAL, 768, 12345, 3000, 6)
    assert c["states"] == [st[0:4], st[4:8], st[8:12]] and c["moments"] == [mom[:8], mom[8:]]
    # the same words as kind 1 but for the kind
    assert want[1:] == A.pack_cursor(A.FULL, 768, 12345, 3000, 6, [st[0:4], st[4:8], st[8:12]], [mom[:8], mom[8:]])[1:]


@pytest.mark.parametrize("order", [1, 2, 31, 32])
def test_conv1_residuals_pack_and_unpack(cursor_lib, order):
    rng = np.random.default_rng(order)
    res = [int(x) for x in rng.integers(0, 1 << 32, order, dtype=np.uint64)]
    res[0] = 0xFFFFFFFF; res[-1] = 0x80000001 if order > 1 else 0xFFFFFFFF
    tail = (C.c_uint64 * 16)(*([ALL_ONES] * 16))   # (every word is written)
    cursor_lib.pack((C.c_uint32 * 32)(*(res + [0xDEADBEEF] * (32 - order))), order, tail)   # (what lies beyond the order is not read into the cursor)
    assert list(tail) == pack_residuals(res)
    assert all(x == 0 for x in list(tail)[(order + 1) // 2:]) and (order % 2 == 0 or list(tail)[order // 2] >> 32 == 0)
    w = pack_general(512, 1000, 3000, 1, STATES, None, res)
    assert unpack_residuals(w, order) == res
    cw = (C.c_uint64 * 32)(*w)
    assert [cursor_lib.residual(cw, i) for i in range(order)] == res
    assert w[26:] == [0] * 6 and w[:10] == good()[:10]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tANS model, batch by batch, over a table of more than 256 bins
# ---------------------------------------------------------------------------------------------------------------------------------------
def wide_table_page(dt, n, n_bins, seed):
    """A one-variable Classic page without delta whose table has `n_bins` > 256 bins: (numbers, ChunkMeta bytes, page bytes)"""
    x = np.random.default_rng(seed).integers(0, 60000 if np.dtype(dt).itemsize > 1 else 256, n).astype(dt)
    meta, pages = O.test_encode(x, pages=[n], mode=O.MODE_CLASSIC, tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_n_bins=n_bins, tbl_seed=seed)
    return x, meta, pages[0]


@pytest.mark.parametrize("dt,n,n_bins", [(np.uint32, 3000, 300), (np.uint16, 2816, 1000), (np.int64, 700, 257)])
def test_the_stepped_model_decodes_a_page_of_more_than_256_bins(dt, n, n_bins):
    x, meta, page = wide_table_page(dt, n, n_bins, n)
    ok, err, in_meta = O.wrapped_page_prefix(meta, page, x.dtype, n)
    assert err == 0 and not in_meta and np.array_equal(ok.view(x.dtype), x), "the oracle decodes the page to the input"
    bits = np.dtype(dt).itemsize * 8
    body, marks, latents, size_log = A.model_cursors(meta, page, n, bits)
    r = TM.Bits(meta); r.read(8); r.read(4)
    assert r.read(15) == n_bins > 256
    assert [int(v) for v in TM.to_latent(x)] == latents
    assert [m[0] for m in marks] == [min(r + 256, n) for r in range(0, n, 256)]
    assert body == -(-4 * size_log // 8) * 8 and all(a[1] <= b[1] for a, b in zip(marks, marks[1:])) and marks[-1][1] <= 8 * len(page)
    assert all(0 <= s < 1 << size_log for m in marks for s in m[2])
