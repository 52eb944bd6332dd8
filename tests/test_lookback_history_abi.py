"""pco_gfx_decompress_page_reads_hist (include/pco_gfx.h section 4i) without a device: the struct and the exports, pco_gfx_lookback_history_bytes,
the host checks (made before a device is asked for) through both forms, pcodec_amd/csrc/pco_history.h and the kind-4 verdict of pco_cursor.h
compiled on their own with g++ (the same lines the general kernel runs per task) against plain Python restatements, the update interval's two
properties on a simulated ring, and the tANS model stepped batch by batch over a Lookback page with its delta variable: the expected cursor
fields of tests/test_gpu_lookback_history.py."""
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
import test_page_reads_abi as A  # noqa: E402  (the cursor's layout restated, the ten-field checks)
import test_general_cursors_abi as GA  # noqa: E402  (kind 3's verdict restated: kind 4's list is the same)
from pcodec_amd import _lib as G  # noqa: E402

HEADER, CSRC, ALL_ONES = A.HEADER, A.CSRC, A.ALL_ONES
LOOKBACK = 4                  # the kind
HEADER_BYTES = 64
FLAG = 1                      # PCO_GFX_CURSOR_GENERAL


# ---------------------------------------------------------------------------------------------------------------------------------------
# the layouts, restated: used here and by the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def pack_lookback(row, bit, page_n, dtype, states=None, version=A.VERSION, kind=LOOKBACK):
    """The 32 words of a kind-4 cursor: kind 1's words 0..9, zeros behind them."""
    return A.pack_cursor(kind, row, bit, page_n, dtype, states, None, version)


def history_bytes(window_n_log, width):
    return HEADER_BYTES + (width << window_n_log) if 1 <= window_n_log <= 24 and width in (1, 2, 4, 8) else 0


def pack_header(row, page_n, dtype, window_n_log, version=1):
    return [version, row, (page_n & 0xFFFFFFFF) | (dtype << 32), window_n_log, 0, 0, 0, 0]


def reach(row, state_n, page_n):
    return min(row + state_n, page_n)


def restated_update_rows(fresh, from_row, to_row, state_n, page_n, window_n_log):
    """The last min(window_n, rows walked) of the rows the read computed"""
    old = 0 if fresh else reach(from_row, state_n, page_n)
    new = reach(to_row, state_n, page_n)
    walked = max(new - old, 0)
    return new - min(walked, 1 << window_n_log), new


def restated_history_verdict(hdr, history_len, resumes, from_row, page_n, dtype, window_n_log, width):
    need = history_bytes(window_n_log, width)
    if need == 0 or history_len < need:
        return G.ST_INVALID_ARGUMENT
    if not resumes:
        return G.ST_OK
    if hdr[0] != 1 or hdr[2] != ((page_n & 0xFFFFFFFF) | (dtype << 32)) or hdr[3] != window_n_log or hdr[1] != from_row:
        return G.ST_INVALID_ARGUMENT
    return G.ST_OK


def restated_verdict_lookback(w, **scene):
    c = A.unpack_cursor(w)
    if c["kind"] != LOOKBACK:
        return G.ST_INVALID_ARGUMENT
    return GA.restated_verdict_general(A.pack_cursor(GA.GENERAL, c["row"], c["bit"], c["page_n"], c["dtype"], c["states"], None, c["version"]), **scene)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the struct, the exports, the size function
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_lays_the_task_out_as_the_header_does():
    want = A.header_fields("PcoGfxPageReadHistTask")
    assert [n for n, _ in want] == ["meta", "meta_len", "page", "page_len", "dst", "page_n", "first", "count", "dtype", "format_major", "from", "to", "history", "history_len"]
    assert [("from" if n == "from_" else n, t) for n, t in G.PageReadHistTask._fields_] == want
    assert C.sizeof(G.PageReadHistTask) == 104
    assert G.PageReadHistTask._fields_[:12] == G.PageReadTask._fields_
    at = 0
    for n, t in G.PageReadHistTask._fields_:
        assert getattr(G.PageReadHistTask, n).offset == at, n
        at += C.sizeof(t)


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(HEADER).read()
    assert re.search(r"#define PCO_GFX_HISTORY_HEADER_BYTES 64\b", text)
    assert re.search(r"size_t pco_gfx_lookback_history_bytes\(uint32_t window_n_log, unsigned char dtype\);", text)
    assert re.search(r"enum PcoError pco_gfx_decompress_page_reads_hist\(size_t n_tasks, const PcoGfxPageReadHistTask\* tasks, uint32_t flags,\s*PcoGfxTaskResult\* results,"
                     r"\s*PcoGfxTaskResult\* d_results, void\* stream\);", text)
    assert hasattr(G.lib(), "pco_gfx_decompress_page_reads_hist") and hasattr(G.lib(), "pco_gfx_lookback_history_bytes")
    assert G.CURSOR_LOOKBACK_KIND == LOOKBACK and G.HISTORY_HEADER_BYTES == HEADER_BYTES
    assert re.search(r"kCursorLookback = 4;", open(os.path.join(CSRC, "pco_cursor.h")).read())
    hist = open(os.path.join(CSRC, "pco_history.h")).read()
    assert re.search(r"kHistoryHeaderBytes = 64, kHistoryHeaderWords = 8;", hist) and re.search(r"kHistoryVersion = 1;", hist)


@pytest.mark.parametrize("window_n_log", [1, 15, 24, 0, 25])
def test_the_size_of_a_history_over_every_number_type(window_n_log):
    L = G.lib()
    for t in G.NUMBER_TYPES:
        want = 64 + (1 << window_n_log) * t.width if 1 <= window_n_log <= 24 else 0
        assert L.pco_gfx_lookback_history_bytes(window_n_log, t.byte) == want == history_bytes(window_n_log, t.width), (t.name, window_n_log)
    for bad in (0, 12, 255):
        assert L.pco_gfx_lookback_history_bytes(window_n_log, bad) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
GOOD_TASK = dict(A.GOOD_TASK, history=A.P, history_len=64 + 16)
HISTORY_CHECKS = [
    (dict(task=dict(history=A.P, history_len=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history=None, history_len=80)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history=A.P + 4)), G.ST_INVALID_ARGUMENT),          # misaligned
    (dict(task=dict(history=A.P + 1)), G.ST_INVALID_ARGUMENT),
]


def call_hist(flags=0, task=None, no_tasks=False, no_results=False, form="sync"):
    L = G.lib()
    kw = dict(GOOD_TASK); kw.update(task or {})
    arr = (G.PageReadHistTask * 1)(G.PageReadHistTask(**kw))
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    if form == "sync":
        code = L.pco_gfx_decompress_page_reads_hist(1, None if no_tasks else arr, flags, None if no_results else res, None, None)
    else:   # (d_results is a device pointer the refused call never touches)
        code = L.pco_gfx_decompress_page_reads_hist(1, None if no_tasks else arr, flags, None, None if no_results else A.P, None)
    return code, L.pco_gfx_last_status(), res[0]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags", [0, FLAG])
@pytest.mark.parametrize("kw,status", A.CHECKS + HISTORY_CHECKS)
def test_every_host_check_comes_before_a_device_is_asked_for(kw, status, flags, form):
    code, st, res = call_hist(flags, form=form, **kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)   # nothing was written


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags", [2, 3, 4, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF])
def test_an_unknown_flag_bit_is_refused_before_anything_else(flags, form):
    code, st, res = call_hist(flags, form=form)
    assert code == G.PcoDecompressionError and st == G.ST_INVALID_ARGUMENT
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)


def test_a_task_without_a_history_passes_the_history_checks():
    """history == NULL with history_len == 0 is the _ex task: what refuses the call below is the device that is (or is not) there, not an argument"""
    code, st, _ = call_hist(task=dict(history=None, history_len=0, page_n=0))
    assert code == G.PcoDecompressionError and st == G.ST_INVALID_ARGUMENT   # (page_n == 0: the ten-field checks still run)


@pytest.mark.parametrize("flags", [0, FLAG])
def test_no_tasks_is_a_success_without_a_device(flags):
    res = (G.TaskResult * 1)()
    assert G.lib().pco_gfx_decompress_page_reads_hist(0, None, flags, res, None, None) == G.PcoSuccess
    assert G.lib().pco_gfx_decompress_page_reads_hist(0, None, flags, None, None, None) == G.PcoSuccess


# ---------------------------------------------------------------------------------------------------------------------------------------
# pco_history.h and the kind-4 verdict, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hist_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("historyverdict")
    src = d / "history.cpp"
    src.write_text(f'''
#include "{CSRC}/pco_cursor.h"
#include "{CSRC}/pco_history.h"
using namespace pcogfx;
extern "C" uint64_t bytes(uint32_t window_n_log, uint32_t width) {{ return history_bytes(window_n_log, width); }}
extern "C" uint64_t slot(uint64_t j, uint32_t window_n_log) {{ return history_slot(j, window_n_log); }}
extern "C" uint64_t reach(uint64_t row, uint64_t state_n, uint64_t page_n) {{ return history_reach(row, state_n, page_n); }}
extern "C" void header(uint64_t row, uint64_t page_n, uint32_t dtype, uint32_t window_n_log, uint64_t* out) {{
  for (uint32_t i = 0; i < kHistoryHeaderWords; i++) out[i] = history_header_word(i, row, page_n, dtype, window_n_log);
}}
extern "C" void update_rows(int fresh, uint64_t from_row, uint64_t to_row, uint64_t state_n, uint64_t page_n, uint32_t window_n_log, uint64_t* out) {{
  const HistoryRows r = history_update_rows(fresh != 0, from_row, to_row, state_n, page_n, window_n_log);
  out[0] = r.lo; out[1] = r.hi;
}}
extern "C" uint32_t hist_verdict(const uint64_t* hdr, uint64_t history_len, int resumes, uint64_t from_row, uint64_t page_n, uint32_t dtype, uint32_t window_n_log, uint32_t width) {{
  return history_verdict(hdr, history_len, resumes != 0, from_row, page_n, dtype, window_n_log, width);
}}
extern "C" uint32_t verdict(const uint64_t* w, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits, const uint32_t* asl,
                            uint64_t end_batch, uint64_t walk_cap) {{
  return cursor_verdict_lookback(w, page_n, dtype, first, body_first_bit, page_bits, asl, end_batch, walk_cap);
}}
extern "C" uint32_t general_verdict(const uint64_t* w, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits, const uint32_t* asl,
                                    uint64_t end_batch, uint64_t walk_cap) {{
  return cursor_verdict_general(w, page_n, dtype, first, body_first_bit, page_bits, asl, end_batch, walk_cap);
}}
extern "C" uint32_t old_verdict(const uint64_t* w, uint32_t want_kind, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits, const uint32_t* asl) {{
  return cursor_verdict(w, want_kind, page_n, dtype, first, body_first_bit, page_bits, asl);
}}
extern "C" void words(uint64_t row, uint64_t bit, uint64_t page_n, uint32_t dtype, const uint32_t* states, uint64_t* out) {{
  for (uint32_t i = 0; i < kCursorWords; i++) {{
    const uint32_t s = i >= kCursorStateWord && i < kCursorMomentWord ? 2 * (i - kCursorStateWord) : 0;
    out[i] = cursor_word_lookback(i, row, bit, page_n, dtype, (uint64_t)states[s] | ((uint64_t)states[s + 1] << 32));
  }}
}}
''')
    out = d / "libhistory.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    u32, u64, p, i = C.c_uint32, C.c_uint64, C.c_void_p, C.c_int
    for name, res, args in (("bytes", u64, [u32, u32]), ("slot", u64, [u64, u32]), ("reach", u64, [u64, u64, u64]), ("header", None, [u64, u64, u32, u32, p]),
                            ("update_rows", None, [i, u64, u64, u64, u64, u32, p]), ("hist_verdict", u32, [p, u64, i, u64, u64, u32, u32, u32]),
                            ("verdict", u32, [p, u64, u32, u64, u64, u64, p, u64, u64]), ("general_verdict", u32, [p, u64, u32, u64, u64, u64, p, u64, u64]),
                            ("old_verdict", u32, [p, u32, u64, u32, u64, u64, u64, p]), ("words", None, [u64, u64, u64, u32, p, p])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def c_update_rows(lib, *args):
    out = (C.c_uint64 * 2)()
    lib.update_rows(int(args[0]), *args[1:], out)
    return out[0], out[1]


def walked_grid(w):
    return sorted({0, 1, 255, 256, 257, max(w - 1, 0), w, w + 1})


def test_sizes_slots_reach_and_the_header_words(hist_lib):
    for wl in list(range(0, 27)):
        for width in (0, 1, 2, 3, 4, 8, 16):
            assert hist_lib.bytes(wl, width) == history_bytes(wl, width), (wl, width)
    for wl in range(1, 10):
        w = 1 << wl
        for j in (0, 1, w - 1, w, w + 1, 3 * w + 5, (1 << 24) - 1, ALL_ONES):
            assert hist_lib.slot(j, wl) == j % w < w
    for row, state_n, page_n in ((0, 1, 3000), (2816, 256, 3000), (2816, 1, 3000), (3000, 2, 3000), (2560, 256, 2816), (0, 256, 256)):
        assert hist_lib.reach(row, state_n, page_n) == reach(row, state_n, page_n)
    out = (C.c_uint64 * 8)(*([ALL_ONES] * 8))
    hist_lib.header(768, 3000, 6, 9, out)
    assert list(out) == pack_header(768, 3000, 6, 9) == [1, 768, 3000 | (6 << 32), 9, 0, 0, 0, 0]


def test_the_update_interval_against_its_restatement(hist_lib):
    """window_n_log 1..9 x rows walked 0/1/255/256/257/w-1/w/w+1 x state_n 1/2/256 x a start in the page, at its front and near its end"""
    n = 0
    for wl in range(1, 10):
        for state_n in (1, 2, 256):
            if state_n > 1 << wl:
                continue   # (the format: state_n_log <= window_n_log)
            for page_n in (3000, 2816, 600):
                for from_row in (0, 256, 512, page_n - page_n % 256 if page_n % 256 else page_n - 256, page_n):
                    for walked in walked_grid(1 << wl):
                        to_row = min(from_row + walked, page_n)
                        for fresh in (False, True):
                            if fresh and from_row:
                                continue
                            args = (fresh, from_row, to_row, state_n, page_n, wl)
                            lo, hi = c_update_rows(hist_lib, *args)
                            assert (lo, hi) == restated_update_rows(*args), args
                            assert hi == reach(to_row, state_n, page_n) and 0 <= lo <= hi and hi - lo <= 1 << wl, args
                            n += 1
    assert n > 2000


class RingModel:
    """slot -> the row whose latent it holds; None: the caller's bytes"""

    def __init__(self, window_n_log):
        self.wl, self.slots, self.row = window_n_log, [None] * (1 << window_n_log), None

    def read(self, lib, fresh, from_row, to_row, state_n, page_n):
        lo, hi = c_update_rows(lib, fresh, from_row, to_row, state_n, page_n, self.wl)
        written = set()
        for j in range(lo, hi):
            s = lib.slot(j, self.wl)
            assert s not in written, ("a slot is written twice in one update", self.wl, from_row, to_row, j)
            written.add(s); self.slots[s] = j
        self.row = to_row

    def check(self, state_n, page_n):
        """exactly the rows the stamp promises: F[j] at j & (w - 1) for j in [max(0, reach - w), reach), the other slots untouched"""
        w = 1 << self.wl
        r = reach(self.row, state_n, page_n)
        want = [None] * w
        for j in range(max(0, r - w), r):
            want[j % w] = j
        assert self.slots == want, (self.wl, self.row, state_n, page_n)


@pytest.mark.parametrize("window_n_log", range(1, 10))
def test_the_update_never_writes_a_slot_twice_and_leaves_the_rows_the_stamp_promises(hist_lib, window_n_log):
    w = 1 << window_n_log
    for state_n in (1, 2, 256):
        if state_n > w:
            continue
        for page_n in (3000, 2816, 300, 256, max(state_n, 2)):
            if page_n < state_n:
                continue
            for step in walked_grid(w) + [768, page_n]:
                if step == 0:
                    continue
                ring = RingModel(window_n_log)
                row = 0; fresh = True
                while True:
                    to = min(row + step, page_n)
                    ring.read(hist_lib, fresh, row, to, state_n, page_n)
                    ring.check(state_n, page_n)
                    fresh = False; row = to
                    if row == page_n:
                        break
                one = RingModel(window_n_log)
                one.read(hist_lib, True, 0, page_n, state_n, page_n)
                assert one.slots == ring.slots, "the ring after one read and after many"
                # a read that walks nothing (rows walked 0) writes nothing
                before = list(ring.slots)
                ring.read(hist_lib, False, page_n, page_n, state_n, page_n)
                assert ring.slots == before


HDR_SCENE = dict(history_len=64 + 8 * 512, resumes=True, from_row=512, page_n=3000, dtype=2, window_n_log=9, width=8)
HDR_ROWS = [
    ("a header that passes", pack_header(512, 3000, 2, 9), {}, G.ST_OK),
    ("exactly the bytes of the window", pack_header(512, 3000, 2, 9), dict(history_len=64 + 4096), G.ST_OK),
    ("one byte short", pack_header(512, 3000, 2, 9), dict(history_len=64 + 4095), G.ST_INVALID_ARGUMENT),
    ("one byte short, and the page starts", pack_header(512, 3000, 2, 9), dict(history_len=64 + 4095, resumes=False), G.ST_INVALID_ARGUMENT),
    ("the header alone", pack_header(512, 3000, 2, 9), dict(history_len=64), G.ST_INVALID_ARGUMENT),
    ("a wrong version", pack_header(512, 3000, 2, 9, version=2), {}, G.ST_INVALID_ARGUMENT),
    ("version 0", pack_header(512, 3000, 2, 9, version=0), {}, G.ST_INVALID_ARGUMENT),
    ("another page_n", pack_header(512, 2999, 2, 9), {}, G.ST_INVALID_ARGUMENT),
    ("another dtype", pack_header(512, 3000, 4, 9), {}, G.ST_INVALID_ARGUMENT),
    ("another window", pack_header(512, 3000, 2, 8), {}, G.ST_INVALID_ARGUMENT),
    ("a larger window than the page's", pack_header(512, 3000, 2, 10), {}, G.ST_INVALID_ARGUMENT),
    ("another row", pack_header(768, 3000, 2, 9), {}, G.ST_INVALID_ARGUMENT),
    ("row 0 where the cursor stands at 512", pack_header(0, 3000, 2, 9), {}, G.ST_INVALID_ARGUMENT),
    ("garbage, but the page starts: the header need not be valid", [ALL_ONES] * 8, dict(resumes=False), G.ST_OK),
    ("garbage, resumed", [ALL_ONES] * 8, {}, G.ST_INVALID_ARGUMENT),
    ("a window_n_log outside the format", pack_header(512, 3000, 2, 25), dict(window_n_log=25, history_len=1 << 40), G.ST_INVALID_ARGUMENT),
]


@pytest.mark.parametrize("row", HDR_ROWS, ids=[r[0] for r in HDR_ROWS])
def test_the_header_verdict_against_its_restatement(hist_lib, row):
    _, hdr, diff, status = row
    scene = dict(HDR_SCENE); scene.update(diff)
    assert restated_history_verdict(hdr, **scene) == status
    assert hist_lib.hist_verdict((C.c_uint64 * 8)(*hdr), scene["history_len"], int(scene["resumes"]), scene["from_row"], scene["page_n"], scene["dtype"],
                                 scene["window_n_log"], scene["width"]) == status


def test_the_header_verdict_over_a_small_grid(hist_lib):
    n = 0
    for version in (0, 1, 2):
        for hrow in (0, 256, 512):
            for page_n in (3000, 2999):
                for dtype in (2, 4):
                    for hwl in (1, 8, 9):
                        for wl in (1, 8, 9):
                            for width in (1, 8):
                                for length in (0, 63, 64, 64 + (width << wl) - 1, 64 + (width << wl), 1 << 30):
                                    for resumes in (False, True):
                                        hdr = pack_header(hrow, page_n, dtype, hwl, version)
                                        args = dict(history_len=length, resumes=resumes, from_row=256, page_n=3000, dtype=2, window_n_log=wl, width=width)
                                        got = hist_lib.hist_verdict((C.c_uint64 * 8)(*hdr), length, int(resumes), 256, 3000, 2, wl, width)
                                        assert got == restated_history_verdict(hdr, **args), (hdr, args)
                                        n += 1
    assert n == 3 * 3 * 2 * 2 * 3 * 3 * 2 * 6 * 2


ASL = [6, 14, 2]
STATES = [[1, 2, 3, 63], [5, 6, 7, (1 << 14) - 1], [1, 2, 3, 3]]
SCENE = dict(page_n=3000, dtype=1, first=600, body_first_bit=40, page_bits=8000, end_batch=4, walk_cap=2)


def good(**kw):
    d = dict(row=512, bit=1000, page_n=3000, dtype=1, states=[list(s) for s in STATES])
    d.update(kw)
    return pack_lookback(**d)


def with_state(v, j, x):
    s = [list(r) for r in STATES]; s[v][j] = x
    return good(states=s)


def run_verdict(lib, w, page_n, dtype, first, body_first_bit, page_bits, asl, end_batch, walk_cap, fn="verdict"):
    return getattr(lib, fn)((C.c_uint64 * 32)(*w), page_n, dtype, first, body_first_bit, page_bits, (C.c_uint32 * 3)(*asl), end_batch, walk_cap)


ROWS = [
    ("a cursor that passes", good(), {}, G.ST_OK),
    ("a wrong version", good(version=2), {}, G.ST_INVALID_ARGUMENT),
    ("kind 1", good(kind=A.FULL), {}, G.ST_INVALID_ARGUMENT),
    ("kind 2", good(kind=A.POSITION), {}, G.ST_INVALID_ARGUMENT),
    ("kind 3", good(kind=GA.GENERAL), {}, G.ST_INVALID_ARGUMENT),
    ("kind 5", good(kind=5), {}, G.ST_INVALID_ARGUMENT),
    ("another page_n", good(page_n=2999), {}, G.ST_INVALID_ARGUMENT),
    ("another dtype", good(dtype=3), {}, G.ST_INVALID_ARGUMENT),
    ("at > first", good(row=768), {}, G.ST_INVALID_ARGUMENT),
    ("at == first", good(), dict(first=512), G.ST_OK),
    ("at neither a multiple of 256 nor page_n", good(row=300), {}, G.ST_INVALID_ARGUMENT),
    ("at == page_n", good(row=3000), dict(first=3000, end_batch=12, walk_cap=1), G.ST_OK),
    ("one bit in front of the body", good(bit=39), {}, G.ST_INVALID_ARGUMENT),
    ("the body's first bit", good(bit=40), {}, G.ST_OK),
    ("one bit beyond the page", good(bit=8001), {}, G.ST_INVALID_ARGUMENT),
    ("the delta variable's state 2^asl - 1", with_state(0, 3, 63), {}, G.ST_OK),
    ("the delta variable's state 2^asl", with_state(0, 3, 64), {}, G.ST_INVALID_ARGUMENT),
    ("the primary's state 2^asl", with_state(1, 0, 1 << 14), {}, G.ST_INVALID_ARGUMENT),
    ("the secondary's state 2^asl", with_state(2, 3, 4), {}, G.ST_INVALID_ARGUMENT),
    ("a state of all ones", with_state(0, 2, 0xFFFFFFFF), {}, G.ST_INVALID_ARGUMENT),
    ("exactly the batches the host gave scratch for", good(), dict(walk_cap=2), G.ST_OK),
    ("one batch more than the host gave scratch for", good(), dict(walk_cap=1), G.ST_INVALID_ARGUMENT),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_the_kind_4_verdict_against_its_restatement(hist_lib, row):
    _, w, diff, status = row
    scene = dict(SCENE); scene.update(diff)
    assert restated_verdict_lookback(w, asl=ASL, **scene) == status
    assert run_verdict(hist_lib, w, asl=ASL, **scene) == status


def test_the_kind_4_verdict_over_a_small_grid(hist_lib):
    n = 0
    for version in (0, 1, 2):
        for kind in (1, 2, 3, 4, 5):
            for row in (0, 256, 300, 512, 3000):
                for first in (0, 256, 511, 3000):
                    for page_n in (3000, 2999):
                        for bit in (39, 40, 8000, 8001):
                            for st in (0, 63, 64):
                                for cap in (0, 1, 12):
                                    s = [list(r) for r in STATES]; s[0][1] = st
                                    w = pack_lookback(row, bit, page_n, 1, s, version, kind)
                                    args = dict(page_n=3000, dtype=1, first=first, body_first_bit=40, page_bits=8000, asl=ASL, end_batch=(first + 1 + 255) // 256, walk_cap=cap)
                                    assert run_verdict(hist_lib, w, **args) == restated_verdict_lookback(w, **args), (version, kind, row, first, page_n, bit, st, cap)
                                    n += 1
    assert n == 3 * 5 * 5 * 4 * 2 * 4 * 3 * 3


def test_kind_4_refuses_kinds_1_to_3_and_they_refuse_it(hist_lib):
    asl = (C.c_uint32 * 3)(*ASL)
    w4 = (C.c_uint64 * 32)(*good())
    for want in (A.FULL, A.POSITION):
        assert hist_lib.old_verdict(w4, want, 3000, 1, 600, 40, 8000, asl) == G.ST_INVALID_ARGUMENT
    assert run_verdict(hist_lib, good(), asl=ASL, fn="general_verdict", **SCENE) == G.ST_INVALID_ARGUMENT
    for kind in (A.FULL, A.POSITION, GA.GENERAL):
        assert run_verdict(hist_lib, A.pack_cursor(kind, 512, 1000, 3000, 1, STATES), asl=ASL, **SCENE) == G.ST_INVALID_ARGUMENT
    # ... and each accepts its own
    assert run_verdict(hist_lib, good(), asl=ASL, **SCENE) == G.ST_OK
    assert run_verdict(hist_lib, GA.pack_general(512, 1000, 3000, 1, STATES), asl=ASL, fn="general_verdict", **SCENE) == G.ST_OK


def test_the_word_writer_is_the_documented_layout(hist_lib):
    st = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]
    out = (C.c_uint64 * 32)(*([ALL_ONES] * 32))
    hist_lib.words(768, 12345, 3000, 6, (C.c_uint32 * 12)(*st), out)
    want = pack_lookback(768, 12345, 3000, 6, [st[0:4], st[4:8], st[8:12]])
    assert list(out) == want and list(out)[10:] == [0] * 22
    c = A.unpack_cursor(out)
    assert (c["version"], c["kind"], c["row"], c["bit"], c["page_n"], c["dtype"]) == (1, LOOKBACK, 768, 12345, 3000, 6)
    assert c["states"] == [st[0:4], st[4:8], st[8:12]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tANS model, batch by batch, over a Lookback page: the delta variable, the primary and (in the two-variable modes) the secondary
# ---------------------------------------------------------------------------------------------------------------------------------------
OB_BITS = {8: 4, 16: 5, 32: 6, 64: 7}


def model_lookback(meta, page, n, latent_bits):
    """tests/tans_model.py stepped batch by batch over a Lookback page in Classic, IntMult, FloatMult or FloatQuant mode (metadata/chunk.rs,
    page.rs, page_latent_decompressor.rs): dict(window_n_log, state_n_log, body = the body's first bit, marks = [(row, bit position, [the four
    state indices of the delta variable, the primary, the secondary])] at every batch boundary and at the page's end, size_logs, lookbacks = the
    delta variable's latents, F = the primary's latents after the lookback decode (delta/lookback.rs), secondary = its latents or None)."""
    r = TM.Bits(meta)
    mode = r.read(4)
    assert mode in (0, 1, 2, 3)
    if mode in (1, 2):
        r.read(latent_bits)
    elif mode == 3:
        r.read(8)
    assert r.read(4) == 2, "Lookback only"
    wlog = 1 + r.read(5); slog = r.read(4); sec_delta = r.read(1)
    assert sec_delta == 0, "no delta'd secondary"
    present = [True, True, mode != 0]
    bits_of = [32, latent_bits, latent_bits]
    tables = []
    for v in range(3):
        if not present[v]:
            tables.append(None); continue
        size_log = r.read(4); n_bins = r.read(15)
        bins = [(r.read(size_log) + 1, r.read(bits_of[v]), r.read(OB_BITS[bits_of[v]])) for _ in range(n_bins)]
        tables.append((size_log, bins, TM.decoder_nodes(size_log, [b[0] for b in bins]) if n_bins else None))
    r.align()
    assert r.pos == r.n
    state_n = 1 << slog
    b = TM.Bits(page)
    states = [[0] * 4 for _ in range(3)]
    header_state = []
    for v in range(3):
        if not present[v]:
            continue
        if v == 1:
            header_state = [b.read(latent_bits) for _ in range(state_n)]
        states[v] = [b.read(tables[v][0]) for _ in range(TM.INTERLEAVING)]
    b.align()
    body = b.pos
    mask = (1 << latent_bits) - 1; mid = 1 << (latent_bits - 1)
    F = list(header_state[:n]); lookbacks = []; secondary = [] if present[2] else None
    marks = []
    remaining = n
    for start in range(0, n, TM.BATCH_N):
        bn = min(TM.BATCH_N, remaining)
        out = [None, None, None]
        for v in range(3):
            if not present[v]:
                continue
            rem = max(remaining - state_n, 0) if v < 2 else remaining
            cnt = min(rem, bn) if v == 0 else min(rem, TM.BATCH_N)
            size_log, bins, nodes = tables[v]
            syms = []
            for i in range(cnt):
                if len(bins) == 1:
                    syms.append(0); continue
                j = i % TM.INTERLEAVING
                s, nbits, base = nodes[states[v][j]]
                syms.append(s); states[v][j] = base + b.read(nbits)
            out[v] = [(bins[s][1] + b.read(bins[s][2])) & ((1 << bits_of[v]) - 1) for s in syms]
        for lb, d in zip(out[0], out[1]):
            assert 1 <= lb <= min(1 << wlog, len(F)), "a lookback inside the window and the page"
            lookbacks.append(lb); F.append((d + mid + F[len(F) - lb]) & mask)
        if present[2]:
            secondary += out[2]
        remaining -= bn
        marks.append((start + bn, b.pos, [list(states[0]), list(states[1]), list(states[2])]))
    b.align()
    assert b.pos == b.n and len(F) == n
    return dict(window_n_log=wlog, state_n_log=slog, body=body, marks=marks, size_logs=[t[0] if t else 0 for t in tables], lookbacks=lookbacks, F=F, secondary=secondary)


def lookback_page(dt, n, window_n_log, state_n_log, seed, mode=O.MODE_CLASSIC, **kw):
    rng = np.random.default_rng(seed + 1)
    if mode == O.MODE_TRY_INT_MULT:
        x = (rng.integers(0, 300, n) * 10 + rng.integers(0, 4, n)).astype(dt)
        kw = dict(kw, mode_u64=10)
    else:
        hi = 200 if np.dtype(dt).itemsize == 1 else 5000
        x = (np.tile(rng.integers(0, hi, 37), n // 37 + 1)[:n] + rng.integers(0, 3, n)).astype(dt)
    meta, pages = O.test_encode(x, pages=[n], mode=mode, delta=O.TE_DELTA_LOOKBACK, window_n_log=window_n_log, state_n_log=state_n_log, lookback_seed=seed, **kw)
    return x, meta, pages[0]


@pytest.mark.parametrize("dt,n,wl,sl,seed,mode", [(np.uint32, 3000, 4, 0, 3, O.MODE_CLASSIC), (np.uint8, 2816, 8, 4, 5, O.MODE_CLASSIC), (np.uint64, 700, 9, 8, 0, O.MODE_CLASSIC),
                                                  (np.uint16, 600, 1, 1, 7, O.MODE_CLASSIC), (np.int64, 3000, 12, 1, 9, O.MODE_TRY_INT_MULT)])
def test_the_stepped_model_decodes_a_lookback_page(dt, n, wl, sl, seed, mode):
    x, meta, page = lookback_page(dt, n, wl, sl, seed, mode)
    ok, err, in_meta = O.wrapped_page_prefix(meta, page, x.dtype, n)
    assert err == 0 and not in_meta and np.array_equal(ok.view(x.dtype), x), "the oracle decodes the page to the input"
    bits = np.dtype(dt).itemsize * 8
    m = model_lookback(meta, page, n, bits)
    assert (m["window_n_log"], m["state_n_log"]) == (wl, sl)
    lat = [int(v) for v in TM.to_latent(x)]
    if mode == O.MODE_CLASSIC:
        assert m["F"] == lat and m["secondary"] is None
    else:
        assert [p * 10 + s for p, s in zip(m["F"], m["secondary"])] == lat
    assert [k[0] for k in m["marks"]] == [min(r + 256, n) for r in range(0, n, 256)]
    assert all(a[1] <= b[1] for a, b in zip(m["marks"], m["marks"][1:])) and m["body"] <= m["marks"][0][1] and m["marks"][-1][1] <= 8 * len(page)
    assert all(0 <= s < 1 << m["size_logs"][v] for k in m["marks"] for v in range(3) for s in k[2][v])
    assert len(m["lookbacks"]) == n - (1 << sl)
