"""CPU: the ABI of pco_gfx_index_pages_hist (include/pco_gfx.h section 4j) -- the task struct against the header and against a g++ offsetof probe, every
host check answered without a device, and the snapshot arithmetic of pcodec_amd/csrc/pco_history.h compiled on its own with g++ (the lines
index_history_snapshot_kernel runs) against a Python restatement and against the union of what a chain of reads writes."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import test_page_reads_abi as A  # noqa: E402  (header_fields, HEADER, CSRC)
import test_page_index_abi as IA  # noqa: E402  (the index task's host checks)
import test_lookback_history_abi as HA  # noqa: E402  (reach, restated_update_rows)
from pcodec_amd import _lib as G  # noqa: E402

FLAG = 1   # PCO_GFX_CURSOR_GENERAL
FIELDS = ["meta", "meta_len", "page", "page_len", "cursors", "page_n", "every_rows", "dtype", "format_major", "histories", "history_stride"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the struct and the exports
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_lays_the_task_out_as_the_header_does(tmp_path):
    want = A.header_fields("PcoGfxPageIndexHistTask")
    assert [n for n, _ in want] == FIELDS and list(G.PageIndexHistTask._fields_) == want
    assert C.sizeof(G.PageIndexHistTask) == 80 and G.PageIndexHistTask._fields_[:9] == G.PageIndexTask._fields_
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "%s"\nint main() { printf("%%zu", sizeof(PcoGfxPageIndexHistTask));\n%s\nreturn 0; }\n' % (
        os.path.abspath(A.HEADER), "\n".join('printf(" %%zu", offsetof(PcoGfxPageIndexHistTask, %s));' % f for f in FIELDS)))
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    size, *offsets = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert size == 80 and offsets == [getattr(G.PageIndexHistTask, n).offset for n in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72]


def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    text = open(A.HEADER).read()
    assert re.search(r"enum PcoError pco_gfx_index_pages_hist\(size_t n_tasks, const PcoGfxPageIndexHistTask\* tasks, uint32_t flags,\s*PcoGfxTaskResult\* results,"
                     r"\s*PcoGfxTaskResult\* d_results, void\* stream\);", text)
    assert hasattr(G.lib(), "pco_gfx_index_pages_hist")
    hist = open(os.path.join(A.CSRC, "pco_history.h")).read()
    assert "history_snapshot_rows" in hist and "history_at" in hist and "__device__" not in hist.replace("#define PCO_HIST_HD __host__ __device__", "")


# ---------------------------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
P = IA.P
GOOD_TASK = dict(IA.GOOD_TASK, histories=P, history_stride=64 + 16)
HISTORY_CHECKS = [
    (dict(task=dict(histories=P, history_stride=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(histories=None, history_stride=80)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(history_stride=84)), G.ST_INVALID_ARGUMENT),          # no multiple of 8
    (dict(task=dict(history_stride=81)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(histories=P + 4)), G.ST_INVALID_ARGUMENT),           # misaligned
    (dict(task=dict(histories=P + 1)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(histories=P, history_stride=0, page_n=50)), G.ST_INVALID_ARGUMENT),   # the pair is judged whatever k is
]


def call_hist(flags=0, task=None, no_tasks=False, no_results=False, form="sync"):
    L = G.lib()
    kw = dict(GOOD_TASK); kw.update(task or {})
    arr = (G.PageIndexHistTask * 1)(G.PageIndexHistTask(**kw))
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    if form == "sync":
        code = L.pco_gfx_index_pages_hist(1, None if no_tasks else arr, flags, None if no_results else res, None, None)
    else:   # (d_results is a device pointer the refused call never touches)
        code = L.pco_gfx_index_pages_hist(1, None if no_tasks else arr, flags, None, None if no_results else P, None)
    return code, L.pco_gfx_last_status(), res[0]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags", [0, FLAG])
@pytest.mark.parametrize("kw,status", IA.CHECKS + HISTORY_CHECKS)
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


@pytest.mark.parametrize("flags", [0, FLAG])
def test_no_tasks_is_a_success_without_a_device(flags):
    res = (G.TaskResult * 1)()
    assert G.lib().pco_gfx_index_pages_hist(0, None, flags, res, None, None) == G.PcoSuccess
    assert G.lib().pco_gfx_index_pages_hist(0, None, flags, None, None, None) == G.PcoSuccess


# ---------------------------------------------------------------------------------------------------------------------------------------
# pco_history.h's snapshot arithmetic, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snap_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("historysnapshot")
    src = d / "snapshot.cpp"
    src.write_text(f'''
#include "{A.CSRC}/pco_history.h"
using namespace pcogfx;
extern "C" void snapshot_rows(uint64_t row, uint64_t state_n, uint64_t page_n, uint32_t window_n_log, uint64_t* out) {{
  const HistoryRows r = history_snapshot_rows(row, state_n, page_n, window_n_log);
  out[0] = r.lo; out[1] = r.hi;
}}
extern "C" void update_rows(int fresh, uint64_t from_row, uint64_t to_row, uint64_t state_n, uint64_t page_n, uint32_t window_n_log, uint64_t* out) {{
  const HistoryRows r = history_update_rows(fresh != 0, from_row, to_row, state_n, page_n, window_n_log);
  out[0] = r.lo; out[1] = r.hi;
}}
extern "C" uint64_t slot(uint64_t j, uint32_t window_n_log) {{ return history_slot(j, window_n_log); }}
extern "C" uint64_t at(uint64_t histories, uint64_t stride, uint64_t i) {{ return (uint64_t)(uintptr_t)history_at((void*)(uintptr_t)histories, stride, i); }}
''')
    out = d / "libsnapshot.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    u32, u64, p, i = C.c_uint32, C.c_uint64, C.c_void_p, C.c_int
    for name, res, args in (("snapshot_rows", None, [u64, u64, u64, u32, p]), ("update_rows", None, [i, u64, u64, u64, u64, u32, p]), ("slot", u64, [u64, u32]),
                            ("at", u64, [u64, u64, u64])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def restated_snapshot_rows(row, state_n, page_n, window_n_log):
    r = min(row + state_n, page_n)
    return max(0, r - (1 << window_n_log)), r


def c_rows(fn, *args):
    out = (C.c_uint64 * 2)()
    fn(*args, out)
    return out[0], out[1]


def test_the_snapshot_rows_against_their_restatement(snap_lib):
    n = 0
    for wl in (1, 2, 8, 9, 12, 24):
        w = 1 << wl
        for state_n in (1, 2, 16, 256):
            # reach one below, on and one above window_n; row + state_n one below, on and above page_n
            for row, page_n in [(w - state_n - 1, w + 1000), (w - state_n, w + 1000), (w - state_n + 1, w + 1000), (256, 256 + state_n + 1), (256, 256 + state_n),
                                (256, 256 + state_n - 1 if state_n > 1 else 257), (512, 513), (2816, 3000), (0, 5)]:
                if row < 0 or page_n <= row:
                    continue
                got = c_rows(snap_lib.snapshot_rows, row, state_n, page_n, wl)
                assert got == restated_snapshot_rows(row, state_n, page_n, wl) and got[1] == HA.reach(row, state_n, page_n) and got[1] - got[0] <= w, (wl, state_n, row, page_n)
                n += 1
    assert n > 150
    assert c_rows(snap_lib.snapshot_rows, 1 << 23, 256, 1 << 24, 24) == (0, (1 << 23) + 256) and c_rows(snap_lib.snapshot_rows, (1 << 24) - 256, 1, 1 << 24, 1) == ((1 << 24) - 257, (1 << 24) - 255)


def test_the_address_of_a_history_under_a_stride(snap_lib):
    for base, stride, i in [(0x1000, 80, 0), (0x1000, 80, 7), (0x7f0000000008, 64 + (8 << 24), 65534), (8, 72, 1)]:
        assert snap_lib.at(base, stride, i) == base + i * stride


@pytest.mark.parametrize("window_n_log", [1, 3, 8, 9, 12])
def test_a_chain_of_reads_leaves_exactly_the_slots_the_snapshot_writes(snap_lib, window_n_log):
    """The union of history_update_rows over a chain of reads from row 0 to r_i, replayed on a model ring: the slots it has written, and the row each
    holds, are those of history_snapshot_rows -- whatever the chain's steps."""
    w = 1 << window_n_log
    for page_n, state_n in ((3000, 1), (3000, 16), (2816, 256), (700, 2)):
        for step in (256, 512, 768):
            ring = {}; at = 0; fresh = True
            while at < page_n:
                to = min(at + step, page_n)
                lo, hi = c_rows(snap_lib.update_rows, int(fresh), at, to, state_n, page_n, window_n_log)
                assert (lo, hi) == HA.restated_update_rows(fresh, at, to, state_n, page_n, window_n_log)
                for j in range(lo, hi):
                    ring[snap_lib.slot(j, window_n_log)] = j
                at, fresh = to, False
                lo, hi = c_rows(snap_lib.snapshot_rows, at, state_n, page_n, window_n_log)
                assert ring == {j & (w - 1): j for j in range(lo, hi)}, (page_n, state_n, step, at)
