"""CPU: pco_gfx_take_rows (include/pco_gfx.h section 4n) without a device.

The task struct against the header and a gcc offsetof probe; every host check of the entry point in the header's order, in both forms, with its pinned
words and `results` untouched, beside the same call made good; pcodec_amd/csrc/pco_take.h compiled alone -- into a stand-alone program under
-fsanitize=address,undefined -- against the plain Python model of the plan (tests/take_model.py) on every case of the model; and the model's named
one-place mutants, each of which the cases must reveal."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import take_model as M  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import build as B  # noqa: E402

CSRC = os.path.abspath(os.path.join(HERE, "..", "pcodec_amd", "csrc"))
INCLUDE = os.path.abspath(os.path.join(HERE, "..", "include"))
INVALID, CORRUPTION, DEVICE = G.ST_INVALID_ARGUMENT, G.ST_CORRUPTION, G.ST_DEVICE_ERROR


@pytest.fixture(scope="module")
def lib():
    if B.needs_build():
        B.build()
    return G.lib()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the struct and the export
# ---------------------------------------------------------------------------------------------------------------------------------------
FIELDS = ["meta", "meta_len", "page", "page_len", "page_n", "row_base", "cursors", "every_rows", "d_rows", "n_rows", "dst", "dtype", "format_major"]
C_TYPES = {"const void*": C.c_void_p, "void*": C.c_void_p, "const PcoGfxPageCursor*": C.c_void_p, "const uint64_t*": C.c_void_p, "uint64_t": C.c_uint64,
           "uint32_t": C.c_uint32}


def header_fields():
    text = open(os.path.join(INCLUDE, "pco_gfx.h")).read()
    body = re.search(r"typedef struct PcoGfxTakeTask \{(.*?)\} PcoGfxTakeTask;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const void\*|void\*|const PcoGfxPageCursor\*|const uint64_t\*|uint64_t|uint32_t)\s+(.*)", decl)
        assert m, decl
        out += [(name.strip(), C_TYPES[m.group(1)]) for name in m.group(2).split(",")]
    return out


def test_the_binding_lays_the_take_task_out_as_the_header_does(tmp_path):
    assert G.TakeTask._fields_ == header_fields() and [n for n, _ in G.TakeTask._fields_] == FIELDS
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pco_gfx.h"\nint main(void) {\n  printf("%zu", sizeof(PcoGfxTakeTask));\n'
                   + "".join(f'  printf(" %zu", offsetof(PcoGfxTakeTask, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 96 == C.sizeof(G.TakeTask)
    assert got[1:] == [getattr(G.TakeTask, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 92]


def test_the_header_declares_the_entry_point_and_the_library_exports_it(lib):
    text = open(os.path.join(INCLUDE, "pco_gfx.h")).read()
    assert re.search(r"enum PcoError pco_gfx_take_rows\(size_t n_tasks, const PcoGfxTakeTask\* tasks, uint32_t flags, PcoGfxTaskResult\* results, PcoGfxTaskResult\* d_results,\s*void\* stream\);", text)
    assert hasattr(lib, "pco_gfx_take_rows") and G.SIGNATURES["pco_gfx_take_rows"] == G.SIGNATURES["pco_gfx_decompress_page_reads_ex"]
    for word in ("Lookback pages with histories", "the _dir forms", "32-bit row ids", "passes under a budget", "split the call"):
        assert word in text[text.index("4n. Rows by ROW ID"):], word   # (what the section says it does not cover, and its scratch limit)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
P = 0x1000   # (never dereferenced: every call below is refused by the argument checks, or finds no device)
GOOD = dict(meta=P, meta_len=10, page=P, page_len=10, page_n=1000, row_base=5, cursors=P, every_rows=256, d_rows=P, n_rows=4, dst=P, dtype=2, format_major=4)
# (name, the call's arguments, the task's fields, status, the refusal's words) in the order of the header's list
CHECKS = [
    ("null tasks", dict(no_tasks=True), {}, INVALID, "take rows: null task array"),
    ("no results", dict(no_results=True), {}, INVALID, "take rows: results and d_results are both null"),
    ("flag bit 1", dict(flags=2), {}, INVALID, "take rows: unknown flags"),
    ("flag bit 31", dict(flags=0x80000001), {}, INVALID, "take rows: unknown flags"),
    ("dtype 0", {}, dict(dtype=0), INVALID, "take rows task 0: invalid number type"),
    ("dtype 12", {}, dict(dtype=12), INVALID, "take rows task 0: invalid number type"),
    ("page_n 0", {}, dict(page_n=0), INVALID, "take rows task 0: a page holds 1 ..= 2^24 numbers"),
    ("page_n 2^24 + 1", {}, dict(page_n=(1 << 24) + 1), INVALID, "take rows task 0: a page holds 1 ..= 2^24 numbers"),
    ("null meta", {}, dict(meta=None), INVALID, "take rows task 0: null ChunkMeta or page"),
    ("null page", {}, dict(page=None), INVALID, "take rows task 0: null ChunkMeta or page"),
    ("row_base wraps", {}, dict(row_base=(1 << 64) - 1000), INVALID, "take rows task 0: row_base + page_n wraps"),
    ("every_rows 100", {}, dict(every_rows=100), INVALID, "take rows task 0: every_rows is a multiple of 256"),
    ("every_rows 2^64 - 1", {}, dict(every_rows=(1 << 64) - 1), INVALID, "take rows task 0: every_rows is a multiple of 256"),
    ("every_rows 0 with cursors", {}, dict(every_rows=0), INVALID, "take rows task 0: cursors and every_rows go together"),
    ("an index without cursors", {}, dict(cursors=None), INVALID, "take rows task 0: cursors and every_rows go together"),
    ("cursors off by 4", {}, dict(cursors=P + 4), INVALID, "take rows task 0: misaligned cursors"),
    ("cursors off by 1", {}, dict(cursors=P + 1), INVALID, "take rows task 0: misaligned cursors"),
    ("null d_rows", {}, dict(d_rows=None), INVALID, "take rows task 0: null or misaligned d_rows"),
    ("d_rows off by 4", {}, dict(d_rows=P + 4), INVALID, "take rows task 0: null or misaligned d_rows"),
    ("null dst", {}, dict(dst=None), INVALID, "take rows task 0: null or misaligned dst"),
    ("dst off by 4 for u64", {}, dict(dst=P + 4), INVALID, "take rows task 0: null or misaligned dst"),
    ("dst off by 1 for u16", {}, dict(dst=P + 1, dtype=7), INVALID, "take rows task 0: null or misaligned dst"),
    ("n_rows 2^32", {}, dict(n_rows=1 << 32), INVALID, "take rows task 0: a task takes fewer than 2^32 row ids"),
    ("format_major 5", {}, dict(format_major=5), CORRUPTION, "take rows task 0: the file's format version definitely cannot be decompressed"),
]
# the good neighbours of the checks above: each passes every check
GOOD_EDGES = [dict(), dict(page_n=1 << 24), dict(page_n=1), dict(row_base=(1 << 64) - 1000 - 1), dict(every_rows=0, cursors=None), dict(every_rows=1024, cursors=None),   # (k == 0: no cursors needed)
              dict(every_rows=1024), dict(n_rows=0, d_rows=None, dst=None), dict(n_rows=0, d_rows=P + 3, dst=P + 3), dict(dst=P + 4, dtype=1), dict(dst=P + 1, dtype=10),
              dict(n_rows=(1 << 32) - 1), dict(format_major=0)]


def call(lib, form="sync", task=None, no_tasks=False, no_results=False, n_tasks=1, second=None, flags=0):
    arr = (G.TakeTask * 2)(G.TakeTask(**dict(GOOD, **(task or {}))), G.TakeTask(**dict(GOOD, **(second or {}))))
    res = (G.TaskResult * 2)()
    for r in res:
        r.n_out, r.consumed, r.status, r.aux = 77, 78, 99, 98
    host, dev = (None if no_results else res, None) if form == "sync" else (None, None if no_results else P)
    code = lib.pco_gfx_take_rows(n_tasks, None if no_tasks else arr, flags, host, dev, None)
    untouched = all((r.n_out, r.consumed, r.status, r.aux) == (77, 78, 99, 98) for r in res)
    return code, lib.pco_gfx_last_status(), (lib.pco_gfx_last_error() or b"").decode(), untouched


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("name,args,kw,status,words", CHECKS, ids=[c[0] for c in CHECKS])
def test_every_host_check_comes_before_a_device_is_asked_for(lib, name, args, kw, status, words, form):
    code, st, msg, untouched = call(lib, form, kw, **args)
    assert (code, st, msg) == (G.PcoDecompressionError, status, words) and untouched
    if kw:   # ... in the second task of two as well
        code, st, msg, untouched = call(lib, form, None, n_tasks=2, second=kw)
        assert (code, st, msg) == (G.PcoDecompressionError, status, words.replace("task 0", "task 1")) and untouched


def test_the_same_calls_made_good_pass_every_check(lib):
    """Without a device a call that passes the checks is refused for the want of one, `results` untouched.  (With one it would run on P.)"""
    if lib.pco_gfx_device_count() >= 1:
        return
    for kw in GOOD_EDGES:
        for flags in (0, G.CURSOR_GENERAL):
            code, st, msg, untouched = call(lib, "sync", kw, flags=flags)
            assert (code, st) == (G.PcoDecompressionError, DEVICE) and "no MI355X/HIP device" in msg and untouched, (kw, msg)


@pytest.mark.parametrize("form", ["sync", "async"])
def test_the_checks_fire_in_the_header_s_order(lib, form):
    order = [c for c in CHECKS if c[0] in ("dtype 0", "page_n 0", "null meta", "row_base wraps", "every_rows 100", "an index without cursors", "null d_rows", "null dst",
                                           "n_rows 2^32", "format_major 5")]
    # (misaligned cursors need cursors, so they come in a chain of their own; every_rows 100 makes the index length 0: the cursor rule is checked behind it)
    for i in range(len(order)):
        kw = {}
        for later in reversed(order[i:]):
            kw.update(later[2])
        if "every_rows" in kw and i > 4:
            del kw["every_rows"]
        code, st, msg, untouched = call(lib, form, kw)
        assert (st, msg) == (order[i][3], order[i][4]) and untouched, (i, msg)
    code, st, msg, _ = call(lib, form, dict(cursors=P + 4, d_rows=None, dst=None, n_rows=1 << 32, format_major=9))
    assert msg == "take rows task 0: misaligned cursors"
    # the call's own checks in front of every task's, in their order
    code, st, msg, _ = call(lib, form, dict(dtype=0), no_tasks=True, no_results=True, flags=2)
    assert msg == "take rows: null task array"
    code, st, msg, _ = call(lib, form, dict(dtype=0), no_results=True, flags=2)
    assert msg == "take rows: results and d_results are both null"
    code, st, msg, _ = call(lib, form, dict(dtype=0), flags=2)
    assert msg == "take rows: unknown flags"
    # a bad first task is reported although the second is bad as well
    code, st, msg, _ = call(lib, form, dict(n_rows=1 << 32), n_tasks=2, second=dict(meta=None))
    assert msg == "take rows task 0: a task takes fewer than 2^32 row ids"


def test_more_than_2_31_segments_in_one_call_are_refused(lib):
    """2^24 rows cut every 256 are 65536 segments: 32768 such tasks are 2^31 segments and pass this check (the last one is then refused for its format
    version, which comes behind it), one more task is refused at the task that crosses."""
    n = 32769
    big = dict(GOOD, page_n=1 << 24, every_rows=256, n_rows=0, d_rows=None, dst=None)
    arr = (G.TakeTask * n)(*([G.TakeTask(**big)] * n))
    res = (G.TaskResult * 1)(); res[0].status = 99
    arr[n - 2].format_major = 5
    assert lib.pco_gfx_take_rows(n - 1, arr, 0, res, None, None) == G.PcoDecompressionError
    assert (lib.pco_gfx_last_status(), lib.pco_gfx_last_error().decode()) == (CORRUPTION, "take rows task 32767: the file's format version definitely cannot be decompressed")
    arr[n - 2].format_major = 4
    assert lib.pco_gfx_take_rows(n, arr, 0, res, None, None) == G.PcoDecompressionError
    assert (lib.pco_gfx_last_status(), lib.pco_gfx_last_error().decode()) == (INVALID, "take rows task 32768: more than 2^31 segments in one call; split the call")
    arr[n - 1].format_major = 5   # (the segment count comes in front of the format version)
    assert lib.pco_gfx_take_rows(n, arr, 0, res, None, None) == G.PcoDecompressionError and "2^31 segments" in lib.pco_gfx_last_error().decode()
    assert res[0].status == 99


def test_no_tasks_is_a_success_without_a_device(lib):
    res = (G.TaskResult * 1)(); res[0].status = 99
    assert lib.pco_gfx_take_rows(0, None, 0, res, None, None) == G.PcoSuccess
    assert lib.pco_gfx_take_rows(0, None, 0, None, None, None) == G.PcoSuccess
    assert lib.pco_gfx_take_rows(0, None, 2, None, None, None) == G.PcoDecompressionError and lib.pco_gfx_last_error().decode() == "take rows: unknown flags"
    assert res[0].status == 99


# ---------------------------------------------------------------------------------------------------------------------------------------
# the plan's arithmetic: pco_take.h alone, in a stand-alone program under the sanitizers, against the model
# ---------------------------------------------------------------------------------------------------------------------------------------
PROGRAM = r'''
#include "%s/pco_take.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace pcogfx;
// stdin: one case a line, "page_n every_rows row_base n id ...".  stdout: "n_seg n_out aux consumed first count ..." per case.
int main() {
  unsigned long long page_n, every_rows, row_base, n;
  while (std::scanf("%%llu %%llu %%llu %%llu", &page_n, &every_rows, &row_base, &n) == 4) {
    const uint32_t n_seg = take_segments(page_n, every_rows);
    std::vector<uint32_t> marks(n_seg, 0);
    unsigned long long n_out = 0, aux = 0, consumed = 0;
    for (unsigned long long j = 0; j < n; j++) {
      unsigned long long id;
      if (std::scanf("%%llu", &id) != 1) return 2;
      const uint32_t local = take_local_row(id, row_base, page_n);
      if (local == kTakeNotMine) continue;
      n_out++;
      uint32_t& m = marks.at(take_segment_of(local, every_rows));   // (a segment beyond n_seg throws)
      if (take_mark_of(local) > m) m = take_mark_of(local);
    }
    std::printf("%%u", n_seg);
    std::vector<unsigned long long> tasks;
    for (uint32_t s = 0; s < n_seg; s++) {
      const uint64_t count = take_count(s, every_rows, marks[s]);
      if (count > take_segment_rows(s, page_n, every_rows)) return 3;   // the host sizes everything by the whole segment
      tasks.push_back(take_first(s, every_rows)); tasks.push_back(count);
      if (marks[s]) { aux++; consumed += take_batches(count); }
    }
    std::printf(" %%llu %%llu %%llu", n_out, aux, consumed);
    for (unsigned long long v : tasks) std::printf(" %%llu", v);
    std::printf("\n");
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("take")
    src = d / "plan.cpp"
    src.write_text(PROGRAM % CSRC)
    exe = d / "plan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    return str(exe)


def run_program(exe, cases):
    text = "".join("%d %d %d %d %s\n" % (page_n, every_rows, row_base, len(ids), " ".join(str(i) for i in ids)) for page_n, every_rows, row_base, ids in cases)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return [[int(x) for x in line.split()] for line in out.stdout.decode().splitlines()]


def as_row(p):
    return [p.n_seg, p.n_out, p.aux, p.consumed] + [v for t in p.tasks for v in t]


def test_the_header_includes_no_device_header():
    text = open(os.path.join(CSRC, "pco_take.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["stdint.h"]


def test_the_header_plans_what_the_model_plans_under_the_sanitizers(plan_program):
    cases = list(M.cases())
    assert len(cases) == len(M.PAGE_NS) * len(M.EVERY_ROWS) * len(M.ROW_BASES) * 10
    got = run_program(plan_program, [(c[0], c[1], c[2], c[4]) for c in cases])
    assert len(got) == len(cases)
    for c, row in zip(cases, got):
        assert row == as_row(M.plan(c[0], c[1], c[2], c[4])), c[:4]


def test_the_header_at_the_format_s_limits(plan_program):
    top = (1 << 24) - 1
    rb = (1 << 64) - (1 << 24) - 1
    cases = [(1 << 24, 256, rb, [(1 << 64) - 2, (1 << 64) - 1, rb, rb - 1]),                                              # row_base + page_n == 2^64 - 1, the largest the entry point takes
             (1 << 24, 0, 0, [top, 1 << 24, 1 << 32, (1 << 32) + top]),                                                   # an id that is a row only when cut to 32 bits
             (1 << 24, 1 << 24, 7, [7, 7 + top]), (1, 256, 0, [0, 1])]
    got = run_program(plan_program, cases)
    for c, row in zip(cases, got):
        assert row == as_row(M.plan(*c)), c[:3]
    assert got[0][:4] == [65536, 2, 2, 2] and got[1][:4] == [1, 1, 1, 65536] and got[2] == [1, 2, 1, 65536, 0, 1 << 24] and got[3] == [1, 1, 1, 1, 0, 1]


def test_the_model_written_out_once():
    p = M.plan(1000, 256, 5, [5, 260, 261, 1004, 1005, 4, 772, 772])
    assert (p.n_seg, p.marks, p.tasks) == (4, [256, 257, 768, 1000], [(0, 256), (256, 1), (512, 256), (768, 232)])
    assert (p.n_out, p.aux, p.consumed, p.local) == (6, 4, 4, [0, 255, 256, 999, None, None, 767, 767])
    p = M.plan(1000, 0, 0, [300])
    assert (p.n_seg, p.tasks, p.n_out, p.aux, p.consumed) == (1, [(0, 301)], 1, 1, 2)
    assert M.plan(70000, 512, 0, [40000]).aux == 1 and M.plan(70000, 512, 0, []).tasks == [(s * 512, 0) for s in range(137)]


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_the_cases_reveal_every_mutant(mutant):
    """Each one-place change of the arithmetic changes the plan of some case -- in the segments walked, a read task, or the result -- so a kernel with that
    change cannot pass the GPU tests, which hold the device to the model on these cases."""
    revealed = [c[:4] for c in M.cases() if M.plan(c[0], c[1], c[2], c[4], mutant) != M.plan(c[0], c[1], c[2], c[4])]
    assert len(revealed) >= 5, (mutant, M.MUTANT_TEXT[mutant], revealed)
    kinds = {name for _, _, _, name in revealed}
    want = {"boundary": "boundaries", "no_plus_one": "row0", "batch_floor": "row0", "row_base_ignored": "row0"}[mutant]
    assert want in kinds, (mutant, sorted(kinds))
