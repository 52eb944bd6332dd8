"""pco_gfx_decompress_page_reads (include/pco_gfx.h section 4f) without a device: the two structs of the ctypes binding against the header,
the argument checks (made before anything is launched, and before a device is asked for), the cursor verdict of pcodec_amd/csrc/pco_cursor.h
compiled on its own with g++ (the same lines the resume walker runs per task) against a plain Python restatement, and the tANS model stepped
batch by batch: the expected cursor fields of tests/test_gpu_page_reads.py."""
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
from pcodec_amd import _lib as G  # noqa: E402

HEADER = os.path.join(HERE, "..", "include", "pco_gfx.h")
CSRC = os.path.abspath(os.path.join(HERE, "..", "pcodec_amd", "csrc"))
ALL_ONES = (1 << 64) - 1
VERSION, FULL, POSITION = 1, 1, 2
STATE_WORD, MOMENT_WORD = 4, 10


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cursor's documented layout, restated: used here and by the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def pack_cursor(kind, row, bit=0, page_n=0, dtype=0, states=None, moments=None, version=VERSION):
    """The 32 words of a cursor as the header lays them out."""
    w = [0] * 32
    w[0] = version | (kind << 32); w[1] = row; w[2] = bit; w[3] = (page_n & 0xFFFFFFFF) | (dtype << 32)
    for v in range(3):
        for j in range(4):
            w[STATE_WORD + 2 * v + j // 2] |= (states[v][j] if states else 0) << (32 * (j % 2))
    for v in range(2):
        for i in range(8):
            w[MOMENT_WORD + 8 * v + i] = (moments[v][i] if moments else 0) & ALL_ONES
    return w


def unpack_cursor(w):
    w = [int(x) for x in w]
    return dict(version=w[0] & 0xFFFFFFFF, kind=w[0] >> 32, row=w[1], bit=w[2], page_n=w[3] & 0xFFFFFFFF, dtype=w[3] >> 32,
                states=[[(w[STATE_WORD + 2 * v + j // 2] >> (32 * (j % 2))) & 0xFFFFFFFF for j in range(4)] for v in range(3)],
                moments=[[w[MOMENT_WORD + 8 * v + i] for i in range(8)] for v in range(2)], tail=w[26:])


def restated_verdict(w, want_kind, page_n, dtype, first, body_first_bit, page_bits, asl):
    """include/pco_gfx.h section 4f's list of refusals"""
    c = unpack_cursor(w)
    if c["version"] != VERSION or c["kind"] != want_kind:
        return G.ST_INVALID_ARGUMENT
    if c["page_n"] != page_n or c["dtype"] != dtype:
        return G.ST_INVALID_ARGUMENT
    if c["row"] > first or (c["row"] % 256 != 0 and c["row"] != page_n):
        return G.ST_INVALID_ARGUMENT
    if want_kind == POSITION:
        return G.ST_OK
    if c["bit"] < body_first_bit or c["bit"] > page_bits:
        return G.ST_INVALID_ARGUMENT
    if any(c["states"][v][j] >= 1 << asl[v] for v in range(3) for j in range(4)):
        return G.ST_INVALID_ARGUMENT
    return G.ST_OK


def model_cursors(meta, page, n, latent_bits):
    """tests/tans_model.py stepped batch by batch over a one-variable Classic page without delta: (the body's first bit, [(row, bit position in
    the page, the four state indices)] at every batch boundary and at the page's end, the latents)."""
    r = TM.Bits(meta)
    assert r.read(4) == 0 and r.read(4) == 0, "Classic mode without delta only"
    size_log = r.read(4); n_bins = r.read(15)
    assert n_bins >= 1
    ob_bits = {8: 4, 16: 5, 32: 6, 64: 7}[latent_bits]
    bins = [(r.read(size_log) + 1, r.read(latent_bits), r.read(ob_bits)) for _ in range(n_bins)]
    r.align()
    assert r.pos == r.n
    nodes = TM.decoder_nodes(size_log, [b[0] for b in bins])
    b = TM.Bits(page)
    state = [b.read(size_log) for _ in range(TM.INTERLEAVING)]
    b.align()
    body = b.pos
    mask = (1 << latent_bits) - 1
    marks = []; out = []
    for start in range(0, n, TM.BATCH_N):
        bn = min(TM.BATCH_N, n - start)
        syms = []
        for i in range(bn):
            if n_bins == 1:
                syms.append(0); continue
            j = i % TM.INTERLEAVING
            s, bits, base = nodes[state[j]]
            syms.append(s); state[j] = base + b.read(bits)
        for s in syms:
            out.append((bins[s][1] + b.read(bins[s][2])) & mask)
        marks.append((start + bn, b.pos, tuple(state)))
    b.align()
    assert b.pos == b.n
    return body, marks, out, size_log


# ---------------------------------------------------------------------------------------------------------------------------------------
# the structs and the export
# ---------------------------------------------------------------------------------------------------------------------------------------
C_TYPES = {"const void*": C.c_void_p, "void*": C.c_void_p, "const PcoGfxPageCursor*": C.c_void_p, "PcoGfxPageCursor*": C.c_void_p, "uint64_t": C.c_uint64,
           "uint32_t": C.c_uint32}


def header_fields(struct):
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const void\*|void\*|const PcoGfxPageCursor\*|PcoGfxPageCursor\*|uint64_t|uint32_t)\s+(.*)", decl)
        assert m, decl
        for name in m.group(2).split(","):
            out.append((name.strip(), C_TYPES[m.group(1)]))
    return out


def test_the_binding_lays_the_read_task_out_as_the_header_does():
    want = header_fields("PcoGfxPageReadTask")
    assert [n for n, _ in want] == ["meta", "meta_len", "page", "page_len", "dst", "page_n", "first", "count", "dtype", "format_major", "from", "to"]
    assert [("from" if n == "from_" else n, t) for n, t in G.PageReadTask._fields_] == want   # (`from` is a Python keyword: the binding says from_)
    assert C.sizeof(G.PageReadTask) == 88
    at = 0
    for n, t in G.PageReadTask._fields_:
        assert getattr(G.PageReadTask, n).offset == at, n
        at += C.sizeof(t)
    assert at == 88
    # PcoGfxPageRangeTask's fields in its order come first
    assert G.PageReadTask._fields_[:10] == G.PageRangeTask._fields_
    assert [(n, getattr(G.PageReadTask, n).offset) for n, _ in G.PageRangeTask._fields_] == [(n, getattr(G.PageRangeTask, n).offset) for n, _ in G.PageRangeTask._fields_]


def test_the_cursor_is_256_bytes_of_words():
    text = open(HEADER).read()
    assert re.search(r"typedef struct PcoGfxPageCursor \{ uint64_t w\[32\]; \} PcoGfxPageCursor;", text)
    assert C.sizeof(G.PageCursor) == 256 == G.CURSOR_BYTES and G.PageCursor.w.offset == 0
    assert (G.CURSOR_VERSION, G.CURSOR_FULL, G.CURSOR_POSITION) == (VERSION, FULL, POSITION)
    cur = open(os.path.join(CSRC, "pco_cursor.h")).read()
    assert re.search(r"kCursorVersion = 1;", cur) and re.search(r"kCursorFull = 1, kCursorPosition = 2;", cur)
    assert re.search(r"kCursorWords = 32, kCursorStateWord = 4, kCursorMomentWord = 10;", cur)


def test_the_header_declares_the_entry_point_and_the_library_exports_it():
    text = open(HEADER).read()
    assert re.search(r"enum PcoError pco_gfx_decompress_page_reads\(size_t n_tasks, const PcoGfxPageReadTask\* tasks, PcoGfxTaskResult\* results,", text)
    assert hasattr(G.lib(), "pco_gfx_decompress_page_reads")


# ---------------------------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
GOOD_TASK = dict(meta=P, meta_len=10, page=P, page_len=10, dst=P, page_n=10, first=0, count=1, dtype=1, format_major=4, from_=P, to=P)


def call(task=None, no_tasks=False, no_results=False):
    L = G.lib()
    kw = dict(GOOD_TASK); kw.update(task or {})
    arr = (G.PageReadTask * 1)(G.PageReadTask(**kw))
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    code = L.pco_gfx_decompress_page_reads(1, None if no_tasks else arr, None if no_results else res, None, None)
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
    (dict(task=dict(dst=None)), G.ST_INVALID_ARGUMENT),                               # with count > 0
    (dict(task=dict(first=5, count=6)), G.ST_INVALID_ARGUMENT),                       # first + count > page_n
    (dict(task=dict(first=10, count=1)), G.ST_INVALID_ARGUMENT),                      # a finished page asked for more
    (dict(task=dict(first=11, count=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(first=ALL_ONES, count=2)), G.ST_INVALID_ARGUMENT),                # the sum wraps
    (dict(task=dict(page_n=0, first=0, count=0)), G.ST_INVALID_ARGUMENT),
    (dict(task=dict(format_major=5)), G.ST_CORRUPTION),
]


@pytest.mark.parametrize("kw,status", CHECKS)
def test_argument_checks_come_before_anything_else(kw, status):
    code, st, res = call(**kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)   # nothing was written


def test_no_tasks_is_a_success_without_a_device():
    res = (G.TaskResult * 1)()
    assert G.lib().pco_gfx_decompress_page_reads(0, None, res, None, None) == G.PcoSuccess


# ---------------------------------------------------------------------------------------------------------------------------------------
# the verdict function, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cursor_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("cursorverdict")
    src = d / "verdict.cpp"
    src.write_text(f'''
#include "{CSRC}/pco_cursor.h"
extern "C" uint32_t verdict(const uint64_t* w, uint32_t want_kind, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits, const uint32_t* asl) {{
  return pcogfx::cursor_verdict(w, want_kind, page_n, dtype, first, body_first_bit, page_bits, asl);
}}
extern "C" void words(uint32_t kind, uint64_t row, uint64_t bit, uint64_t page_n, uint32_t dtype, const uint32_t* states, const uint64_t* moments, uint64_t* out) {{
  for (uint32_t i = 0; i < pcogfx::kCursorWords; i++) out[i] = pcogfx::cursor_word(i, kind, row, bit, page_n, dtype, states, moments);
}}
''')
    out = d / "libcursor.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.verdict.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.verdict.restype = C.c_uint32
    lib.words.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.words.restype = None
    return lib


def run_verdict(lib, w, want_kind, page_n, dtype, first, body_first_bit, page_bits, asl):
    a = (C.c_uint64 * 32)(*w); s = (C.c_uint32 * 3)(*asl)
    return lib.verdict(a, want_kind, page_n, dtype, first, body_first_bit, page_bits, s)


ASL = [0, 10, 2]
STATES = [[0, 0, 0, 0], [5, 6, 7, 1023], [1, 2, 3, 3]]
SCENE = dict(want_kind=FULL, page_n=3000, dtype=1, first=600, body_first_bit=40, page_bits=8000)


def good(**kw):
    d = dict(kind=FULL, row=512, bit=1000, page_n=3000, dtype=1, states=[list(s) for s in STATES], moments=[[7] * 8, [9] * 8])
    d.update(kw)
    return pack_cursor(**d)


def with_state(v, j, x):
    s = [list(r) for r in STATES]; s[v][j] = x
    return good(states=s)


# (name, cursor words, what differs from SCENE, the status expected -- written down here, not taken from either implementation)
ROWS = [
    ("a cursor that passes", good(), {}, G.ST_OK),
    ("a wrong version", good(version=2), {}, G.ST_INVALID_ARGUMENT),
    ("version 0", good(version=0), {}, G.ST_INVALID_ARGUMENT),
    ("position only where full state is wanted", good(kind=POSITION), {}, G.ST_INVALID_ARGUMENT),
    ("kind 0", good(kind=0), {}, G.ST_INVALID_ARGUMENT),
    ("kind 3", good(kind=3), {}, G.ST_INVALID_ARGUMENT),
    ("another page_n", good(page_n=2999), {}, G.ST_INVALID_ARGUMENT),
    ("another dtype", good(dtype=3), {}, G.ST_INVALID_ARGUMENT),
    ("at > first", good(row=768), {}, G.ST_INVALID_ARGUMENT),
    ("at == first", good(), dict(first=512), G.ST_OK),
    ("first one row in front of at", good(), dict(first=511), G.ST_INVALID_ARGUMENT),
    ("at neither a multiple of 256 nor page_n", good(row=300), {}, G.ST_INVALID_ARGUMENT),
    ("at == page_n", good(row=3000), dict(first=3000), G.ST_OK),
    ("at == page_n but first in front of it", good(row=3000), dict(first=2999), G.ST_INVALID_ARGUMENT),
    ("the body's first bit", good(bit=40), {}, G.ST_OK),
    ("one bit in front of the body", good(bit=39), {}, G.ST_INVALID_ARGUMENT),
    ("the page's last bit position", good(bit=8000), {}, G.ST_OK),
    ("one bit beyond the page", good(bit=8001), {}, G.ST_INVALID_ARGUMENT),
    ("a bit position of all ones", good(bit=ALL_ONES), {}, G.ST_INVALID_ARGUMENT),
    ("the primary's state 2^asl - 1", with_state(1, 0, 1023), {}, G.ST_OK),
    ("the primary's state 2^asl", with_state(1, 0, 1024), {}, G.ST_INVALID_ARGUMENT),
    ("the secondary's state 2^asl - 1", with_state(2, 3, 3), {}, G.ST_OK),
    ("the secondary's state 2^asl", with_state(2, 3, 4), {}, G.ST_INVALID_ARGUMENT),
    ("a state of all ones", with_state(1, 2, 0xFFFFFFFF), {}, G.ST_INVALID_ARGUMENT),
    ("a state for a variable the page does not have", with_state(0, 1, 1), {}, G.ST_INVALID_ARGUMENT),
    ("position only, wanted", pack_cursor(POSITION, 512, 0, 3000, 1), dict(want_kind=POSITION), G.ST_OK),
    ("full state where position only is wanted", good(), dict(want_kind=POSITION), G.ST_INVALID_ARGUMENT),
    ("position only, at > first", pack_cursor(POSITION, 768, 0, 3000, 1), dict(want_kind=POSITION), G.ST_INVALID_ARGUMENT),
    ("position only, unaligned", pack_cursor(POSITION, 100, 0, 3000, 1), dict(want_kind=POSITION), G.ST_INVALID_ARGUMENT),
    ("position only, at == page_n", pack_cursor(POSITION, 3000, 0, 3000, 1), dict(want_kind=POSITION, first=3000), G.ST_OK),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_the_verdict_function_against_its_restatement(cursor_lib, row):
    _, w, diff, status = row
    scene = dict(SCENE); scene.update(diff)
    assert restated_verdict(w, asl=ASL, **scene) == status
    assert run_verdict(cursor_lib, w, asl=ASL, **scene) == status


def test_the_verdict_function_over_a_small_grid(cursor_lib):
    """version x kind x wanted kind x row x first x the cursor's page_n x bit position x one state: 3 * 4 * 2 * 5 * 4 * 2 * 4 * 3 cursors"""
    n = 0
    for version in (0, 1, 2):
        for kind in (0, 1, 2, 3):
            for want in (FULL, POSITION):
                for row in (0, 256, 300, 512, 3000):
                    for first in (0, 256, 511, 3000):
                        for page_n in (3000, 2999):
                            for bit in (39, 40, 8000, 8001):
                                for st in (0, 3, 4):
                                    s = [list(r) for r in STATES]; s[2][1] = st
                                    w = pack_cursor(kind, row, bit, page_n, 1, s, None, version)
                                    args = dict(want_kind=want, page_n=3000, dtype=1, first=first, body_first_bit=40, page_bits=8000, asl=ASL)
                                    assert run_verdict(cursor_lib, w, **args) == restated_verdict(w, **args), (version, kind, want, row, first, page_n, bit, st)
                                    n += 1
    assert n == 11520


def test_the_header_s_word_function_is_the_documented_layout(cursor_lib):
    st = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]; mom = [(1 << 63) + i * 977 for i in range(16)]
    out = (C.c_uint64 * 32)()
    cursor_lib.words(FULL, 768, 12345, 3000, 6, (C.c_uint32 * 12)(*st), (C.c_uint64 * 16)(*mom), out)
    want = pack_cursor(FULL, 768, 12345, 3000, 6, [st[0:4], st[4:8], st[8:12]], [mom[:8], mom[8:]])
    assert list(out) == want and list(out)[26:] == [0] * 6
    assert unpack_cursor(out)["states"] == [st[0:4], st[4:8], st[8:12]] and unpack_cursor(out)["moments"] == [mom[:8], mom[8:]]
    cursor_lib.words(POSITION, 768, 12345, 3000, 6, None, None, out)
    assert list(out) == pack_cursor(POSITION, 768, 0, 3000, 6) and sum(1 for x in out if x) == 3


# ---------------------------------------------------------------------------------------------------------------------------------------
# the tANS model, batch by batch
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n", [(np.uint32, 3000), (np.uint16, 2816), (np.int64, 700), (np.uint8, 256)])
def test_the_stepped_model_decodes_an_oracle_page(dt, n):
    rng = np.random.default_rng(n)
    x = (rng.integers(0, 50, n) * 3 + rng.integers(0, 2, n) * 90).astype(dt)
    meta, pages, page_ns = O.wrapped_compress(x, O.make_config(mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP, max_page_n=1 << 20))
    assert page_ns == [n]
    bits = np.dtype(dt).itemsize * 8
    body, marks, latents, size_log = model_cursors(meta, pages[0], n, bits)
    assert [int(v) for v in TM.to_latent(x)] == latents
    assert [m[0] for m in marks] == [min(r + 256, n) for r in range(0, n, 256)]
    assert body == -(-4 * size_log // 8) * 8 and all(a[1] <= b[1] for a, b in zip(marks, marks[1:])) and marks[-1][1] <= 8 * len(pages[0])
    assert all(0 <= s < 1 << size_log for m in marks for s in m[2])
