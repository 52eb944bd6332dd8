"""CPU: standalone chunks from a device directory (include/pco_gfx.h section 4l) without a device.

pcodec_amd/csrc/pco_chunk_dir.h compiled alone with g++ -- the lines the resolve kernels run per task -- against an INDEPENDENT split of the same
chunks: the ChunkMeta and the one page the oracle's wrapped writer produces for the same numbers and config (pco_oracle_wrapped_compress against
pco_oracle_simple_compress; the test-only generator's wrapped form against its standalone form for Dict and Conv1), and for the reference's golden
.pco assets, which reach back to format version 1, the end of the ChunkMeta as the oracle's own reader finds it.  Then chunk_verdict over hand-built
directories that hit every row of the header's table in its order, with gaps of 0 and 4 and a chunk cut after every byte; the same through
pco_gfx_standalone_chunk_split; every host check of the three entry points in both forms; and the task lists pcodec_amd.paged builds from _DirChunks.
The sanitised run is a stand-alone program with its own main."""
import ctypes as C
import glob
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
import paged_plan_util as U  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import build as B  # noqa: E402

CSRC = os.path.abspath(os.path.join(HERE, "..", "pcodec_amd", "csrc"))
HEADER = os.path.join(HERE, "..", "include", "pco_gfx.h")
ASSETS = os.path.join(HERE, "golden", "ref_assets")
ALL_ONES = (1 << 64) - 1
OK, CORRUPTION, INSUFFICIENT, INVALID = G.ST_OK, G.ST_CORRUPTION, G.ST_INSUFFICIENT_DATA, G.ST_INVALID_ARGUMENT

PROBE = r'''
#include "%s/pco_chunk_dir.h"
using namespace pcogfx;
extern "C" void extent(const uint8_t* p, uint64_t len, uint32_t dtype, uint32_t format_major, uint64_t* out) {
  uint64_t meta_len = 77; uint32_t status = 77;
  out[2] = chunk_meta_extent(p, len, dtype, format_major, &meta_len, &status);
  out[0] = meta_len; out[1] = status;
}
// out: meta - blob, meta_len, page - blob, page_len, status
extern "C" void verdict(const uint8_t* blob, uint64_t blob_len, uint32_t gap, uint64_t end, uint64_t c0, uint64_t c1, uint32_t dtype, uint64_t page_n, uint32_t format_major, uint64_t* out) {
  const DirVerdict v = chunk_verdict(blob, blob_len, gap, end, c0, c1, dtype, page_n, format_major);
  out[0] = (uint64_t)(v.meta - blob); out[1] = v.meta_len; out[2] = (uint64_t)(v.page - blob); out[3] = v.page_len; out[4] = v.status;
}
''' % CSRC


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunkdir")
    src = d / "probe.cpp"; src.write_text(PROBE)
    out = d / "libprobe.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-o", str(out), str(src)])
    lib = C.CDLL(str(out))
    lib.extent.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]; lib.extent.restype = None
    lib.verdict.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]; lib.verdict.restype = None

    class P:
        @staticmethod
        def extent(data, dtype, fm=4):
            """(meta_len, status) of the ChunkMeta at data[0:]; the buffer handed over holds exactly len(data) bytes"""
            buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0"); o = (C.c_uint64 * 3)()
            lib.extent(buf, len(data), dtype, fm, o)
            assert o[2] == o[0]
            return int(o[0]), int(o[1])

        @staticmethod
        def verdict(blob, gap, end, c0, c1, dtype, page_n, fm=4, blob_len=None):
            buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0"); o = (C.c_uint64 * 5)()
            lib.verdict(buf, len(blob) if blob_len is None else blob_len, gap, end, c0, c1, dtype, page_n, fm, o)
            return tuple(int(x) for x in o)
    return P


# ---------------------------------------------------------------------------------------------------------------------------------------
# the chunks, each with its independent split: (name, chunk bytes, dtype byte, format major, the ChunkMeta's bytes or None, its length, n)
# ---------------------------------------------------------------------------------------------------------------------------------------
def file_header(f):
    """(bytes in front of the first chunk, the wrapped format's major version) of a standalone file, by the format's arithmetic
    (standalone/decompressor.rs:85-137): the magic, from standalone version 2 on the version byte, from 3 on the uniform type byte, the varint n_hint,
    then the wrapped header -- the major version and, from 4 on, the minor one."""
    assert f[:4] == b"pco!"
    at = 4; sv = f[4]
    if sv >= 2:
        at = 5 + (1 if sv >= 3 else 0)
        power = 1 + (f[at] & 63)
        at += (6 + power + 7) // 8
    major = f[at]
    return at + (2 if major >= 4 else 1), major


def numbers(name, n, kind, seed=1):
    rng = np.random.default_rng(seed); dt = np.dtype(name)
    if kind == "constant":
        return np.full(n, 7, dt)
    if kind == "mult":      # multiples of 7 (integers) / of 0.25 (floats)
        base = rng.integers(0, 100, n)
        return (base * 7).astype(dt) if dt.kind != "f" else (base * 0.25).astype(dt)
    if kind == "smooth":
        return (np.cumsum(rng.integers(-3, 4, n)) + 1000).astype(dt)
    if kind == "periodic":
        return (rng.integers(0, 1 << 20, 37)[np.arange(n) % 37] + rng.integers(0, 3, n)).astype(dt)
    if kind == "few":       # a handful of distinct values
        return rng.integers(0, 1 << 14, 5).astype(dt)[rng.integers(0, 5, n)]
    if kind == "two":
        return np.where(rng.integers(0, 2, n) == 1, 5, 900).astype(dt)
    if dt.kind == "f":
        return (rng.standard_normal(n) * 100).astype(dt)
    return rng.integers(0, min(1 << (8 * dt.itemsize - 1), 1 << 40), n).astype(dt)


def oracle_case(name, arr, **cfg):
    ocfg = O.make_config(max_page_n=1 << 20, **cfg)
    f = O.simple_compress(arr, ocfg)
    meta, pages, ns = O.wrapped_compress(arr, ocfg)
    assert ns == [arr.size] and len(pages) == 1
    hdr, major = file_header(f)
    assert major == 4 and f[-1] == 0
    return (name, f[hdr:-1], O.dtype_byte(arr), 4, meta, len(meta), arr.size, pages[0])


def generator_case(name, arr, **kw):
    f = O.test_encode(arr, **kw)
    meta, pages = O.test_encode(arr, pages=[arr.size], **kw)
    hdr, major = file_header(f)
    return (name, f[hdr:-1], O.dtype_byte(arr), major, meta, len(meta), arr.size, pages[0])


def asset_case(name, path):
    f = open(path, "rb").read()
    hdr, major = file_header(f)
    info, _ = O.inspect_first_chunk(f)
    assert info.fmt_major == major and info.dtype == f[hdr]
    return (name, f[hdr:], int(info.dtype), major, None, int(info.meta_end_byte) - hdr - 4, int(info.n), None)


# The corpus: its NAMES are known when the module is collected (the arrays are plain numpy, the assets are files of the repository), so every test
# below is parametrised over them and no row is empty; a chunk is built from the oracle on first use and kept.
BUILDERS = {}


def add(fn, name, *args, **kw):
    assert name not in BUILDERS
    BUILDERS[name] = lambda: fn(name, *args, **kw)


def declare():
    for t in G.NUMBER_TYPES:   # every number type, f16 included
        add(oracle_case, f"classic {t.name}", numbers(t.name, 300, "random", t.byte), mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP)
    add(oracle_case, "int mult i32", numbers("int32", 600, "mult"), mode=O.MODE_TRY_INT_MULT, mode_u64=7, delta=O.DELTA_NOOP)
    add(oracle_case, "int mult u64 + consecutive 1", numbers("uint64", 600, "mult"), mode=O.MODE_TRY_INT_MULT, mode_u64=7, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=1)
    add(oracle_case, "float mult f32", numbers("float32", 600, "mult"), mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.DELTA_NOOP)
    add(oracle_case, "float mult f64 + lookback", numbers("float64", 600, "mult"), mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.DELTA_TRY_LOOKBACK)
    add(oracle_case, "float quant f32", numbers("float32", 600, "random").astype(np.float16).astype(np.float32), mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=13, delta=O.DELTA_NOOP)
    add(oracle_case, "float quant f16", (numbers("float16", 600, "random").view(np.uint16) & 0xFFF0).view(np.float16), mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=4, delta=O.DELTA_NOOP)
    add(oracle_case, "consecutive 1 i64", numbers("int64", 1000, "smooth"), mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=1)
    add(oracle_case, "consecutive 7 i16", numbers("int16", 1000, "smooth"), mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=7)
    add(oracle_case, "lookback i64", numbers("int64", 1000, "periodic"), mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_LOOKBACK)
    add(oracle_case, "lookback u8", numbers("uint8", 1000, "periodic"), mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_LOOKBACK)
    add(oracle_case, "constant u32: 1 bin, a page of 0 bytes", numbers("uint32", 500, "constant"), mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP)
    add(oracle_case, "two values u16: 2 bins", numbers("uint16", 500, "two"), mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP)
    add(oracle_case, "one number f64", numbers("float64", 1, "random"), mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP)
    add(oracle_case, "level 12 u32: >= 256 bins", numbers("uint32", 1 << 13, "random"), level=12, mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP)
    add(oracle_case, "2 numbers under consecutive 2: 0 bins", np.array([5, 9], np.int32), mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=2)
    for name in ("uint32", "int16", "float64", "uint8"):
        add(generator_case, f"dict {name}", numbers(name, 700, "few"), mode=O.MODE_TRY_DICT)
    add(generator_case, "dict u64 + consecutive 1", numbers("uint64", 700, "few"), mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_CONSECUTIVE, order=1)
    add(generator_case, "dict u32 + lookback", numbers("uint32", 700, "few"), mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1, lookback_seed=5)
    add(generator_case, "conv1 i32, 2 weights", numbers("int32", 700, "smooth"), mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=4, bias=5, weights=[-16, 32])
    add(generator_case, "conv1 u16, 1 weight", numbers("uint16", 700, "smooth"), mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=0, bias=0, weights=[1])
    add(generator_case, "conv1 f32 + float mult, 5 weights", numbers("float32", 700, "mult"), mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_CONV1, quantization=3, bias=-2,
                            weights=[1, -2, 3, -4, 8])
    add(generator_case, "dict + conv1 u32", numbers("uint32", 700, "few"), mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_CONV1, quantization=2, bias=1, weights=[2, 2])
    add(generator_case, "a table of 300 bins", numbers("uint32", 4000, "random"), tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_n_bins=300, tbl_seed=3)
    add(generator_case, "delta'd secondary under lookback", numbers("int32", 900, "mult"), mode=O.MODE_TRY_INT_MULT, mode_u64=7, delta=O.TE_DELTA_LOOKBACK, window_n_log=10, state_n_log=0,
                            secondary_uses_delta=True, lookback_seed=5)
    for path in sorted(glob.glob(os.path.join(ASSETS, "*.pco"))):
        f = open(path, "rb").read()
        if f[file_header(f)[0]] != 0:   # (else a file without a chunk: the terminator alone)
            add(asset_case, "asset " + os.path.basename(path), path)


declare()
CASE_NAMES = list(BUILDERS)
assert len(CASE_NAMES) == 50
_built = {}


def case(name):
    if name not in _built:
        _built[name] = BUILDERS[name]()
    return _built[name]


def cases():
    return [case(name) for name in CASE_NAMES]


def test_the_corpus_covers_what_the_issue_lists():
    cs = cases()
    info = []
    for name, chunk, dt, major, meta, meta_len, n, page in cs:
        m = chunk[4: 4 + meta_len]
        mode = m[0] & 15
        delta = None
        if mode == 0 and major >= 3:
            delta = ((m[0] >> 4) & 15)
        info.append((dt, mode, delta, major, len(chunk) - 4 - meta_len if page is not None else None))
    assert {i[0] for i in info} == set(range(1, 12))
    assert {i[1] for i in info} == {0, 1, 2, 3, 4}
    assert {i[2] for i in info if i[2] is not None} == {0, 1, 2, 3}
    assert {i[3] for i in info} >= {1, 2, 3, 4}
    assert any(i[4] == 0 for i in info), "no chunk with a page of 0 bytes"
    bins = set()
    for name, chunk, dt, major, meta, meta_len, n, page in cs:
        if not name.startswith("asset"):
            ci, _ = O.inspect_first_chunk(G_file(chunk))
            bins |= {int(ci.n_bins[1])}
    assert {0, 1, 2} <= bins and any(b >= 256 for b in bins), bins


def G_file(chunk):
    """a current-version standalone file around one chunk"""
    buf = (C.c_uint8 * 64)()
    k = G.lib().pco_gfx_write_standalone_header(buf, 64, 0, 0)
    return bytes(buf[:k]) + bytes(chunk) + b"\0"


@pytest.mark.parametrize("k", CASE_NAMES)
def test_the_extent_is_the_wrapped_writer_s_chunk_meta(probe, k):
    c = case(k)
    name, chunk, dt, major, meta, meta_len, n, page = c
    assert chunk[0] == dt and 1 + int.from_bytes(chunk[1:4], "little") == n, name
    got, status = probe.extent(chunk[4:], dt, major)
    assert (got, status) == (meta_len, OK), name
    if meta is not None:
        assert chunk[4: 4 + got] == meta and chunk[4 + got:] == page, name
    # header fields only: the same answer with nothing behind the header but zeros in place of the bins' bytes would be a different chunk, so check the
    # weaker, exact property -- a ChunkMeta cut anywhere INSIDE its bins still gives the full length, and the verdict then finds it too long
    if got > 16:
        assert probe.extent(chunk[4: 4 + got - 1], dt, major) == (got, OK), name


def page_len_of(c):
    name, chunk, dt, major, meta, meta_len, n, page = c
    return len(chunk) - 4 - meta_len if page is None else len(page)   # (an asset: the rest of its file follows the first chunk's ChunkMeta)


@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("k", CASE_NAMES)
def test_the_verdict_on_every_chunk_and_every_cut(probe, k, gap):
    c = case(k)
    name, chunk, dt, major, meta, meta_len, n, page = c
    page_len = page_len_of(c)
    blob = b"\xEE" * 5 + b"\xDD" * gap + chunk + b"\xEE" * 7
    c0, c1 = 5, 5 + gap + len(chunk)
    assert probe.verdict(blob, gap, c1, c0, c1, dt, n, major) == (c0 + gap + 4, meta_len, c0 + gap + 4 + meta_len, page_len, OK), (name, gap)
    assert probe.verdict(blob, gap, c1, c0, c1, dt, n + 1, major)[4] == INVALID and probe.verdict(blob, gap, c1, c0, c1, dt, max(n - 1, 2 if n == 1 else 1), major)[4] == INVALID
    wrong = 1 if dt != 1 else 3
    assert probe.verdict(blob, gap, c1, c0, c1, wrong, n, major) == (0, 0, 0, 0, CORRUPTION), (name, gap)
    # the chunk cut after every byte up to its ChunkMeta's end and a little beyond: refused until the whole ChunkMeta is there
    for cut in list(range(0, min(4 + meta_len, 80))) + [4 + meta_len - 1]:
        v = probe.verdict(blob, gap, c1, c0, c0 + gap + cut, dt, n, major)
        assert v == (0, 0, 0, 0, INSUFFICIENT), (name, gap, cut, v)
    v = probe.verdict(blob, gap, c1, c0, c0 + gap + 4 + meta_len, dt, n, major)
    assert v == (c0 + gap + 4, meta_len, c0 + gap + 4 + meta_len, 0, OK)


@pytest.mark.parametrize("k", CASE_NAMES)
def test_the_host_split_on_every_chunk(k):
    """pco_gfx_standalone_chunk_split: the same two functions on host bytes, gap 0, no n to compare"""
    c = case(k)
    name, chunk, dt, major, meta, meta_len, n, page = c
    page_len = page_len_of(c); L = G.lib()
    nn, ml, pl = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77)
    buf = (C.c_uint8 * len(chunk)).from_buffer_copy(chunk)
    assert L.pco_gfx_standalone_chunk_split(buf, len(chunk), dt, major, C.byref(nn), C.byref(ml), C.byref(pl)) == G.PcoSuccess
    assert (nn.value, ml.value, pl.value) == (n, meta_len, page_len), name
    for cut in (0, 3, 4, 4 + meta_len - 1):
        assert L.pco_gfx_standalone_chunk_split(buf, cut, dt, major, C.byref(nn), C.byref(ml), C.byref(pl)) == G.PcoDecompressionError
        assert L.pco_gfx_last_status() == INSUFFICIENT and (nn.value, ml.value, pl.value) == (0, 0, 0)
    assert L.pco_gfx_standalone_chunk_split(buf, len(chunk), 1 if dt != 1 else 3, major, C.byref(nn), C.byref(ml), C.byref(pl)) == G.PcoDecompressionError
    assert L.pco_gfx_last_status() == CORRUPTION


def test_the_host_split_refuses_bad_arguments():
    L = G.lib(); buf = (C.c_uint8 * 16)(1); a = C.c_uint64()
    assert L.pco_gfx_standalone_chunk_split(None, 16, 1, 4, C.byref(a), C.byref(a), C.byref(a)) == G.PcoInvalidType
    assert L.pco_gfx_standalone_chunk_split(buf, 16, 0, 4, C.byref(a), C.byref(a), C.byref(a)) == G.PcoInvalidType
    assert L.pco_gfx_standalone_chunk_split(buf, 16, 12, 4, C.byref(a), C.byref(a), C.byref(a)) == G.PcoInvalidType
    assert L.pco_gfx_standalone_chunk_split(buf, 16, 1, 4, None, C.byref(a), C.byref(a)) == G.PcoInvalidType
    assert L.pco_gfx_standalone_chunk_split(buf, 16, 1, 5, C.byref(a), C.byref(a), C.byref(a)) == G.PcoDecompressionError and L.pco_gfx_last_status() == CORRUPTION


# ---------------------------------------------------------------------------------------------------------------------------------------
# the ChunkMeta's header, field by field, on hand-built bits
# ---------------------------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v |= (value & ((1 << bits) - 1)) << self.n; self.n += bits
        return self

    def pad(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def bytes(self, extra=0):
        return self.v.to_bytes((self.n + 7) // 8 + extra, "little")


def var(b, ans_size_log, n_bins):
    return b.put(ans_size_log, 4).put(n_bins, 15)


def bins_bits(n_bins, ans_size_log, latent_bits):
    return n_bins * (ans_size_log + latent_bits + {8: 4, 16: 5, 32: 6, 64: 7}[latent_bits])


# (name, dtype, format major, the ChunkMeta up to its LAST variable's header as (value, bits) fields -- "pad": the Dict mode's alignment; a variable's bins
#  lie between its header and the next one's, zeros here --, the bits of the last variable's bins)
HAND = [
    ("classic, no delta, u32, 3 bins", 1, 4, [(0, 4), (0, 4), (2, 4), (3, 15)], bins_bits(3, 2, 32)),
    ("classic, no delta, u8, 0 bins", 10, 4, [(0, 4), (0, 4), (0, 4), (0, 15)], 0),
    ("classic, format 2: the order alone", 3, 2, [(0, 4), (5, 3), (1, 4), (2, 15)], bins_bits(2, 1, 32)),
    ("classic, format 1, order 0", 2, 1, [(0, 4), (0, 3), (0, 4), (1, 15)], bins_bits(1, 0, 64)),
    ("int mult i64, consecutive 7", 4, 4, [(1, 4), (7, 64), (1, 4), (7, 3), (1, 1), (3, 4), (8, 15), (0, bins_bits(8, 3, 64)), (1, 4), (2, 15)], bins_bits(2, 1, 64)),
    ("float mult f16, lookback", 9, 4, [(2, 4), (0x3400, 16), (2, 4), (9, 5), (1, 4), (0, 1), (4, 4), (16, 15), (0, bins_bits(16, 4, 32)), (5, 4), (20, 15), (0, bins_bits(20, 5, 16)),
                                        (0, 4), (1, 15)], bins_bits(1, 0, 16)),
    ("float quant f32", 5, 4, [(3, 4), (13, 8), (0, 4), (6, 4), (64, 15), (0, bins_bits(64, 6, 32)), (2, 4), (4, 15)], bins_bits(4, 2, 32)),
    ("dict u16, 5 entries", 7, 4, [(4, 4), (5, 25), "pad", (0, 5 * 16), (0, 4), (3, 4), (5, 15)], bins_bits(5, 3, 32)),
    ("dict f64, 0 entries, lookback", 6, 4, [(4, 4), (0, 25), "pad", (2, 4), (7, 5), (0, 4), (1, 1), (1, 4), (2, 15), (0, bins_bits(2, 1, 32)), (0, 4), (1, 15)], bins_bits(1, 0, 32)),
    ("conv1 i32, 3 weights", 3, 4, [(0, 4), (3, 4), (4, 5), (1 << 63, 64), (2, 5), (0, 96), (14, 4), (32767, 15)], bins_bits(32767, 14, 32)),
    ("conv1 u8, 32 weights", 10, 4, [(0, 4), (3, 4), (0, 5), (0, 64), (31, 5), (0, 32 * 32), (1, 4), (2, 15)], bins_bits(2, 1, 8)),
]


def hand_built(fields):
    b = Bits(); ends = []
    for f in fields:
        if f == "pad":
            b.pad()
        else:
            b.put(*f)
        ends.append(b.n)
    return b, ends


@pytest.mark.parametrize("row", HAND, ids=[r[0] for r in HAND])
def test_the_extent_of_a_hand_built_header_and_of_every_cut_of_it(probe, row):
    name, dt, major, fields, bins = row
    b, ends = hand_built(fields)
    want = (b.n + bins + 7) // 8
    header_bytes = (b.n + 7) // 8
    data = b.bytes()
    assert probe.extent(data, dt, major) == (want, OK)               # the header alone: the bins are not asked to be there
    assert probe.extent(data + b"\xFF" * 40, dt, major) == (want, OK)
    for cut in range(header_bytes):                                  # cut after every byte, which is after every field and inside every field
        assert probe.extent(data[:cut], dt, major) == (0, INSUFFICIENT), cut
    # ... and through the verdict: a chunk of exactly the preamble and this header is too short unless it has no bins
    n = 300
    chunk = bytes([dt]) + (n - 1).to_bytes(3, "little") + data
    v = probe.verdict(chunk, 0, len(chunk), 0, len(chunk), dt, n, major)
    assert v == ((4, want, 4 + want, 0, OK) if want == header_bytes else (0, 0, 0, 0, INSUFFICIENT))


@pytest.mark.parametrize("nibble", range(5, 16))
def test_an_unknown_mode_is_corruption(probe, nibble):
    assert probe.extent(bytes([nibble]) + b"\0" * 8, 1) == (0, CORRUPTION)
    assert probe.extent(bytes([nibble]), 1) == (0, CORRUPTION)      # one byte is enough to know
    assert probe.extent(b"", 1) == (0, INSUFFICIENT)


@pytest.mark.parametrize("variant", range(4, 16))
def test_an_unknown_delta_variant_is_corruption_from_format_3_on(probe, variant):
    data = bytes([variant << 4]) + b"\0" * 8
    assert probe.extent(data, 1, 4) == (0, CORRUPTION) and probe.extent(data, 1, 3) == (0, CORRUPTION)
    assert probe.extent(data, 1, 2)[1] == OK                        # (below 3 the bits are an order)
    assert probe.extent(bytes([1, 0, 0, 0, variant << 4]) + b"\0" * 16, 1, 4) == (0, CORRUPTION)   # behind an IntMult base: bit 36


def test_the_dict_and_conv1_terms_count(probe):
    """the two terms a closed form is most likely to lose: dict_n * L bits behind the padding, and 32 bits per weight"""
    for dict_n in (0, 1, 5, 1000):
        b, _ = hand_built([(4, 4), (dict_n, 25), "pad", (0, dict_n * 64), (0, 4), (0, 4), (0, 15)])
        assert probe.extent(b.bytes(), 2) == (4 + dict_n * 8 + 3, OK)
    for w in (1, 2, 32):
        b, _ = hand_built([(0, 4), (3, 4), (0, 5), (0, 64), (w - 1, 5), (0, 32 * w), (0, 4), (0, 15)])
        assert probe.extent(b.bytes(), 1) == ((8 + 5 + 64 + 5 + 32 * w + 19 + 7) // 8, OK)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the verdict's table, row by row and in its order
# ---------------------------------------------------------------------------------------------------------------------------------------
def good_chunk(dt=1, n=300):
    b, _ = hand_built([(0, 4), (0, 4), (2, 4), (3, 15)])
    meta = (b.v).to_bytes((b.n + bins_bits(3, 2, 32) + 7) // 8, "little")
    return bytes([dt]) + (n - 1).to_bytes(3, "little") + meta + b"\x11" * 9, len(meta)


REFUSED = lambda st: (0, 0, 0, 0, st)   # noqa: E731


@pytest.mark.parametrize("gap", [0, 4])
def test_every_row_of_the_table_in_its_order(probe, gap):
    chunk, meta_len = good_chunk()
    blob = b"\xEE" * 8 + b"\xDD" * gap + chunk
    c0, c1, end, n = 8, len(blob), len(blob), 300
    ok = (c0 + gap + 4, meta_len, c0 + gap + 4 + meta_len, 9, OK)
    run = lambda **kw: probe.verdict(kw.get("blob", blob), gap, kw.get("end", end), kw.get("c0", c0), kw.get("c1", c1), kw.get("dtype", 1), kw.get("page_n", n), 4, kw.get("blob_len"))   # noqa: E731
    assert run() == ok
    # 1. the sentinel -- in front of everything, a swapped pair and a dropped chunk included
    assert run(end=ALL_ONES) == REFUSED(INVALID) and run(end=ALL_ONES, c0=c1, c1=c0) == REFUSED(INVALID) and run(end=ALL_ONES, c1=c0) == REFUSED(INVALID)
    # 2. a swapped pair, an end beyond blob_len -- in front of "dropped" and of the gap
    assert run(c0=c1, c1=c0) == REFUSED(INVALID) and run(blob_len=c1 - 1) == REFUSED(INVALID) and run(c0=c1 + 5, c1=c1 + 5) == REFUSED(INVALID)
    assert run(blob_len=c1) == ok
    # 3. dropped -- in front of the gap check and of the preamble
    assert run(c1=c0) == REFUSED(INSUFFICIENT) and run(c0=0, c1=0) == REFUSED(INSUFFICIENT)
    # 4. an extent below the gap
    if gap:
        assert run(c1=c0 + 1) == REFUSED(INVALID) and run(c1=c0 + gap - 1) == REFUSED(INVALID)
    # 5. fewer than 4 bytes behind the gap -- in front of the dtype byte, which is wrong here as well
    for k in range(0 if gap else 1, 4):
        assert run(c1=c0 + gap + k) == REFUSED(INSUFFICIENT) and run(c1=c0 + gap + k, dtype=2) == REFUSED(INSUFFICIENT)
    # 6. the dtype byte -- in front of n; a terminator's 0 included
    assert run(dtype=3) == REFUSED(CORRUPTION) and run(dtype=3, page_n=n + 1) == REFUSED(CORRUPTION)
    zero = bytearray(blob); zero[c0 + gap] = 0
    assert run(blob=bytes(zero)) == REFUSED(CORRUPTION)
    # 7. n -- in front of the ChunkMeta: an unknown mode nibble behind a wrong n is the wrong n
    bad_mode = bytearray(blob); bad_mode[c0 + gap + 4] |= 0x0F
    assert run(page_n=n - 1) == REFUSED(INVALID) and run(page_n=n + 1) == REFUSED(INVALID) and run(blob=bytes(bad_mode), page_n=n + 1) == REFUSED(INVALID)
    assert run(page_n=1 << 24) == REFUSED(INVALID)
    # 8. chunk_meta_extent's status
    assert run(blob=bytes(bad_mode)) == REFUSED(CORRUPTION)
    assert run(c1=c0 + gap + 4) == REFUSED(INSUFFICIENT) and run(c1=c0 + gap + 6) == REFUSED(INSUFFICIENT)
    # 9. a ChunkMeta longer than what is left
    assert run(c1=c0 + gap + 4 + meta_len - 1) == REFUSED(INSUFFICIENT)
    # 10. a page of 0 bytes is legal
    assert run(c1=c0 + gap + 4 + meta_len) == (c0 + gap + 4, meta_len, c0 + gap + 4 + meta_len, 0, OK)
    # n = 2^24 reads back from 24 bits of ones
    big, ml = good_chunk(n=1 << 24)
    assert probe.verdict(big, 0, len(big), 0, len(big), 1, 1 << 24)[4] == OK and big[1:4] == b"\xff\xff\xff"


def test_gap_is_part_of_where_the_chunk_starts(probe):
    """with gap 4 the preamble is read 4 bytes in: the same bytes under gap 0 are another chunk"""
    chunk, meta_len = good_chunk()
    blob = bytes([1, 0, 0, 0]) + chunk   # (the gap's bytes look like a preamble with n = 1)
    assert probe.verdict(blob, 4, len(blob), 0, len(blob), 1, 300)[4] == OK
    assert probe.verdict(blob, 0, len(blob), 0, len(blob), 1, 300)[4] == INVALID     # n = 1 there
    assert probe.verdict(blob, 4, len(blob), 0, len(blob), 1, 1)[4] == INVALID


def test_a_sanitised_stand_alone_program_reads_nothing_beyond_any_cut(tmp_path):
    """g++ -fsanitize=address,undefined over a program with its own main: every case's chunk, cut after every byte into a heap block of exactly that
    many bytes, through chunk_verdict under gaps 0 and 4 -- a read past a cut is a heap-buffer-overflow and the program's exit status says so"""
    cs = [c for c in cases() if len(c[1]) < 6000]
    data = tmp_path / "chunks.bin"
    with open(data, "wb") as f:
        for name, chunk, dt, major, meta, meta_len, n, page in cs:
            f.write(np.array([len(chunk), dt, major, n, meta_len], "<u8").tobytes() + chunk)
    src = tmp_path / "main.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "%s/pco_chunk_dir.h"
using namespace pcogfx;
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  uint64_t h[5]; long runs = 0;
  while (fread(h, 8, 5, f) == 5) {
    std::vector<uint8_t> chunk(h[0]); if (fread(chunk.data(), 1, h[0], f) != h[0]) return 3;
    for (uint32_t gap = 0; gap <= 4; gap += 4)
      for (uint64_t cut = 0; cut <= h[0]; cut += (cut < h[4] + 8 || cut + 8 > h[0]) ? 1 : 97) {
        uint8_t* blob = (uint8_t*)malloc(gap + cut + 1);   // (+ 1: malloc(0) may be null; the byte is beyond blob_len and never the chunk's)
        memset(blob, 0xEE, gap + cut + 1); memcpy(blob + gap, chunk.data(), cut);
        const DirVerdict v = chunk_verdict(blob, gap + cut, gap, gap + cut, 0, gap + cut, (uint32_t)h[1], h[3], (uint32_t)h[2]);
        const bool whole = cut >= 4 + h[4];
        if ((v.status == kDirOk) != whole) { printf("chunk of %%llu bytes cut at %%llu: status %%u\n", (unsigned long long)h[0], (unsigned long long)cut, v.status); return 4; }
        if (whole && (v.meta != blob + gap + 4 || v.meta_len != h[4] || v.page != v.meta + h[4] || v.page_len != cut - 4 - h[4])) return 5;
        if (!whole && (v.meta != blob || v.page != blob || v.meta_len || v.page_len)) return 6;
        free(blob); runs++;
      }
  }
  printf("%%ld verdicts\n", runs);
  return runs > 1000 ? 0 : 7;
}
''' % CSRC)
    exe = tmp_path / "main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header, the binding, the host checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entry_points_over_the_same_structs_and_the_library_exports_them():
    text = open(HEADER).read()
    tail = r"\s*PcoGfxTaskResult\* results, PcoGfxTaskResult\* d_results, void\* stream\);"
    assert re.search(r"enum PcoError pco_gfx_decompress_chunks_dir\(size_t n_tasks, const PcoGfxDirPageTask\* tasks, const PcoGfxDirectory\* dir," + tail, text)
    assert re.search(r"enum PcoError pco_gfx_decompress_chunk_reads_dir\(size_t n_tasks, const PcoGfxDirPageReadTask\* tasks, const PcoGfxDirectory\* dir, uint32_t flags," + tail, text)
    assert re.search(r"enum PcoError pco_gfx_index_chunks_dir\(size_t n_tasks, const PcoGfxDirPageIndexTask\* tasks, const PcoGfxDirectory\* dir, uint32_t flags," + tail, text)
    assert re.search(r"enum PcoError pco_gfx_standalone_chunk_split\(const void\* chunk, size_t len, unsigned char dtype, uint8_t format_major, uint64_t\* n,\s*uint64_t\* meta_len, uint64_t\* page_len\);", text)
    for name in ("pco_gfx_decompress_chunks_dir", "pco_gfx_decompress_chunk_reads_dir", "pco_gfx_index_chunks_dir", "pco_gfx_standalone_chunk_split"):
        assert hasattr(G.lib(), name) and name in G.SIGNATURES
    assert G.SIGNATURES["pco_gfx_decompress_chunks_dir"] == G.SIGNATURES["pco_gfx_decompress_pages_dir"]
    assert G.SIGNATURES["pco_gfx_decompress_chunk_reads_dir"] == G.SIGNATURES["pco_gfx_decompress_page_reads_dir"] == G.SIGNATURES["pco_gfx_index_chunks_dir"]
    # no struct of its own: the header has none, and the binding's kinds add no field
    assert "DirChunk" not in text
    for chunk_kind, page_kind in ((G.DirChunkTask, G.DirPageTask), (G.DirChunkReadTask, G.DirPageReadTask), (G.DirChunkIndexTask, G.DirPageIndexTask)):
        assert issubclass(chunk_kind, page_kind) and C.sizeof(chunk_kind) == C.sizeof(page_kind)
        assert [getattr(chunk_kind, n).offset for n, _ in page_kind._fields_] == [getattr(page_kind, n).offset for n, _ in page_kind._fields_]


P = 0x1000   # (never dereferenced: every call below is refused by the argument checks)
GOOD_DIR = dict(d_blob=P, blob_len=100, d_offsets=P, n_pieces=8, gap=0, reserved=0)
GOOD_PAGE = dict(dst=P, page_n=10, meta_piece=1, page_piece=1, dtype=1, format_major=4)
GOOD_READ = dict(dst=P, page_n=10, first=0, count=1, meta_piece=1, page_piece=1, dtype=1, format_major=4, from_=P, to=P, history=P, history_len=80)
GOOD_INDEX = dict(cursors=P, page_n=1000, every_rows=256, meta_piece=1, page_piece=1, dtype=1, format_major=4, histories=P, history_stride=80)
KINDS = {"page": (G.DirPageTask, GOOD_PAGE, "pco_gfx_decompress_chunks_dir", False),
         "read": (G.DirPageReadTask, GOOD_READ, "pco_gfx_decompress_chunk_reads_dir", True),
         "index": (G.DirPageIndexTask, GOOD_INDEX, "pco_gfx_index_chunks_dir", True)}

# section 4e's list, then the fields every task kind has: the rows of the page forms' tests with the chunk's one piece named twice
COMMON = [
    (dict(no_tasks=True), INVALID),
    (dict(no_dir=True), INVALID),
    (dict(directory=dict(d_blob=None)), INVALID),
    (dict(directory=dict(d_offsets=None)), INVALID),
    (dict(no_results=True), INVALID),                                        # results and d_results both NULL
    (dict(directory=dict(n_pieces=1 << 31)), INVALID),
    (dict(task=dict(meta_piece=8, page_piece=8)), INVALID),                  # a piece index >= n_pieces
    (dict(task=dict(meta_piece=0xFFFFFFFF, page_piece=0xFFFFFFFF)), INVALID),
    (dict(task=dict(dtype=0)), INVALID),
    (dict(task=dict(dtype=12)), INVALID),
    (dict(task=dict(page_n=0)), INVALID),
    (dict(task=dict(page_n=(1 << 24) + 1)), INVALID),
    (dict(task=dict(format_major=5)), CORRUPTION),
    (dict(task=dict(format_major=5, meta_piece=8, page_piece=8)), CORRUPTION),   # the version first
]
PIECES = [
    (dict(task=dict(meta_piece=0, page_piece=1)), INVALID),                 # the one difference from the page forms: a chunk is ONE piece
    (dict(task=dict(meta_piece=1, page_piece=0)), INVALID),
    (dict(task=dict(meta_piece=7, page_piece=6)), INVALID),
    (dict(task=dict(meta_piece=1, page_piece=8)), INVALID),                 # beyond the directory
    (dict(task=dict(meta_piece=8, page_piece=1)), INVALID),
    (dict(task=dict(meta_piece=0, page_piece=1, format_major=5)), CORRUPTION),
]
PAGE_ONLY = [(dict(task=dict(dst=None)), INVALID)]
READ_ONLY = [   # sections 4f and 4i
    (dict(task=dict(dst=None)), INVALID),                                    # with count > 0
    (dict(task=dict(first=5, count=6)), INVALID),                            # first + count > page_n
    (dict(task=dict(first=10, count=1)), INVALID),
    (dict(task=dict(first=11, count=0)), INVALID),
    (dict(task=dict(first=ALL_ONES, count=2)), INVALID),                     # the sum wraps
    (dict(task=dict(page_n=0, first=0, count=0)), INVALID),
    (dict(task=dict(history=P, history_len=0)), INVALID),
    (dict(task=dict(history=None, history_len=80)), INVALID),
    (dict(task=dict(history=P + 4)), INVALID),                               # misaligned
    (dict(task=dict(history=P + 1)), INVALID),
    (dict(task=dict(history=P, history_len=0, count=0)), INVALID),           # the pair is judged whatever the count is
]
INDEX_ONLY = [   # sections 4g and 4j
    (dict(task=dict(every_rows=0)), INVALID),
    (dict(task=dict(every_rows=100)), INVALID),
    (dict(task=dict(every_rows=257)), INVALID),
    (dict(task=dict(every_rows=ALL_ONES)), INVALID),
    (dict(task=dict(every_rows=100, page_n=50, cursors=None)), INVALID),     # a bad every_rows is refused whatever k would be
    (dict(task=dict(cursors=None)), INVALID),                                # k = 3
    (dict(task=dict(cursors=P + 4)), INVALID),                               # misaligned
    (dict(task=dict(cursors=P + 1)), INVALID),
    (dict(task=dict(histories=P, history_stride=0)), INVALID),
    (dict(task=dict(histories=None, history_stride=80)), INVALID),
    (dict(task=dict(history_stride=84)), INVALID),                           # no multiple of 8
    (dict(task=dict(history_stride=81)), INVALID),
    (dict(task=dict(histories=P + 4)), INVALID),                             # misaligned
    (dict(task=dict(histories=P, history_stride=0, page_n=50)), INVALID),    # the pair is judged whatever k is
]
CASES = ([("page", kw, st) for kw, st in COMMON + PIECES + PAGE_ONLY] + [("read", kw, st) for kw, st in COMMON + READ_ONLY + PIECES]
         + [("index", kw, st) for kw, st in COMMON + INDEX_ONLY + PIECES])


def call(kind, flags=0, form="sync", task=None, directory=None, no_tasks=False, no_dir=False, no_results=False, n_tasks=1):
    struct, good, name, with_flags = KINDS[kind]
    kw = dict(good); kw.update(task or {})
    arr = (struct * 1)(struct(**kw))
    dkw = dict(GOOD_DIR); dkw.update(directory or {})
    d = G.Directory(**dkw)
    res = (G.TaskResult * 1)(); res[0].n_out = 77; res[0].consumed = 78; res[0].status = 99; res[0].aux = 98
    host, dev = (None if no_results else res, None) if form == "sync" else (None, None if no_results else P)
    args = [n_tasks, None if no_tasks else arr, None if no_dir else C.addressof(d)] + ([flags] if with_flags else []) + [host, dev, None]
    code = getattr(G.lib(), name)(*args)
    return code, G.lib().pco_gfx_last_status(), res[0]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("kind,kw,status", CASES)
def test_every_host_check_comes_before_a_device_is_asked_for(kind, kw, status, flags, form):
    code, st, res = call(kind, flags, form, **kw)
    assert code == G.PcoDecompressionError and st == status
    assert (res.n_out, res.consumed, res.status, res.aux) == (77, 78, 99, 98)   # nothing was written


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("kind", ["read", "index"])
@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFF])
def test_an_unknown_flag_bit_is_refused_before_anything_else(flags, kind, form):
    for kw in ({}, dict(no_dir=True), dict(no_tasks=True)):
        code, st, res = call(kind, flags, form, **kw)
        assert code == G.PcoDecompressionError and st == INVALID and res.status == 99


@pytest.mark.parametrize("kind", ["page", "read", "index"])
def test_no_tasks_is_a_success_without_a_device_given_a_directory_and_results(kind):
    assert call(kind, n_tasks=0, no_tasks=True)[0] == G.PcoSuccess and call(kind, 0, "async", n_tasks=0, no_tasks=True)[0] == G.PcoSuccess
    assert call(kind, n_tasks=0, no_results=True)[:2] == (G.PcoDecompressionError, INVALID)
    assert call(kind, n_tasks=0, no_dir=True)[:2] == (G.PcoDecompressionError, INVALID)


def test_the_page_forms_keep_refusing_one_piece_for_both():
    """(unchanged behaviour: this test passes on the commit before as well)"""
    L = G.lib(); d = G.Directory(**GOOD_DIR); res = (G.TaskResult * 1)()
    same = dict(meta_piece=3, page_piece=3)
    calls = [(L.pco_gfx_decompress_pages_dir, G.DirPageTask(**dict(GOOD_PAGE, **same)), ()),
             (L.pco_gfx_decompress_page_ranges_dir, G.DirPageRangeTask(dst=P, page_n=10, first=0, count=1, dtype=1, format_major=4, **same), ()),
             (L.pco_gfx_decompress_page_reads_dir, G.DirPageReadTask(**dict(GOOD_READ, **same)), (0,)),
             (L.pco_gfx_index_pages_dir, G.DirPageIndexTask(**dict(GOOD_INDEX, **same)), (0,))]
    for fn, task, flags in calls:
        arr = (type(task) * 1)(task)
        assert fn(1, arr, C.addressof(d), *flags, res, None, None) == G.PcoDecompressionError and L.pco_gfx_last_status() == INVALID


# ---------------------------------------------------------------------------------------------------------------------------------------
# pcodec_amd.paged: the task lists of _DirChunks, field for field
# ---------------------------------------------------------------------------------------------------------------------------------------
NS = [3000, 257, 1]
NAMES = ["uint32", "int64", "float16"]
EVERY = 256


class Lib(U.FakeLib):
    FORWARDED = U.FakeLib.FORWARDED + ("pco_gfx_lookback_window_n_log", "pco_gfx_lookback_history_bytes")
    DIR_FORMS = U.FakeLib.DIR_FORMS + ("pco_gfx_decompress_page_reads_dir", "pco_gfx_index_pages_dir", "pco_gfx_decompress_chunks_dir", "pco_gfx_decompress_chunk_reads_dir",
                                       "pco_gfx_index_chunks_dir")


@pytest.fixture()
def stand_ins(monkeypatch):
    if B.needs_build():
        B.build()
    from pcodec_amd import paged
    G.lib()
    real_torch = sys.modules.get("torch")
    torch = sys.modules["torch"] = U.FakeTorch()
    lib = Lib(G)
    monkeypatch.setattr(paged, "_require_device", lambda: lib)
    try:
        blob = torch.empty(100000 + 64, dtype=torch.uint8, device="cuda"); offsets = torch.empty(len(NS) + 1, dtype=torch.int64, device="cuda")
        cc = paged.CompressedStandaloneChunks(blob, offsets, None, NS, NAMES, 11, None, None)
        yield paged, lib, cc
    finally:
        if real_torch is None:
            sys.modules.pop("torch", None)
        else:
            sys.modules["torch"] = real_torch


def rows_of(struct, call_):
    return [dict(zip([n for n, _ in struct._fields_], t)) for t in call_["tasks"]]


def test_whole_chunks_and_rows_are_one_task_per_chunk_by_its_piece(stand_ins):
    paged, lib, cc = stand_ins
    torch = sys.modules["torch"]
    base = torch._next
    outs, results = paged.decompress_chunks_async(cc)
    (d,) = lib.calls
    assert d["fn"] == "pco_gfx_decompress_chunks_dir" and d["dir"] == [cc.blob.data_ptr(), cc.blob.numel() - 64, cc.offsets.data_ptr(), 3, 0, 0]
    assert d["args"] == [None, results.data_ptr(), U.STREAM_HANDLE]
    t = rows_of(G.DirPageTask, d)
    assert [(x["page_n"], x["meta_piece"], x["page_piece"], x["dtype"], x["format_major"]) for x in t] == [(3000, 0, 0, 1, 4), (257, 1, 1, 4, 4), (1, 2, 2, 9, 4)]
    assert [o.shape[0] for o in outs] == NS and t[0]["dst"] == base and t[0]["dst"] < t[1]["dst"] < t[2]["dst"]
    lib.calls.clear()
    outs, results = paged.decompress_rows_async(cc, [(990, 2100), None, (0, 1)])
    (d,) = lib.calls
    assert d["fn"] == "pco_gfx_decompress_chunk_reads_dir" and d["args"] == [0, None, results.data_ptr(), U.STREAM_HANDLE]
    t = rows_of(G.DirPageReadTask, d)
    assert [(x["page_n"], x["first"], x["count"], x["meta_piece"], x["page_piece"], x["dtype"]) for x in t] == [(3000, 990, 1110, 0, 0, 1), (1, 0, 1, 2, 2, 9)]
    assert all((x["from_"], x["to"], x["history"], x["history_len"]) == (None, None, None, 0) for x in t)   # a read without cursors: a row range
    assert [o.shape[0] for o in outs] == [1110, 1]


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("history", [False, True])
def test_the_index_and_the_reads_from_it(stand_ins, history, general):
    paged, lib, cc = stand_ins
    idx = paged.index_pages_async(cc, EVERY, general=general, history=history)
    (d,) = lib.calls
    assert d["fn"] == "pco_gfx_index_chunks_dir" and d["args"] == [1 if general else 0, None, idx.results.data_ptr(), U.STREAM_HANDLE] and d["dir"][3:5] == [3, 0]
    t = rows_of(G.DirPageIndexTask, d)
    ks = [(n - 1) // EVERY for n in NS]
    assert ks == [11, 1, 0]
    assert [(x["page_n"], x["every_rows"], x["meta_piece"], x["page_piece"], x["dtype"], x["format_major"]) for x in t] == [(n, EVERY, c, c, G.DTYPE_BYTE[nm], 4) for c, (n, nm) in enumerate(zip(NS, NAMES))]
    assert [x["cursors"] for x in t] == [pc.cursors.data_ptr() if k else None for pc, k in zip(idx, ks)]
    assert [(pc.chunk, pc.piece, pc.every_rows, pc.cursors.shape) for pc in idx] == [(c, 1, EVERY, (k, 256)) for c, k in enumerate(ks)]
    if history:
        want = [(G.lib().pco_gfx_lookback_history_bytes(G.lib().pco_gfx_lookback_window_n_log(n), G.DTYPE_BYTE[nm]) + 7) // 8 * 8 for n, nm in zip(NS, NAMES)]
        assert [x["history_stride"] for x in t] == [s if k else 0 for s, k in zip(want, ks)]
        assert [x["histories"] for x in t] == [h.data_ptr() if k else None for h, k in zip(idx.histories, ks)]
    else:
        assert all((x["histories"], x["history_stride"]) == (None, 0) for x in t) and idx.histories is None
    lib.calls.clear()
    outs, results = paged.decompress_chunks_from_async(cc, idx, general=general)
    (d,) = lib.calls
    assert d["fn"] == "pco_gfx_decompress_chunk_reads_dir" and d["args"][0] == (1 if general else 0)
    t = rows_of(G.DirPageReadTask, d)
    want = [(c, row, min(EVERY, n - row), s) for c, n in enumerate(NS) for s, row in enumerate(range(0, n, EVERY if (n - 1) // EVERY else n))]
    assert [(x["meta_piece"], x["first"], x["count"]) for x in t] == [(c, row, cnt) for c, row, cnt, s in want] and all(x["meta_piece"] == x["page_piece"] for x in t)
    assert [x["from_"] for x in t] == [None if s == 0 else idx[c].cursors.data_ptr() + (s - 1) * 256 for c, row, cnt, s in want] and all(x["to"] is None for x in t)
    if history:
        assert [x["history"] for x in t] == [None if s == 0 else idx.histories[c].data_ptr() + (s - 1) * idx.histories[c].shape[1] for c, row, cnt, s in want]
    lib.calls.clear()
    outs, results = paged.decompress_rows_from_async(cc, idx, [(700, 701), (0, 257), None], general=general)
    (d,) = lib.calls
    t = rows_of(G.DirPageReadTask, d)
    assert d["fn"] == "pco_gfx_decompress_chunk_reads_dir"
    assert [(x["meta_piece"], x["first"], x["count"], x["from_"]) for x in t] == [(0, 700, 1, idx[0].cursors.data_ptr() + 256), (1, 0, 257, None)]
