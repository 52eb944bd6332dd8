"""-m gpu: pco_gfx_scan_chunks (include/pco_gfx.h section 4m) -- the chunk directory of standalone streams found on the device -- and
pcodec_amd.paged.scan_files / decompress_files over it.

Truth is one of two things.  For files written here, the offsets pco_gfx_compact_chunks left: the encoder knows its lengths, so they are independent
of any walk.  For everything else, the CHAIN the header defines: pco_gfx_decompress_chunks with one PCO_GFX_TASK_ONE_CHUNK task per step (code from
before the scan), the first step with the file-header flag, the later ones with the version, while aux bit 0 is set and fewer than max_chunks chunks
are decoded.  A chain step's dst has room for 2^24 numbers where a stream is foreign; the cut and damaged copies of the 3-chunk file run their chains
in lockstep, hundreds of tasks a call, with room for 512: dst_cap takes part in ONE check, n > dst_cap, behind the preamble's own, and every
preamble there that is whole says n = 300.  The format version of the later steps and the header's length come from the format's arithmetic in
Python.  Every scan's two output arrays are filled with canaries first and compared whole.

Shapes: chunks of 1, 255, 256, 257 and 3000 numbers (8192 for the level-12 table); files of 1, 2, 3 and 65 chunks.

Measured on an MI355X: 47 tests in 2.4 to 2.8 s, the encodes of the 16 files (once) included."""
import ctypes as C
import glob
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402

pytestmark = pytest.mark.gpu

_u8, _u4 = "<u8", "<u4"
SCAN_DT = np.dtype([("src", _u8), ("src_len", _u8), ("d_offsets", _u8), ("d_counts", _u8), ("max_chunks", _u4), ("dtype", _u4), ("flags", _u4), ("reserved", _u4)])
DIRREAD_DT = np.dtype([("dst", _u8), ("page_n", _u8), ("first", _u8), ("count", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4),
                       ("from", _u8), ("to", _u8), ("history", _u8), ("history_len", _u8)])
DIRINDEX_DT = np.dtype([("cursors", _u8), ("page_n", _u8), ("every_rows", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4),
                        ("histories", _u8), ("history_stride", _u8)])
assert (SCAN_DT.itemsize, DIRREAD_DT.itemsize, DIRINDEX_DT.itemsize) == (48, 80, 56)
CAN_O, CAN_C = 0x1111111111111111, 0x22222222
HEADER, ONE_CHUNK = 1, 8
OK, CORRUPTION, INSUFFICIENT = G.ST_OK, G.ST_CORRUPTION, G.ST_INSUFFICIENT_DATA
ASSETS = sorted(glob.glob(os.path.join(HERE, "golden", "ref_assets", "*.pco")))
LDS_TABLE_BUDGET = 16 * 1024 - 5472   # the general kernel's dynamic LDS less its fixed area (decode_kernel.hip, kLdsFixed)

Scan = namedtuple("Scan", "n_out consumed status aux offsets counts")
Row = namedtuple("Row", "stream start dtype max_chunks flags hdr version", defaults=(0, 4))   # hdr: the header's length where flags has HEADER and the header is whole


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    lib.pco_gfx_compact_chunks.argtypes = U.COMPACT_ARGTYPES
    return lib


@pytest.fixture(autouse=True)
def nothing_more_after_a_device_error(L):
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error; nothing more is launched on it: {e}", returncode=3)


def file_header(f):
    """(bytes in front of the first chunk, the format's major version) by the format's arithmetic (standalone/decompressor.rs:85-137)"""
    assert f[:4] == b"pco!"
    at = 4; sv = f[4]
    if sv >= 2:
        at = 5 + (1 if sv >= 3 else 0)
        at += (6 + 1 + (f[at] & 63) + 7) // 8
    major = f[at]
    return at + (2 if major >= 4 else 1), major


# ---------------------------------------------------------------------------------------------------------------------------------------
# the harness: streams side by side on the device, one scan call over rows of them, the chain over the same rows
# ---------------------------------------------------------------------------------------------------------------------------------------
class Streams:
    """Byte strings side by side in one device tensor, each behind 64 readable bytes that are not its own."""

    def __init__(self, datas):
        import torch
        self.datas = [bytes(d) for d in datas]
        self.bases = []; total = 0
        for d in self.datas:
            self.bases.append(total); total += (len(d) + 64 + 15) // 16 * 16
        self.host = np.full(total + 64, 0xC3, np.uint8)
        for d, b in zip(self.datas, self.bases):
            self.host[b: b + len(d)] = np.frombuffer(d, np.uint8)
        self.blob = torch.from_numpy(self.host.copy()).cuda()
        torch.cuda.synchronize()

    def ptr(self, i, start=0):
        return self.blob.data_ptr() + self.bases[i] + start

    def unchanged(self):
        return np.array_equal(self.blob.cpu().numpy(), self.host)


def scan(L, s, rows, form="sync", stream=None, keep=None):
    """ONE pco_gfx_scan_chunks call over `rows`; [Scan], offsets and counts trimmed to what the result names.  Both arrays lie in one area between
    canaries, and everything of it the results do not name must be unchanged."""
    import torch
    k = len(rows)
    caps = [r.max_chunks for r in rows]
    o_at = np.concatenate([[0], np.cumsum([c + 1 for c in caps])]).astype(np.int64)
    c_at = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    d_off = torch.full((int(o_at[-1]) + 2,), CAN_O, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((int(c_at[-1]) + 2,), CAN_C, dtype=torch.int32, device="cuda")
    d_res = torch.full((k * 3 + 1,), 0x55, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t = np.zeros(k, SCAN_DT)
    for i, r in enumerate(rows):
        t[i] = (s.ptr(r.stream, r.start), len(s.datas[r.stream]) - r.start, d_off.data_ptr() + 8 * (1 + int(o_at[i])), d_cnt.data_ptr() + 4 * (1 + int(c_at[i])), r.max_chunks, r.dtype, r.flags, 0)
    res = np.zeros(k, U.RES_DT)
    sh = None if stream is None else stream.cuda_stream
    code = L.pco_gfx_scan_chunks(k, U.ptr(t), U.ptr(res) if form == "sync" else None, d_res.data_ptr(), sh)
    t[:] = 0   # (the library copied the tasks)
    if keep is not None:   # the pipeline test goes on in the stream's order
        keep.update(d_off=d_off, d_cnt=d_cnt, d_res=d_res, o_at=o_at, c_at=c_at, code=code)
        return None
    torch.cuda.synchronize()
    dev = d_res.cpu().numpy()[: k * 3].view(U.RES_DT)
    if form == "sync":
        assert np.array_equal(res, dev), "the host results are the device's"
        assert (code == G.PcoSuccess) == bool((res["status"] == 0).all())
    else:
        assert code == G.PcoSuccess
    off = d_off.cpu().numpy().view(np.uint64); cnt = d_cnt.cpu().numpy().view(np.uint32)
    want_off = np.full(off.size, CAN_O, np.uint64); want_cnt = np.full(cnt.size, CAN_C, np.uint32)
    out = []
    for i in range(k):
        n = int(dev["n_out"][i]); assert n <= caps[i]
        a, b = 1 + int(o_at[i]), 1 + int(c_at[i])
        want_off[a: a + n + 1] = off[a: a + n + 1]; want_cnt[b: b + n] = cnt[b: b + n]
        out.append(Scan(n, int(dev["consumed"][i]), int(dev["status"][i]), int(dev["aux"][i]), tuple(int(x) for x in off[a: a + n + 1]), tuple(int(x) for x in cnt[b: b + n])))
    assert np.array_equal(off, want_off) and np.array_equal(cnt, want_cnt), "an entry outside [0, n_out] / [0, n_out) was written"
    return out


def chain(L, s, rows, dst_cap, lockstep):
    """The chain of one-chunk decodes per row -> [Scan] as the header derives the scan's fields from it.  lockstep: every row's step k in ONE
    pco_gfx_decompress_chunks call (each row a dst of its own); else row after row, through one dst."""
    import torch
    width = 8
    n_dst = len(rows) if lockstep else 1
    dst = torch.empty(n_dst * dst_cap * width + 64, dtype=torch.uint8, device="cuda")
    st = [dict(off=r.start, end=r.start, k=0, starts=[], counts=[], status=OK, aux=0, done=False, first=True) for r in rows]   # off: the next step's start; end: behind the last chunk found
    groups = [list(range(len(rows)))] if lockstep else [[i] for i in range(len(rows))]
    for group in groups:
        while True:
            act = [i for i in group if not st[i]["done"]]
            if not act:
                break
            t = np.zeros(len(act), U.DEC_DT)
            for j, i in enumerate(act):
                r, x = rows[i], st[i]
                with_header = x["first"] and (r.flags & HEADER)
                flags = ONE_CHUNK | (HEADER if with_header else ((r.version if (r.flags & HEADER) else (r.flags >> 8) & 0xFF) << 8))
                t[j] = (s.ptr(r.stream, x["off"]), len(s.datas[r.stream]) - x["off"], dst.data_ptr() + (i if lockstep else 0) * dst_cap * width, dst_cap, r.dtype, flags)
            res = np.zeros(len(act), U.RES_DT)
            L.pco_gfx_decompress_chunks(len(act), U.ptr(t), U.ptr(res), None, None)
            for j, i in enumerate(act):
                r, x = rows[i], st[i]
                status, n_out, consumed, aux = int(res["status"][j]), int(res["n_out"][j]), int(res["consumed"][j]), int(res["aux"][j])
                with_header = x["first"] and (r.flags & HEADER)
                lead = r.hdr if with_header else 0   # the header's bytes in this step's consumed
                if status != OK:   # the failing chunk's start: behind the last chunk found -- behind the header when the step read one and it is whole
                    if with_header and len(s.datas[r.stream]) - r.start >= r.hdr:
                        x["end"] = r.start + r.hdr
                    x.update(status=status, aux=0, done=True)
                elif n_out == 0:   # no chunk: the stream's end, or the terminator where a preamble would stand (which the step says through consumed alone)
                    took = consumed - lead
                    assert took in (0, 1)
                    x.update(aux=2 if took else 0, done=True, end=x["off"] + lead, off=x["off"] + consumed)
                else:
                    x["starts"].append(x["off"] + lead); x["counts"].append(n_out); x["k"] += 1
                    x.update(aux=aux & 3, end=x["off"] + consumed - (1 if aux & 2 else 0), off=x["off"] + consumed)
                    if not (aux & 1) or x["k"] >= r.max_chunks:
                        x["done"] = True
                x["first"] = False
    out = []
    for r, x in zip(rows, st):
        version = r.version if (r.flags & HEADER) else (((r.flags >> 8) & 0xFF) or 4)
        end = x["end"] - r.start
        out.append(Scan(x["k"], end + (1 if x["aux"] & 2 else 0), x["status"], x["aux"] | (version << 8), tuple(a - r.start for a in x["starts"]) + (end,), tuple(x["counts"])))
    return out


def strip_version_of_refused_headers(got, want, rows, s):
    """a header that is refused names no version the chain could know: compare aux without bits 8..15 there"""
    out = []
    for g, w, r in zip(got, want, rows):
        if (r.flags & HEADER) and g.status != OK and g.n_out == 0 and len(s.datas[r.stream]) - r.start < r.hdr:
            g = g._replace(aux=g.aux & 0xFF); w = w._replace(aux=w.aux & 0xFF)
        out.append((g, w))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# files written here: one encode call per file, compacted behind a header, a terminator behind the last chunk
# ---------------------------------------------------------------------------------------------------------------------------------------
def numbers(name, n, kind, seed=1):
    rng = np.random.default_rng(seed + n); dt = np.dtype(name)
    if kind == "constant":
        return np.full(n, 7, dt)
    if kind == "mult":
        base = rng.integers(0, 100, n)
        return (base * 7).astype(dt) if dt.kind != "f" else (base * 0.25).astype(dt)
    if kind == "smooth":
        return (np.cumsum(rng.integers(-3, 4, n)) + 1000).astype(dt)
    if kind == "periodic":
        return (rng.integers(0, 100, 37)[np.arange(n) % 37] + rng.integers(0, 3, n)).astype(dt)
    if kind == "few":
        return rng.integers(0, 1 << 14, 200).astype(dt)[rng.integers(0, 200, n)]
    if kind == "bell":    # densities that differ from bin to bin: at level 12 the optimiser keeps a table of 2^12 states
        return (rng.standard_normal(n) * 200 + 100000).astype(dt)
    if kind == "four":
        return rng.integers(0, 1 << 14, 4).astype(dt)[rng.integers(0, 4, n)]
    if kind == "noise":   # every bit random: under a delta encoding the encoder falls back to the uncompressed-equivalent chunk
        return rng.integers(0, 1 << 63, n, dtype=np.uint64).astype(dt) * np.uint64(2) + rng.integers(0, 2, n).astype(dt)
    if kind == "quant":   # float32 with 13 low mantissa bits of zeros
        return (((rng.standard_normal(n) * 100).astype(np.float32)).view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    if dt.kind == "f":
        return (rng.standard_normal(n) * 100).astype(np.float32).astype(dt)
    return rng.integers(0, min(1 << (8 * dt.itemsize - 1), 1 << 20), n).astype(dt)


SIZES = [1, 255, 256, 257, 3000]
OWN = {
    "classic u32, 65 chunks": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), [("uint32", SIZES[i % 5], "bell", i) for i in range(65)]),
    "level 12 u32, 1 chunk, a table beyond the LDS budget": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP, level=12), [("uint32", 8192, "bell")]),
    "int mult i32, 2 chunks": (dict(mode=G.MODE_TRY_INT_MULT, mode_u64=7, delta=G.DELTA_NOOP), [("int32", 3000, "mult"), ("int32", 257, "mult")]),
    "float mult f32 + consecutive 1, 3 chunks": (dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1),
                                                 [("float32", 255, "mult"), ("float32", 3000, "mult"), ("float32", 1, "mult")]),
    "float quant f32": (dict(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=13, delta=G.DELTA_NOOP), [("float32", 3000, "quant"), ("float32", 256, "quant")]),
    "consecutive 7 i16": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7), [("int16", 3000, "smooth"), ("int16", 257, "smooth"), ("int16", 255, "smooth")]),
    "consecutive 1 u64, one fallback chunk": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), [("uint64", 3000, "smooth"), ("uint64", 600, "noise"), ("uint64", 256, "smooth")]),
    "lookback i64": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK), [("int64", 3000, "periodic"), ("int64", 1000, "periodic")]),
    "lookback u8": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK), [("uint8", 3000, "periodic"), ("uint8", 257, "periodic")]),
    "dict u64 + consecutive 1": (dict(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1, dict=True), [("uint64", 3000, "few"), ("uint64", 256, "few")]),
    "dict i16": (dict(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True), [("int16", 3000, "few")]),
    "conv1 i32": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=3, conv1=True), [("int32", 3000, "smooth"), ("int32", 255, "smooth")]),
    "classic f16": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), [("float16", 3000, "random"), ("float16", 1, "random")]),
    "classic f64, a constant chunk with a page of 0 bytes": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), [("float64", 500, "constant"), ("float64", 300, "random")]),
    "classic i8": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), [("int8", 3000, "periodic"), ("int8", 256, "periodic")]),
    "four values u32, 3 chunks of 300": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), [("uint32", 300, "four", 1), ("uint32", 300, "four", 2), ("uint32", 300, "four", 3)]),
}
OWN_NAMES = list(OWN)
F65, F3 = OWN_NAMES[0], OWN_NAMES[-1]

OwnFile = namedtuple("OwnFile", "name data hdr offsets ns dtype arrays aux")
_own = {}


def own_file(L, name):
    """The file, and the compactor's offsets: chunk k at data[offsets[k] : offsets[k + 1]], the terminator at offsets[-1]."""
    if name in _own:
        return _own[name]
    import torch
    kw, rows = OWN[name]
    arrays = [numbers(*r) for r in rows]
    st = U.Staged(L, arrays)
    tasks = st.enc_tasks()
    cfg = G.make_config(enable_8_bit=True, **kw)
    res = np.zeros(st.k, U.RES_DT)
    G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(cfg), U.ptr(res), st.d_res.data_ptr(), None))
    assert (res["status"] == 0).all()
    buf = (C.c_uint8 * 64)()
    header = bytes(buf[: L.pco_gfx_write_standalone_header(buf, 64, sum(a.size for a in arrays), int(st.dtb[0]))])
    cap = len(header) + int(res["n_out"].sum())
    blob = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(st.k + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    G.check(L.pco_gfx_compact_chunks(st.k, U.ptr(tasks), st.d_res.data_ptr(), blob.data_ptr(), cap, len(header), offs.data_ptr(), None, None))
    torch.cuda.synchronize()
    offsets = [int(x) for x in offs.cpu().numpy()]
    assert offsets[0] == len(header) and offsets[-1] == cap
    data = header + blob.cpu().numpy()[len(header): cap].tobytes() + b"\0"
    _own[name] = OwnFile(name, data, len(header), offsets, [a.size for a in arrays], int(st.dtb[0]), arrays, [int(a) for a in res["aux"]])
    return _own[name]


_own_scan = {}


def own_scans(L):
    """every file written here in ONE scan call (mixed number types), kept"""
    if not _own_scan:
        files = [own_file(L, n) for n in OWN_NAMES]
        s = Streams([f.data for f in files])
        rows = [Row(i, 0, f.dtype, len(f.ns) + 3, HEADER, f.hdr) for i, f in enumerate(files)]
        for f, g in zip(files, scan(L, s, rows)):
            _own_scan[f.name] = g
        assert s.unchanged()
    return _own_scan


def test_the_files_cover_what_the_module_says(L):
    files = [own_file(L, n) for n in OWN_NAMES]
    assert sorted({len(f.ns) for f in files} & {1, 2, 3, 65}) == [1, 2, 3, 65]
    assert {n for f in files for n in f.ns} >= set(SIZES)
    assert {f.dtype for f in files} >= {1, 2, 3, 4, 5, 6, 8, 9, 10, 11}
    modes, deltas = set(), set()
    for f in files:
        ci, _ = O.inspect_first_chunk(f.data)
        modes.add(int(ci.mode_kind)); deltas.add((int(ci.delta_kind), int(ci.delta_order) if ci.delta_kind == 1 else 0))
    assert modes == {0, 1, 2, 3, 4} and deltas >= {(0, 0), (1, 1), (1, 7), (2, 0), (3, 0)}, (modes, deltas)
    f = own_file(L, OWN_NAMES[1]); ci, _ = O.inspect_first_chunk(f.data, max_bins=1 << 14)
    a, nb = int(ci.ans_size_log[1]), int(ci.n_bins[1])
    assert (4 << a) + (nb * 4 + 7) // 8 * 8 + (nb + 7) // 8 * 8 + ((nb + 1) * 4 + 7) // 8 * 8 > LDS_TABLE_BUDGET, "the level-12 table fits the LDS budget"
    f = own_file(L, "classic f64, a constant chunk with a page of 0 bytes")
    ci, _ = O.inspect_first_chunk(f.data)
    assert int(ci.meta_end_byte) == f.offsets[1], "the constant chunk's page has bytes"
    assert own_file(L, "consecutive 1 u64, one fallback chunk").aux[1] & 1, "the noise chunk did not fall back"
    assert len(own_file(L, F3).data) < 600


@pytest.mark.parametrize("name", OWN_NAMES)
def test_the_scan_finds_the_compactor_s_offsets(L, name):
    f = own_file(L, name); g = own_scans(L)[name]
    assert g.status == OK and g.n_out == len(f.ns)
    assert list(g.offsets) == f.offsets, "the offsets are the compactor's"
    assert list(g.counts) == f.ns
    assert g.aux == 2 | (4 << 8) and g.consumed == len(f.data) == f.offsets[-1] + 1   # the terminator was taken


# ---------------------------------------------------------------------------------------------------------------------------------------
# foreign streams: the reference's golden files and the test-only generator's
# ---------------------------------------------------------------------------------------------------------------------------------------
def generator_streams():
    few = numbers("uint32", 700, "few")
    return {
        "three variables: int mult under lookback with a delta'd secondary": O.test_encode(numbers("int32", 900, "mult"), chunks=[600, 300], mode=O.MODE_TRY_INT_MULT, mode_u64=7,
                                                                                           delta=O.TE_DELTA_LOOKBACK, window_n_log=10, state_n_log=0, secondary_uses_delta=True, lookback_seed=5),
        "three variables: float mult under lookback, a state of 2": O.test_encode(numbers("float32", 700, "mult"), mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_LOOKBACK,
                                                                                  window_n_log=8, state_n_log=1, lookback_seed=3),
        "a foreign table of 300 bins": O.test_encode(numbers("uint32", 4000, "bell"), chunks=[3000, 1000], tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_n_bins=300, tbl_seed=3),
        "ans_size_log 14, random weights": O.test_encode(numbers("uint32", 4000, "bell"), tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_RANDOM, tbl_seed=12),
        "ans_size_log 14, 16384 bins of weight 1": O.test_encode(numbers("uint32", 3000, "bell"), tbl_vars=O.TBL_PRIMARY, tbl_n_bins=16384, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_ONES,
                                                                 tbl_seed=3),
        "dict u32 under lookback": O.test_encode(few, mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1, lookback_seed=5),
        "dict + conv1 u32": O.test_encode(few, chunks=[400, 300], mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_CONV1, quantization=2, bias=1, weights=[2, 2]),
    }


GENERATED = ["three variables: int mult under lookback with a delta'd secondary", "three variables: float mult under lookback, a state of 2", "a foreign table of 300 bins",
             "ans_size_log 14, random weights", "ans_size_log 14, 16384 bins of weight 1", "dict u32 under lookback", "dict + conv1 u32"]
FOREIGN = ["asset " + os.path.basename(p) for p in ASSETS] + GENERATED
_foreign = {}


def foreign(name):
    if not _foreign:
        for p in ASSETS:
            _foreign["asset " + os.path.basename(p)] = open(p, "rb").read()
        _foreign.update(generator_streams())
        assert sorted(_foreign) == sorted(FOREIGN)
    return _foreign[name]


def dtype_of(f):
    hdr, _ = file_header(f)
    return f[hdr] or 1


def test_there_are_13_golden_files():
    assert len(ASSETS) == 13


@pytest.mark.parametrize("name", FOREIGN)
def test_a_foreign_stream_scans_as_the_chain_decodes_it(L, name):
    f = foreign(name)
    hdr, major = file_header(f)
    s = Streams([f])
    rows = [Row(0, 0, dtype_of(f), 8, HEADER, hdr, major)]
    if major != 0:   # its chunks without the header, the version in flags (which cannot say 0: that is "the current one")
        rows.append(Row(0, hdr, dtype_of(f), 8, major << 8))
    got = scan(L, s, rows)
    want = chain(L, s, rows, 1 << 24, lockstep=False)
    assert got == want
    assert got[0].status == OK and got[0].aux == 2 | (major << 8) and got[0].consumed == len(f), "a golden file scans to its end"
    if major != 0:
        assert got[1].offsets == tuple(o - hdr for o in got[0].offsets) and got[1].counts == got[0].counts
    if f[hdr] != 0:
        ci, _ = O.inspect_first_chunk(f, max_bins=1 << 14)
        assert got[0].counts[0] == int(ci.n) and got[0].offsets[0] == hdr and got[0].offsets[1] >= int(ci.meta_end_byte)
        assert sum(got[0].counts) == O.simple_decompress(f, G.DTYPE_NAME[dtype_of(f)]).size   # the reference's reader finds as many numbers
    else:
        assert got[0].n_out == 0 and got[0].offsets == (hdr,)


# ---------------------------------------------------------------------------------------------------------------------------------------
# truncation and damage: one 3-chunk u32 file of a few hundred bytes
# ---------------------------------------------------------------------------------------------------------------------------------------
def compare_with_the_chain(L, datas, hdr, dtype=1, allowed=()):
    """every stream as a file in ONE scan call against the lockstep chain; returns the rows compared"""
    s = Streams(datas)
    rows = [Row(i, 0, dtype, 5, HEADER, hdr) for i in range(len(datas))]
    got = scan(L, s, rows)
    want = chain(L, s, rows, 512, lockstep=True)
    compared = 0
    for i, (g, w) in enumerate(strip_version_of_refused_headers(got, want, rows, s)):
        if i in allowed:
            continue
        assert g == w, (i, len(datas[i]), g, w)
        compared += 1
    assert s.unchanged()
    return compared, got, want


def test_a_file_cut_after_every_byte_scans_as_the_chain_decodes_it(L):
    f = own_file(L, F3)
    cuts = [f.data[:k] for k in range(len(f.data) + 1)]
    compared, got, want = compare_with_the_chain(L, cuts, f.hdr)
    assert compared == len(f.data) + 1
    # what the cuts are expected to show, from the compactor's offsets alone
    for k, g in enumerate(got):
        whole = sum(1 for e in f.offsets[1:] if e <= k)
        if k < f.hdr:
            assert (g.n_out, g.status, g.offsets) == (0, INSUFFICIENT, (0,)), k
        elif k == len(f.data):
            assert (g.n_out, g.status, g.aux & 3, g.consumed) == (3, OK, 2, k)
        elif k == f.offsets[1]:   # the file ends right behind its first chunk: the chain's header step wants a terminator or a chunk
            assert (g.n_out, g.status, g.offsets) == (0, INSUFFICIENT, (f.hdr,)), k
        elif k in f.offsets[2:]:  # ... behind a later chunk it simply ends
            assert (g.n_out, g.status, g.aux & 3, g.consumed) == (whole, OK, 0, k), k
        else:
            assert (g.n_out, g.status, g.offsets) == (whole, INSUFFICIENT, tuple(f.offsets[: whole + 1])), k


def meta_len_of(L, chunk, dt):
    n, ml, pl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    G.check(L.pco_gfx_standalone_chunk_split((C.c_uint8 * len(chunk)).from_buffer_copy(chunk), len(chunk), dt, 4, C.byref(n), C.byref(ml), C.byref(pl)))
    return ml.value


def dict_file_with_one_index_out_of_range():
    """a Dict file of the generator's (no delta) whose first bin's lower is moved far beyond the dictionary: the framing is what it was"""
    f = bytearray(O.test_encode(numbers("uint32", 300, "four"), mode=O.MODE_TRY_DICT))
    hdr, _ = file_header(f)
    meta = hdr + 4
    v = int.from_bytes(f[meta: meta + 4], "little")
    assert v & 15 == 4
    dict_n = (v >> 4) & ((1 << 25) - 1)
    bit = 32 + dict_n * 32               # behind the dictionary: delta variant (4 bits), ans_size_log (4), n_bins (15), then bin 0: weight - 1, lower (32 bits), offset bits
    word = int.from_bytes(f[meta + bit // 8: meta + bit // 8 + 16], "little")
    assert word & 15 == 0, "the generator wrote a delta encoding"
    asl = (word >> 4) & 15
    at = 4 + 4 + 15 + asl
    word |= 0x7FFF0000 << at
    f[meta + bit // 8: meta + bit // 8 + 16] = word.to_bytes(16, "little")
    return bytes(f), hdr


def test_a_file_with_one_byte_flipped_scans_as_the_chain_decodes_it(L):
    f = own_file(L, F3)
    damaged = []
    for k in range(3):
        c0 = f.offsets[k]
        ml = meta_len_of(L, f.data[c0: f.offsets[k + 1]], 1)
        for at in list(range(c0 + 4, c0 + 4 + ml)) + list(range(c0 + 4 + ml, min(c0 + 4 + ml + 8, f.offsets[k + 1]))):   # the ChunkMeta, and the page's head: its tANS states and first symbols
            for x in (0x01, 0x10, 0x80, 0xFF):
                d = bytearray(f.data); d[at] ^= x
                damaged.append(bytes(d))
    assert len(damaged) > 150
    compared, got, want = compare_with_the_chain(L, damaged, f.hdr)
    assert compared == len(damaged)
    assert {g.status for g in got} >= {OK, CORRUPTION, INSUFFICIENT} and {g.n_out for g in got} == {0, 1, 2, 3}
    # the one exception the header lists, used by the one row built for it
    bad, hdr = dict_file_with_one_index_out_of_range()
    with pytest.raises(O.OracleError):
        O.simple_decompress(bad, "uint32")
    good = O.test_encode(numbers("uint32", 300, "four"), mode=O.MODE_TRY_DICT)
    compared, got, want = compare_with_the_chain(L, [good, bad], hdr, allowed=(1,))
    assert compared == 1 and got[0].status == OK
    assert want[1].status == CORRUPTION and want[1].n_out == 0, "the chain decodes the rows and finds the index"
    assert got[1] == got[0], "the scan reports the boundary the framing gives"


# ---------------------------------------------------------------------------------------------------------------------------------------
# max_chunks, batching
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_chunks", [1, 64, 65])
def test_a_scan_stopped_at_max_chunks_continues_from_consumed(L, max_chunks):
    f = own_file(L, F65); whole = own_scans(L)[F65]
    s = Streams([f.data])
    at, offsets, counts, calls = 0, [], [], 0
    while True:
        (g,) = scan(L, s, [Row(0, at, 1, max_chunks, HEADER if at == 0 else 4 << 8, f.hdr)])
        calls += 1
        assert g.status == OK and g.aux >> 8 == 4
        offsets += [at + o for o in g.offsets[:-1]]; counts += g.counts
        end = at + g.offsets[-1]; at += g.consumed
        if not (g.aux & 1):
            assert g.aux & 2 and at == end + 1
            break
        assert g.n_out == max_chunks and at == end and not (g.aux & 2)
    assert offsets + [end] == list(whole.offsets) and counts == list(whole.counts) and at == whole.consumed
    assert calls == (65 + max_chunks - 1) // max_chunks


def batch_of_64(L):
    good = [own_file(L, n) for n in OWN_NAMES[1:]]
    datas = [(f.data, f.dtype, f.hdr) for f in good]
    datas += [(foreign(n), dtype_of(foreign(n)), file_header(foreign(n))[0]) for n in FOREIGN]
    for f in good:   # further different files: the same chunks without the terminator, and without their last chunk either
        datas.append((f.data[:-1], f.dtype, f.hdr))
        if len(f.ns) > 1:
            datas.append((f.data[: f.offsets[-2]], f.dtype, f.hdr))
    assert len(datas) >= 61
    f3 = own_file(L, F3)
    bad = bytearray(f3.data); bad[f3.offsets[1] + 4] ^= 0x0F   # an unknown mode in the second chunk's ChunkMeta
    datas = datas[:61]
    for slot in (0, 31, 63):
        datas.insert(slot, (bytes(bad), 1, f3.hdr))
    assert len(datas) == 64 and len({d[0] for d in datas}) == 62
    return datas


@pytest.mark.parametrize("form", ["sync", "async"])
def test_64_files_in_one_call_scan_as_each_alone(L, form):
    import torch
    datas = batch_of_64(L)
    s = Streams([d[0] for d in datas])
    rows = [Row(i, 0, d[1], 70, HEADER, d[2]) for i, d in enumerate(datas)]
    assert len({r.dtype for r in rows}) >= 8
    stream = torch.cuda.Stream() if form == "async" else None
    together = scan(L, s, rows, form, stream)
    alone = [scan(L, s, [r], form, stream)[0] for r in rows]
    assert together == alone
    for slot in (0, 31, 63):
        assert (together[slot].status, together[slot].n_out) == (CORRUPTION, 1)
    assert sum(1 for g in together if g.status == OK) >= 40 and s.unchanged()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pipeline: scan -> index -> segment reads on one stream, one synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_scan_index_and_segment_reads_in_one_stream_s_order(L):
    import torch
    from pcodec_amd import paged, standalone
    f = own_file(L, "classic u32, 65 chunks")
    ns, k = f.ns, len(f.ns)
    s = Streams([f.data])
    stream = torch.cuda.Stream()
    every = 256
    n_cur = [(n - 1) // every for n in ns]
    cursors = torch.zeros(max(sum(n_cur), 1) * 256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(sum(ns) * 4 + 64, dtype=torch.uint8, device="cuda")
    it = np.zeros(k, DIRINDEX_DT); c_at = np.concatenate([[0], np.cumsum(n_cur)])
    for c in range(k):
        it[c] = (cursors.data_ptr() + 256 * int(c_at[c]) if n_cur[c] else 0, ns[c], every, c, c, 1, 4, 0, 0)
    segs = [(c, first) for c in range(k) for first in range(0, ns[c], every)]
    rt = np.zeros(len(segs), DIRREAD_DT); row_at = np.concatenate([[0], np.cumsum(ns)])
    for j, (c, first) in enumerate(segs):
        sidx = first // every
        rt[j] = (out.data_ptr() + 4 * (int(row_at[c]) + first), ns[c], first, min(every, ns[c] - first), c, c, 1, 4,
                 cursors.data_ptr() + 256 * (int(c_at[c]) + sidx - 1) if sidx else 0, 0, 0, 0)
    d_ires = torch.zeros(k * 3, dtype=torch.int64, device="cuda"); d_rres = torch.zeros(len(segs) * 3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()   # (the buffers above were made on the default stream; nothing of the pipeline below synchronises)
    kept = {}
    scan(L, s, [Row(0, 0, 1, k, HEADER, f.hdr)], "async", stream, keep=kept)
    assert kept["code"] == G.PcoSuccess
    d = G.Directory(s.ptr(0), len(f.data), kept["d_off"].data_ptr() + 8, k, 0, 0)   # (the scan's offsets, behind the area's leading canary)
    G.check(L.pco_gfx_index_chunks_dir(k, U.ptr(it), C.addressof(d), 0, None, d_ires.data_ptr(), stream.cuda_stream))
    G.check(L.pco_gfx_decompress_chunk_reads_dir(len(segs), U.ptr(rt), C.addressof(d), 0, None, d_rres.data_ptr(), stream.cuda_stream))
    stream.synchronize()   # the one synchronisation
    ires = d_ires.cpu().numpy().view(U.RES_DT); rres = d_rres.cpu().numpy().view(U.RES_DT)
    assert (ires["status"] == 0).all() and (rres["status"] == 0).all()
    assert [int(x) for x in ires["n_out"]] == n_cur
    got = out.cpu().numpy()[: sum(ns) * 4].view(np.uint32)
    want = np.concatenate(f.arrays)
    assert np.array_equal(got, want)
    assert np.array_equal(standalone.simple_decompress(f.data), want)
    (t,) = paged.decompress_files([f.data], "uint32")
    assert np.array_equal(t.cpu().numpy(), want)
    # several files of different types, from bytes and from a device tensor
    names = ["lookback i64", "classic f16", "dict u64 + consecutive 1"]
    files = [own_file(L, n) for n in names]
    blobs = [files[0].data, torch.from_numpy(np.frombuffer(files[1].data, np.uint8).copy()).cuda(), files[2].data]
    outs = paged.decompress_files(blobs, ["int64", "float16", "uint64"])
    for t, ff in zip(outs, files):
        assert U.bits_equal(t.cpu().numpy(), np.concatenate(ff.arrays))
    sc = paged.scan_files(blobs, ["int64", "float16", "uint64"])
    assert [(x.n_chunks, x.version, x.ns, x.consumed) for x in sc] == [(len(ff.ns), 4, ff.ns, len(ff.data)) for ff in files]
    assert [[int(o) for o in x.offsets.cpu().numpy()] for x in sc] == [ff.offsets for ff in files]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the work
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_work_is_one_scan_kernel(L):
    import torch
    files = [own_file(L, n) for n in OWN_NAMES]
    s = Streams([f.data for f in files])
    rows = [Row(i, 0, f.dtype, len(f.ns) + 3, HEADER, f.hdr) for i, f in enumerate(files)]
    for form in ("sync", "async"):
        scan(L, s, rows, form)   # (untimed: the workspace grows here)
        torch.cuda.synchronize()
        L.pco_gfx_profile_begin()
        got = scan(L, s, rows, form)   # (its canary comparison: nothing but the two arrays' named entries was written)
        assert U.profile_launches(L) == ["pco_scan_kernel"]
        assert [g.n_out for g in got] == [len(f.ns) for f in files] and s.unchanged()
