"""-m gpu: pco_gfx_decompress_chunks_dir / pco_gfx_decompress_chunk_reads_dir / pco_gfx_index_chunks_dir (include/pco_gfx.h section 4l) -- STANDALONE
chunks decoded, read in slices and indexed from the directory pco_gfx_compact_chunks leaves in DEVICE memory, and pcodec_amd.paged over them.

Truth is one of two things: the input array, or the POINTER form (pco_gfx_decompress_pages, pco_gfx_decompress_page_reads_hist,
pco_gfx_index_pages_hist: code from before these entry points) given the four values pco_gfx_standalone_chunk_split finds in the chunk's bytes on
the host.  That split is code these entry points came with, so the pointer form is no independent witness of it: a split wrong in a way both forms
agree on is caught by the comparison with the INPUT here, and the split itself is held against the oracle's wrapped writer, chunk by chunk, in
tests/test_chunk_directory_abi.py.  Every output of a call -- dst, `to` cursors, histories, cursor slots -- lies in ONE device area between canary bytes; the pointer form
runs on a second area of the same layout, and the two areas are compared WHOLE, so a refused task that wrote a byte or a cursor that differs in one
bit fails.  The task array and the directory are overwritten as each _dir call returns.

Shapes: classic chunks of 1, 255, 256, 257, 1000 and 2049 numbers and one chunk per number width, a constant chunk and an incompressible one in ONE
call; one chunk or two per other mode and delta family (2049 / 1000 numbers); one level-12 chunk of 2^13 numbers, whose tables leave the walkers' LDS;
one Lookback i64 chunk of 4096 numbers.  Gap 0 is the compactor's own stream (behind 11 bytes of a caller's header); gap 4 a stream of the same chunks
assembled on the host with 4 bytes of framing in front of each.  Damaged directories are refused by verdict: nothing here runs into a fault.

Measured on an MI355X: 542 tests in 4 to 10 s, the encodes of the ten specs (1.7 s, once) included.  Which rows the five named wrong variants of
pco_chunk_dir.h fail is recorded in DESIGN.md section 2."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY, PAD, FLAG, TAIL, ALL_ONES, HDR = 0xA5, 64, 1, 24, (1 << 64) - 1, 11
_u8, _u4 = "<u8", "<u4"
READ_DT = np.dtype([("meta", _u8), ("meta_len", _u8), ("page", _u8), ("page_len", _u8), ("dst", _u8), ("page_n", _u8), ("first", _u8), ("count", _u8), ("dtype", _u4),
                    ("format_major", _u4), ("from", _u8), ("to", _u8), ("history", _u8), ("history_len", _u8)])
INDEX_DT = np.dtype([("meta", _u8), ("meta_len", _u8), ("page", _u8), ("page_len", _u8), ("cursors", _u8), ("page_n", _u8), ("every_rows", _u8), ("dtype", _u4),
                     ("format_major", _u4), ("histories", _u8), ("history_stride", _u8)])
DIRPAGE_DT = np.dtype([("dst", _u8), ("page_n", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4)])
DIRREAD_DT = np.dtype([("dst", _u8), ("page_n", _u8), ("first", _u8), ("count", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4),
                       ("from", _u8), ("to", _u8), ("history", _u8), ("history_len", _u8)])
DIRINDEX_DT = np.dtype([("cursors", _u8), ("page_n", _u8), ("every_rows", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4),
                        ("histories", _u8), ("history_stride", _u8)])
assert (READ_DT.itemsize, INDEX_DT.itemsize, DIRPAGE_DT.itemsize, DIRREAD_DT.itemsize, DIRINDEX_DT.itemsize) == (104, 80, 32, 80, 56)


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


# ---------------------------------------------------------------------------------------------------------------------------------------
# the chunks: one encode call per spec, one stream per (spec, gap)
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
        return (rng.integers(0, 1 << 20, 37)[np.arange(n) % 37] + rng.integers(0, 3, n)).astype(dt)
    if kind == "few":
        return rng.integers(0, 1 << 14, 200).astype(dt)[rng.integers(0, 200, n)]
    if kind == "noise":   # every bit random: under a delta encoding the encoder falls back to the uncompressed-equivalent chunk
        return rng.integers(0, 1 << 63, n, dtype=np.uint64).astype(dt) * np.uint64(2) + rng.integers(0, 2, n).astype(dt)
    if kind == "quant":   # float32 with 13 low mantissa bits of zeros
        return (((rng.standard_normal(n) * 100).astype(np.float32)).view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)
    if dt.kind == "f":
        return (rng.standard_normal(n) * 100).astype(np.float32).astype(dt)
    return rng.integers(0, min(1 << (8 * dt.itemsize - 1), 1 << 20), n).astype(dt)


SPECS = {
    "classic": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP),
                [("uint32", 1, "random"), ("uint32", 255, "random"), ("uint32", 2049, "random"), ("uint32", 256, "random"), ("uint32", 257, "random"), ("int64", 300, "random"),
                 ("float32", 300, "random"), ("uint16", 300, "random"), ("float16", 300, "random"), ("uint8", 300, "random"), ("float64", 300, "random"),
                 ("uint32", 500, "constant"), ("uint32", 1000, "random")]),
    "consecutive1": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), [("int32", 2049, "smooth"), ("uint64", 1000, "smooth"), ("uint64", 600, "noise")]),
    "consecutive7": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7), [("int16", 2049, "smooth")]),
    "lookback": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK), [("int64", 4096, "periodic"), ("uint32", 2049, "periodic"), ("int64", 1000, "periodic")]),
    "int_mult": (dict(mode=G.MODE_TRY_INT_MULT, mode_u64=7, delta=G.DELTA_NOOP), [("int32", 1000, "mult")]),
    "float_mult": (dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), [("float32", 2049, "mult")]),
    "float_quant": (dict(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=13, delta=G.DELTA_NOOP), [("float32", 1000, "quant")]),
    "dict": (dict(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1, dict=True), [("uint64", 2049, "few"), ("int16", 1000, "few")]),
    "conv1": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=3, conv1=True), [("int32", 2049, "smooth")]),
    "level12": (dict(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP, level=12), [("uint32", 1 << 13, "random")]),
}
ALL_SPECS = sorted(SPECS)
MODE_KIND = {"classic": 0, "consecutive1": 0, "consecutive7": 0, "lookback": 0, "int_mult": 1, "float_mult": 2, "float_quant": 3, "dict": 4, "conv1": 0, "level12": 0}
DELTA_KIND = {"classic": 0, "consecutive1": 1, "consecutive7": 1, "lookback": 2, "int_mult": 0, "float_mult": 1, "float_quant": 0, "dict": 1, "conv1": 3, "level12": 0}


def split(L, chunk, dt):
    """(n, meta_len, page_len) of a chunk's bytes on the host"""
    n, ml, pl = C.c_uint64(), C.c_uint64(), C.c_uint64()
    buf = (C.c_uint8 * len(chunk)).from_buffer_copy(chunk)
    G.check(L.pco_gfx_standalone_chunk_split(buf, len(chunk), dt, 4, C.byref(n), C.byref(ml), C.byref(pl)))
    return n.value, ml.value, pl.value


class Encoded:
    def __init__(self, L, spec):
        kw, rows = SPECS[spec]
        self.L, self.spec = L, spec
        self.arrays = [numbers(*r) for r in rows]
        self.st = st = U.Staged(L, self.arrays)
        self.k, self.dtb = st.k, [int(d) for d in st.dtb]
        self.tasks = st.enc_tasks()
        self.cfg = G.make_config(enable_8_bit=True, **kw)
        self.res = np.zeros(st.k, U.RES_DT)
        G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(self.tasks), C.byref(self.cfg), U.ptr(self.res), st.d_res.data_ptr(), None))
        assert (self.res["status"] == 0).all()
        self.chunks = st.slot_bytes(self.res["n_out"])
        self.splits = [split(L, c, d) for c, d in zip(self.chunks, self.dtb)]
        assert [s[0] for s in self.splits] == [a.size for a in self.arrays]
        info = G.ChunkMetaInfo(); m = self.chunks[0][4: 4 + self.splits[0][1]]
        G.check(L.pco_gfx_chunk_meta_info((C.c_uint8 * len(m)).from_buffer_copy(m), len(m), self.dtb[0], 4, C.byref(info)))
        assert info.mode_kind == MODE_KIND[spec] and (spec == "dict" or info.delta_kind == DELTA_KIND[spec]), "the spec was not taken"   # (Dict: the accessor stops at the kind)


class Blob:
    """The chunks of an Encoded as one stream: gap 0 -- pco_gfx_compact_chunks' own, behind HDR bytes; gap 4 -- assembled on the host.  blob_len is the
    stream's end; 64 more bytes are readable."""

    def __init__(self, e, gap):
        import torch
        self.e, self.gap, L = e, gap, e.L
        if gap == 0:
            self.cap = HDR + int(e.res["n_out"].sum())
            self.blob = torch.full((self.cap + 64,), 0xC3, dtype=torch.uint8, device="cuda")
            self.offs = torch.full((e.k + 1,), 0x1111111111111111, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            G.check(L.pco_gfx_compact_chunks(e.k, U.ptr(e.tasks), e.st.d_res.data_ptr(), self.blob.data_ptr(), self.cap, HDR, self.offs.data_ptr(), None, None))
            torch.cuda.synchronize()
        else:
            host = b"".join(b"\xDD" * gap + c for c in e.chunks)
            self.cap = len(host)
            self.blob = torch.from_numpy(np.frombuffer(host + b"\xC3" * 64, np.uint8).copy()).cuda()
            self.offs = torch.from_numpy(np.concatenate([[0], np.cumsum([gap + len(c) for c in e.chunks])]).astype(np.int64)).cuda()
        self.true = self.offs.cpu().numpy().view(np.uint64).copy()
        assert int(self.true[-1]) == self.cap and [int(x) for x in np.diff(self.true.astype(np.int64))] == [gap + len(c) for c in e.chunks]

    def pointers(self, i):
        """(meta, meta_len, page, page_len) of chunk i, as the host found them"""
        n, ml, pl = self.e.splits[i]
        at = self.blob.data_ptr() + int(self.true[i]) + self.gap + 4
        return at, ml, at + ml, pl


_encoded, _blobs = {}, {}


def blob_of(L, spec, gap):
    if spec not in _encoded:
        _encoded[spec] = Encoded(L, spec)
    if (spec, gap) not in _blobs:
        _blobs[spec, gap] = Blob(_encoded[spec], gap)
    return _blobs[spec, gap]


def test_the_chunk_set_is_what_the_module_says(L):
    e = blob_of(L, "classic", 0).e
    assert sorted({a.size for a in e.arrays} & {1, 255, 256, 257, 1000, 2049}) == [1, 255, 256, 257, 1000, 2049]
    assert e.splits[11][2] == 0, "the constant chunk has a page of 0 bytes"
    assert blob_of(L, "consecutive1", 0).e.res["aux"][2] & 1, "the incompressible chunk fell back"   # (the delta's moments make it longer than the plain numbers)
    assert {a.dtype.itemsize for a in e.arrays} == {1, 2, 4, 8}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the harness: a layout of output extents, areas of it, the two forms of a call over the same task descriptions
# ---------------------------------------------------------------------------------------------------------------------------------------
class Layout:
    """Extents handed out side by side, PAD canary bytes around each; `first` = [(offset, bytes)] that an area starts with in place of canaries."""

    def __init__(self):
        self.size, self.first = PAD, []

    def take(self, nbytes, first=None):
        o = self.size
        self.size += (nbytes + 15) // 16 * 16 + PAD
        if first is not None:
            self.first.append((o, np.frombuffer(bytes(first), np.uint8)))
        return o

    def image(self):
        img = np.full(self.size, CANARY, np.uint8)
        for o, b in self.first:
            img[o: o + b.size] = b
        return img

    def areas(self, n=2):
        import torch
        img = self.image()
        out = [torch.from_numpy(img.copy()).cuda() for _ in range(n)]
        torch.cuda.synchronize()
        return out


class Source:
    """A Blob behind a directory that may be an edited copy: `offs` / `blob` (device tensors) and blob_len."""

    def __init__(self, b, offs=None, blob=None, blob_len=None):
        self.b, self.offs, self.blob, self.blob_len = b, b.offs if offs is None else offs, b.blob if blob is None else blob, b.cap if blob_len is None else blob_len

    def directory(self):
        return G.Directory(self.blob.data_ptr(), self.blob_len, self.offs.data_ptr(), self.b.e.k, self.b.gap, 0)


def kind_of(t):
    return "index" if "every" in t else ("read" if "first" in t else "page")


def records(src, tasks, base, pointer_form):
    kind = kind_of(tasks[0]); b = src.b
    dt = {"page": U.PAGE_DT if pointer_form else DIRPAGE_DT, "read": READ_DT if pointer_form else DIRREAD_DT, "index": INDEX_DT if pointer_form else DIRINDEX_DT}[kind]
    rec = np.zeros(len(tasks), dt)
    for r, t in zip(rec, tasks):
        i = t["i"]
        at = lambda key: (base + t[key + "_off"]) if t.get(key + "_off") is not None else (t.get(key + "_abs") or 0)   # noqa: E731
        if pointer_form:
            r["meta"], r["meta_len"], r["page"], r["page_len"] = b.pointers(i)
        else:
            r["meta_piece"] = r["page_piece"] = t.get("piece", i)
        r["page_n"], r["dtype"], r["format_major"] = b.e.arrays[i].size, b.e.dtb[i], 4
        if kind == "index":
            r["every_rows"], r["cursors"], r["histories"], r["history_stride"] = t["every"], at("cursors"), at("histories"), t.get("stride", 0)
        elif kind == "read":
            r["first"], r["count"], r["dst"], r["from"], r["to"], r["history"], r["history_len"] = t["first"], t["count"], at("dst"), at("from"), at("to"), at("history"), t.get("history_len", 0)
        else:
            r["dst"] = at("dst")
    return rec


def run(L, src, tasks, area, pointer_form, flags, form, subset=None, stream=None):
    """One call of either form over `tasks` (the pointer form over tasks[j] for j in `subset` alone): (code, last status, results as RES_DT of len(tasks))."""
    import torch
    kind = kind_of(tasks[0])
    js = list(range(len(tasks))) if subset is None else list(subset)
    rec = records(src, [tasks[j] for j in js], area.data_ptr(), pointer_form)
    d_res = torch.full((max(len(js), 1) * U.RES_DT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    host = np.zeros(len(js), U.RES_DT); host["status"] = 99
    torch.cuda.synchronize()
    res_arg = U.ptr(host) if form == "sync" else None
    sh = C.c_void_p(stream.cuda_stream) if stream is not None else None
    if pointer_form:
        if kind == "page":
            code = L.pco_gfx_decompress_pages(len(rec), U.ptr(rec), res_arg, d_res.data_ptr(), sh)
        else:
            code = (L.pco_gfx_index_pages_hist if kind == "index" else L.pco_gfx_decompress_page_reads_hist)(len(rec), U.ptr(rec), flags, res_arg, d_res.data_ptr(), sh)
        status = L.pco_gfx_last_status()
    else:
        d = src.directory()
        if kind == "page":
            code = L.pco_gfx_decompress_chunks_dir(len(rec), U.ptr(rec), C.addressof(d), res_arg, d_res.data_ptr(), sh)
        else:
            code = (L.pco_gfx_index_chunks_dir if kind == "index" else L.pco_gfx_decompress_chunk_reads_dir)(len(rec), U.ptr(rec), C.addressof(d), flags, res_arg, d_res.data_ptr(), sh)
        status = L.pco_gfx_last_status()
        rec[:] = 0; C.memset(C.addressof(d), 0, C.sizeof(d))   # (the library copied both: they may be overwritten as soon as the call returns)
    torch.cuda.synchronize()
    dev = d_res.cpu().numpy().view(U.RES_DT)[: len(js)].copy()
    if form == "sync":
        assert np.array_equal(dev, host), "the host results of a synchronous call are not its device results"
    out = np.zeros(len(tasks), U.RES_DT); out["status"] = 1000
    out[js] = dev
    return code, status, out


def tuples(res):
    return [(int(r["status"]), int(r["n_out"]), int(r["consumed"]), int(r["aux"])) for r in res]


def both(L, src, tasks, layout, flags, form, failing=None, areas=None, what=""):
    """The pointer form on area 0 (over the tasks the directory does not fail), the _dir form on area 1: results and whole areas equal; a task in
    `failing` = {j: status} answers {status, 0, 0, 0} and leaves every one of its extents as it was.  Returns (the areas, the results)."""
    failing = failing or {}
    a = areas or layout.areas()
    ok = [j for j in range(len(tasks)) if j not in failing]
    want = np.zeros(len(tasks), U.RES_DT)
    if ok:
        _, _, want = run(L, Source(src.b), tasks, a[0], True, flags, form, subset=ok)
    for j, st in failing.items():
        want[j] = (0, 0, st, 0)
    code, status, got = run(L, src, tasks, a[1], False, flags, form)
    assert tuples(got) == tuples(want), f"{what}: (status, n_out, consumed, aux) of the _dir form, then of the pointer form"
    bad = [j for j in range(len(tasks)) if want[j]["status"] != 0]
    if form == "sync":
        assert (code, status) == ((G.PcoSuccess, 0) if not bad else (G.PcoDecompressionError, int(want[bad[0]]["status"]))), (code, status)
    else:
        assert code == G.PcoSuccess
    h0, h1 = (x.cpu().numpy() for x in a[:2])
    if not np.array_equal(h0, h1):
        at = int(np.flatnonzero(h0 != h1)[0])
        owner = [j for j, t in enumerate(tasks) if any(o - PAD <= at < o + n + PAD for o, n in t["extents"])]
        raise AssertionError(f"{what}: the areas of the two forms differ in {int((h0 != h1).sum())} bytes, first at {at} (task {owner})")
    img = layout.image()
    for j in failing:
        for o, n in tasks[j]["extents"]:
            assert np.array_equal(h1[o - PAD: o + n + PAD], img[o - PAD: o + n + PAD]), f"{what}: the refused task {j} wrote into one of its extents"
    return a, got


def rows_equal_the_input(e, area, dst_of, what=""):
    """dst_of: [(chunk, first row, count, offset in the area)]"""
    host = area.cpu().numpy()
    for i, first, count, o in dst_of:
        want = e.arrays[i][first: first + count].view(np.uint8).reshape(-1)
        assert np.array_equal(host[o: o + want.size], want), f"{what}: rows {first}..{first + count} of chunk {i} differ from the input"


def window_bytes(L, e, i):
    return L.pco_gfx_lookback_history_bytes(L.pco_gfx_lookback_window_n_log(e.arrays[i].size), e.dtb[i])


def stride_of(L, e, i):
    return (window_bytes(L, e, i) + 7) // 8 * 8 + TAIL


MODES = [(0, False), (FLAG, False), (0, True), (FLAG, True)]
MODE_IDS = ["plain", "general", "hist", "general+hist"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. whole chunks
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_whole_chunks_are_the_pointer_form_s_and_the_input(L, spec, gap, form):
    b = blob_of(L, spec, gap); e = b.e; lay = Layout(); tasks = []; dst_of = []
    for i, a in enumerate(e.arrays):
        o = lay.take(a.nbytes)
        tasks.append(dict(i=i, dst_off=o, extents=[(o, a.nbytes)])); dst_of.append((i, 0, a.size, o))
    areas, res = both(L, Source(b), tasks, lay, 0, form, what=f"{spec} gap {gap}")
    assert tuples(res) == [(0, a.size, e.splits[i][2], 0) for i, a in enumerate(e.arrays)]   # consumed: the page's bytes
    rows_equal_the_input(e, areas[1], dst_of, f"{spec} gap {gap}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. row ranges: a read without cursors
# ---------------------------------------------------------------------------------------------------------------------------------------
def ranges_of(n):
    """empty, inside the first batch, across a batch boundary, the last row, the whole chunk (the sixth, count == 0 behind garbage pieces, is its own call)"""
    out = [(min(5, n), 0), (min(3, n - 1), min(7, n - min(3, n - 1)))]
    if n > 256:
        out.append((250, min(12, n - 250)))
    return out + [(n - 1, 1), (0, n)]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_row_ranges_are_the_pointer_form_s_and_the_input(L, spec, form):
    b = blob_of(L, spec, 0 if form == "sync" else 4); e = b.e; lay = Layout(); tasks = []; dst_of = []
    for i, a in enumerate(e.arrays):
        for first, count in ranges_of(a.size):
            o = lay.take(count * a.itemsize)
            tasks.append(dict(i=i, first=first, count=count, dst_off=o, extents=[(o, count * a.itemsize)])); dst_of.append((i, first, count, o))
    areas, res = both(L, Source(b), tasks, lay, 0, form, what=spec)
    assert [(r[0], r[1]) for r in tuples(res)] == [(0, t["count"]) for t in tasks]
    rows_equal_the_input(e, areas[1], dst_of, spec)


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("kind", ["read", "index"])
def test_a_task_without_rows_takes_no_verdict_and_reads_nothing(L, kind, form):
    """count == 0 / k == 0 behind a directory of garbage: the sentinel, descending offsets, a blob_len of 0"""
    import torch
    b = blob_of(L, "classic", 0); e = b.e; lay = Layout()
    garbage = torch.from_numpy(np.array([ALL_ONES - j for j in range(e.k + 1)], np.uint64).view(np.int64)).cuda()
    if kind == "read":
        tasks = [dict(i=i, first=min(3, a.size), count=0, extents=[]) for i, a in enumerate(e.arrays)]
    else:
        tasks = [dict(i=i, every=256, extents=[]) for i, a in enumerate(e.arrays) if a.size <= 256]   # k == 0
    a = lay.areas()
    code, status, res = run(L, Source(b, offs=garbage, blob_len=0), tasks, a[1], False, 0, form)
    assert code == G.PcoSuccess and tuples(res) == [(0, 0, 0, 0)] * len(tasks)
    assert np.array_equal(a[1].cpu().numpy(), lay.image())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. slices: a chain of reads, each from the `to` of the last
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_a_chain_of_slices_each_from_the_to_of_the_last(L, spec, flags, hist, form):
    """Slice s of every chunk in call s: from == to == the chunk's one cursor slot, its one history beside it.  Slices of 256 rows over gap 0 in the
    synchronous form, of 512 over gap 4 in the asynchronous one.  Cursors of every kind (1, 2, under the flag 3, beside a history 4) and the histories
    are compared with the pointer form's after every call."""
    gap = 0 if form == "sync" else 4
    b = blob_of(L, spec, gap); e = b.e; lay = Layout(); every = 512 if gap else 256
    if spec == "level12":
        every *= 4
    pages = []
    for i, a in enumerate(e.arrays):
        pg = dict(i=i, n=a.size, w=a.itemsize, dst=lay.take(a.nbytes), cur=lay.take(256))
        if hist:
            pg["stride"] = stride_of(L, e, i); pg["hist"] = lay.take(pg["stride"])
        pages.append(pg)
    areas = lay.areas()
    for s in range(max(-(-pg["n"] // every) for pg in pages)):
        tasks = []
        for pg in pages:
            row = s * every
            if row >= pg["n"]:
                continue
            count = min(every, pg["n"] - row)
            t = dict(i=pg["i"], first=row, count=count, dst_off=pg["dst"] + row * pg["w"], to_off=pg["cur"], from_off=pg["cur"] if s else None,
                     extents=[(pg["dst"] + row * pg["w"], count * pg["w"]), (pg["cur"], 256)])
            if hist:
                t["history_off"], t["history_len"] = pg["hist"], pg["stride"]; t["extents"].append((pg["hist"], pg["stride"]))
            tasks.append(t)
        _, res = both(L, Source(b), tasks, lay, flags, form, areas=areas, what=f"{spec} gap {gap} slice {s}")
        assert [r[0] for r in tuples(res)] == [0] * len(tasks), tuples(res)
    rows_equal_the_input(e, areas[1], [(pg["i"], 0, pg["n"], pg["dst"]) for pg in pages], f"{spec} gap {gap}")
    if hist and spec == "lookback":   # kind 4 beside a history; else the kinds the pointer form writes, which the areas' equality covers
        host = areas[1].cpu().numpy()
        assert any((host[pg["hist"]: pg["hist"] + 64] != CANARY).any() for pg in pages)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. indexes, and the segments decoded side by side from their pairs
# ---------------------------------------------------------------------------------------------------------------------------------------
def index_tasks(L, e, layout, every, hist):
    tasks = []
    for i, a in enumerate(e.arrays):
        k = max((a.size - 1) // every, 0)
        t = dict(i=i, every=every, k=k, extents=[])
        if k:
            t["cursors_off"] = layout.take(k * 256); t["extents"].append((t["cursors_off"], k * 256))
        if hist and k:
            t["stride"] = stride_of(L, e, i)
            t["histories_off"] = layout.take(k * t["stride"]); t["extents"].append((t["histories_off"], k * t["stride"]))
        tasks.append(t)
    return tasks


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("every", [256, 512])
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_the_index_is_the_pointer_form_s_byte_for_byte(L, spec, every, flags, hist, form):
    b = blob_of(L, spec, 0 if every == 256 else 4); e = b.e; lay = Layout()
    tasks = index_tasks(L, e, lay, every, hist)
    a, res = both(L, Source(b), tasks, lay, flags, form, what=f"{spec} every {every}")
    assert [(r[0], r[1]) for r in tuples(res)] == [(0, t["k"]) for t in tasks]
    if hist:   # the stride's tail is nobody's, and a chunk without Lookback leaves its histories alone altogether
        host = a[1].cpu().numpy(); stamped = 0
        for t in tasks:
            for s in range(t["k"]):
                o = t["histories_off"] + s * t["stride"]; used = window_bytes(L, e, t["i"]) if spec == "lookback" else 0
                assert (host[o + used: o + t["stride"]] == CANARY).all(), (t["i"], s)
                stamped += int((host[o: o + 64] != CANARY).any())
        assert (stamped > 0) == (spec == "lookback")


@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("gap,index_dir", [(0, True), (4, False)], ids=["gap0-index_dir", "gap4-segments_dir"])
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_segments_side_by_side_from_an_index_of_either_form(L, spec, gap, index_dir, flags, hist):
    """The index from the _dir form (asynchronous), its segments through the POINTER form; the index from the pointer form, its segments through the _dir
    form: cursors and histories are interchangeable, and either way the rows are the input's."""
    every = 512 if spec == "level12" else 256
    b = blob_of(L, spec, gap); e = b.e; ilay = Layout()
    itasks = index_tasks(L, e, ilay, every, hist)
    iarea = ilay.areas(1)[0]
    code, _, res = run(L, Source(b), itasks, iarea, not index_dir, flags, "async")
    assert code == G.PcoSuccess and [(r[0], r[1]) for r in tuples(res)] == [(0, t["k"]) for t in itasks]
    ihost = iarea.cpu().numpy().copy()
    lay = Layout(); tasks = []; dst_of = []
    for it in itasks:
        i = it["i"]; a = e.arrays[i]; o = lay.take(a.nbytes); dst_of.append((i, 0, a.size, o))
        for s, row in enumerate(range(0, a.size, every) if it["k"] else [0]):
            count = min(every, a.size - row) if it["k"] else a.size
            t = dict(i=i, first=row, count=count, dst_off=o + row * a.itemsize, extents=[(o + row * a.itemsize, count * a.itemsize)])
            if s:
                t["from_abs"] = iarea.data_ptr() + it["cursors_off"] + (s - 1) * 256
                if hist:
                    t["history_abs"], t["history_len"] = iarea.data_ptr() + it["histories_off"] + (s - 1) * it["stride"], it["stride"]
            tasks.append(t)
    area = lay.areas(1)[0]
    code, _, res = run(L, Source(b), tasks, area, index_dir, flags, "sync" if gap else "async")
    assert code == G.PcoSuccess and [(r[0], r[1]) for r in tuples(res)] == [(0, t["count"]) for t in tasks], tuples(res)
    rows_equal_the_input(e, area, dst_of, f"{spec} gap {gap}")
    assert np.array_equal(iarea.cpu().numpy(), ihost), "to == NULL leaves the index's pairs as they are"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. directory verdicts, edited into a device copy of d_offsets or of the blob
# ---------------------------------------------------------------------------------------------------------------------------------------
EDITS = ["sentinel", "swapped pair", "end beyond blob_len", "dropped chunk", "extent of 3 bytes", "wrong dtype byte", "terminator byte", "n off by one", "meta cut in its header",
         "meta cut in its bins", "unknown mode nibble", "unknown delta variant"]


def defective(b, edit):
    """(the Source with the defect, {chunk it fails: status}): offset edits hit the LAST chunk, blob edits chunk 2 -- the others are as they were"""
    import torch
    e = b.e; n = e.k; last = n - 1; mid = min(2, n - 1)
    o = b.true.copy(); blob = None; blob_len = None
    c0 = int(b.true[mid]) + b.gap
    if edit == "sentinel":
        o[n] = ALL_ONES; failing = {i: G.ST_INVALID_ARGUMENT for i in range(n)}
    elif edit == "swapped pair":
        o[n] = o[last] - np.uint64(1); failing = {last: G.ST_INVALID_ARGUMENT}
    elif edit == "end beyond blob_len":
        blob_len = b.cap - 1; failing = {last: G.ST_INVALID_ARGUMENT}
    elif edit == "dropped chunk":
        o[n] = o[last]; failing = {last: G.ST_INSUFFICIENT_DATA}
    elif edit == "extent of 3 bytes":
        o[n] = o[last] + np.uint64(b.gap + 3); failing = {last: G.ST_INSUFFICIENT_DATA}
    elif edit == "meta cut in its header":
        o[n] = o[last] + np.uint64(b.gap + 4 + 2); failing = {last: G.ST_INSUFFICIENT_DATA}
    elif edit == "meta cut in its bins":
        o[n] = o[last] + np.uint64(b.gap + 4 + e.splits[last][1] - 1); failing = {last: G.ST_INSUFFICIENT_DATA}
    else:
        host = b.blob.cpu().numpy().copy()
        if edit == "wrong dtype byte":
            host[c0] = 1 if host[c0] != 1 else 3; failing = {mid: G.ST_CORRUPTION}
        elif edit == "terminator byte":
            host[c0] = 0; failing = {mid: G.ST_CORRUPTION}
        elif edit == "n off by one":
            host[c0 + 1] ^= 1; failing = {mid: G.ST_INVALID_ARGUMENT}
        elif edit == "unknown mode nibble":
            host[c0 + 4] |= 0x0F; failing = {mid: G.ST_CORRUPTION}
        else:   # the variant nibble behind a Classic mode's: chunk 2 of both specs used here is Classic
            assert host[c0 + 4] & 0x0F == 0
            host[c0 + 4] |= 0xF0; failing = {mid: G.ST_CORRUPTION}
        blob = torch.from_numpy(host).cuda()
    return Source(b, offs=torch.from_numpy(o.view(np.int64).copy()).cuda(), blob=blob, blob_len=blob_len), failing


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("kind", ["page", "read", "index"])
@pytest.mark.parametrize("edit", EDITS)
@pytest.mark.parametrize("spec,gap", [("classic", 0), ("lookback", 4)])
def test_every_verdict_refuses_its_task_alone_and_leaves_its_extents(L, spec, gap, edit, kind, form):
    """A refused task answers {status, 0, 0, 0}; its dst, its `to` cursor, its history, its cursor slots and its histories stay canaries (the history and the
    `from` cursor start as VALID ones a run would update); its neighbours in the same call are the pointer form's."""
    b = blob_of(L, spec, gap); e = b.e
    src, failing = defective(b, edit)
    flags, hist = (FLAG, True)
    lay = Layout(); tasks = []
    if kind == "index":
        tasks = index_tasks(L, e, lay, 256, hist)
    else:
        # a `from` cursor and a history for the second half of every chunk of more than 512 rows, from the pointer form
        ilay = Layout(); itasks = index_tasks(L, e, ilay, 512, hist); iarea = ilay.areas(1)[0]
        code, _, _ = run(L, Source(b), itasks, iarea, True, flags, "sync")
        assert code == G.PcoSuccess
        ihost = iarea.cpu().numpy()
        for it in itasks:
            i = it["i"]; a = e.arrays[i]
            if kind == "page":
                o = lay.take(a.nbytes); tasks.append(dict(i=i, dst_off=o, extents=[(o, a.nbytes)]))
                continue
            first = 512 if it["k"] else 0
            o = lay.take((a.size - first) * a.itemsize)
            t = dict(i=i, first=first, count=a.size - first, dst_off=o, extents=[(o, (a.size - first) * a.itemsize)])
            t["to_off"] = lay.take(256); t["extents"].append((t["to_off"], 256))
            if it["k"]:
                t["from_abs"] = iarea.data_ptr() + it["cursors_off"]
                h = ihost[it["histories_off"]: it["histories_off"] + it["stride"]]
                t["history_off"], t["history_len"] = lay.take(it["stride"], h), it["stride"]; t["extents"].append((t["history_off"], it["stride"]))
            tasks.append(t)
    if kind == "index":   # (a chunk without cursors takes no verdict)
        failing = {j: st for j, st in failing.items() if tasks[j]["k"]}
    assert failing
    both(L, src, tasks, lay, flags if kind != "page" else 0, form, failing=failing, what=f"{spec} {edit} {kind}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the pipeline: compress -> compact -> decode on one stream, one synchronisation at its end
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_encode_compact_decode_is_one_stream_ordered_pipeline(L):
    """Chunk 2's dst_cap is too small for the encoder: it fails honestly, the compactor drops it, and its decode task answers INSUFFICIENT_DATA."""
    import torch
    arrays = [numbers("uint32", 1000, "random", s) for s in range(3)] + [numbers("int64", 2049, "smooth"), numbers("float32", 257, "mult")]
    st = U.Staged(L, arrays)
    caps = st.caps.copy(); caps[2] = 48
    tasks = st.enc_tasks(caps=caps)
    cfg = G.make_config(enable_8_bit=True, mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1)
    stream = torch.cuda.Stream(); sh = C.c_void_p(stream.cuda_stream)
    cap = int(caps.sum())
    blob = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device="cuda"); offs = torch.zeros(st.k + 1, dtype=torch.int64, device="cuda")
    d_dres = torch.full((st.k * U.RES_DT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    rec = np.zeros(st.k, DIRPAGE_DT)
    rec["dst"] = st.out.data_ptr() + st.in_off[:-1].astype(np.uint64); rec["page_n"] = st.n; rec["meta_piece"] = rec["page_piece"] = np.arange(st.k); rec["dtype"] = st.dtb
    rec["format_major"] = 4
    d = G.Directory(blob.data_ptr(), cap, offs.data_ptr(), st.k, 0, 0)
    torch.cuda.synchronize()
    U.device_delay(stream, 20)   # (the three calls below return while the stream is still busy: none of them waits for it)
    G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(cfg), None, st.d_res.data_ptr(), sh))
    G.check(L.pco_gfx_compact_chunks(st.k, U.ptr(tasks), st.d_res.data_ptr(), blob.data_ptr(), cap, 0, offs.data_ptr(), None, sh))
    G.check(L.pco_gfx_decompress_chunks_dir(st.k, U.ptr(rec), C.addressof(d), None, d_dres.data_ptr(), sh))
    stream.synchronize()
    enc = st.results(); dec = st.results(d_dres); o = offs.cpu().numpy()
    assert [int(s) for s in enc["status"]] == [0, 0, G.ST_INVALID_ARGUMENT, 0, 0] and o[2] == o[3]
    assert tuples(dec)[2] == (G.ST_INSUFFICIENT_DATA, 0, 0, 0) and [t[:2] for j, t in enumerate(tuples(dec)) if j != 2] == [(0, a.size) for j, a in enumerate(arrays) if j != 2]
    assert st.outputs_equal() == [2]
    assert (st.out.cpu().numpy()[st.in_off[2]: st.in_off[3]] == 0).all(), "the dropped chunk's dst was written"


CONFIGS = {"consecutive": lambda P: P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_consecutive(1)),
           "lookback": lambda P: P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_lookback())}


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_the_same_through_paged_and_the_framed_blob_is_a_file_the_oracle_reads(L, config):
    import torch
    import pcodec_amd as P
    from pcodec_amd import paged
    kind = "smooth" if config == "consecutive" else "periodic"
    arrays = [numbers("int64", n, kind, s) for s, n in enumerate((2049, 1, 257, 4096))]
    tensors = [torch.from_numpy(a).cuda() for a in arrays]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    cc = paged.compress_standalone_chunks(tensors, CONFIGS[config](P), stream=stream)
    outs, results = paged.decompress_chunks_async(cc, stream=stream)
    rows, rres = paged.decompress_rows_async(cc, [(250, 262), None, (256, 257), (0, 4096)], stream=stream)
    idx = paged.index_pages_async(cc, 512, stream=stream, history=True)
    segs, sres = paged.decompress_chunks_from_async(cc, idx, stream=stream)
    stream.synchronize()   # the one synchronisation
    for res in (results, rres, idx.results, sres):
        assert (res.cpu().numpy().view(paged.RESULT_DT)["status"] == 0).all()
    for a, o, s in zip(arrays, outs, segs):
        assert np.array_equal(o.cpu().numpy(), a) and np.array_equal(s.cpu().numpy(), a)
    assert [r.cpu().numpy().tolist() for r in rows] == [arrays[0][250:262].tolist(), arrays[2][256:257].tolist(), arrays[3].tolist()]
    assert [pc.cursors.shape[0] for pc in idx] == [4, 0, 0, 7]
    if config == "lookback":
        assert any((h.cpu().numpy()[:, :64] != 0).any() for h, pc in zip(idx.histories, idx) if pc.cursors.shape[0])
    f = cc.file.cpu().numpy().tobytes()
    assert len(f) == cc.total + 1 and f[-1] == 0 and f[:4] == b"pco!" and cc.header_len == U.standalone_header_len(sum(a.size for a in arrays))
    assert np.array_equal(O.simple_decompress(f, np.int64, cap=sum(a.size for a in arrays) + 8), np.concatenate(arrays))
    # without the frame the chunks start at 0 and nothing follows them
    bare = paged.compress_standalone_chunks(tensors, CONFIGS[config](P), file_frame=False)
    assert bare.header_len == 0 and bare.file.cpu().numpy().tobytes() == f[cc.header_len:-1]


def test_a_blob_too_small_for_the_chunks_raises_on_the_host_and_refuses_every_task(L):
    """compress_standalone_chunks(blob_cap=...) one byte short: the compactor copies nothing and leaves its sentinel; `.total` / `.file` raise, the
    terminator lands in the slack behind the capacity, and every decode, read and index task answers INVALID_ARGUMENT with its output untouched.  One
    byte more and the file is whole."""
    import torch
    import pcodec_amd as P
    from pcodec_amd import paged
    arrays = [numbers("int64", n, "smooth", s) for s, n in enumerate((2049, 257))]
    tensors = [torch.from_numpy(a).cuda() for a in arrays]
    cfg = CONFIGS["consecutive"](P)
    need = len(paged.compress_standalone_chunks(tensors, cfg).file)
    ok = paged.compress_standalone_chunks(tensors, cfg, blob_cap=need)
    assert ok.blob.numel() == need + 64 and np.array_equal(O.simple_decompress(ok.file.cpu().numpy().tobytes(), np.int64, cap=4096), np.concatenate(arrays))
    cc = paged.compress_standalone_chunks(tensors, cfg, blob_cap=need - 1)
    outs, results = paged.decompress_chunks_async(cc)
    rows, rres = paged.decompress_rows_async(cc, [(0, 10), (256, 257)])
    idx = paged.index_pages_async(cc, 256)
    torch.cuda.synchronize()
    assert int(cc.offsets[-1].item()) == -1
    for res in (results, rres, idx.results):
        assert tuples(res.cpu().numpy().view(U.RES_DT)) == [(G.ST_INVALID_ARGUMENT, 0, 0, 0)] * 2
    assert (idx[0].cursors.cpu().numpy() == 0).all()
    for name in ("total", "file"):
        with pytest.raises(G.PcoGfxError) as err:
            getattr(cc, name)
        assert err.value.status == G.ST_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        paged.compress_standalone_chunks(tensors, cfg, blob_cap=3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the work: the pointer form's kernels and ONE resolve kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def launches(L, fn):
    import torch
    fn()   # (untimed: the workspace grows here)
    torch.cuda.synchronize()
    L.pco_gfx_profile_begin()
    fn()
    return U.profile_launches(L)


@pytest.mark.parametrize("kind", ["page", "read", "index"])
@pytest.mark.parametrize("spec", ["classic", "lookback", "dict"])
def test_a_chunk_call_is_the_pointer_form_s_kernels_and_one_resolve_kernel(L, spec, kind):
    b = blob_of(L, spec, 0); e = b.e; lay = Layout()
    if kind == "index":
        tasks = index_tasks(L, e, lay, 256, True)
    else:
        tasks = []
        for i, a in enumerate(e.arrays):
            o = lay.take(a.nbytes)
            tasks.append(dict(i=i, dst_off=o, extents=[]) if kind == "page" else dict(i=i, first=0, count=a.size, dst_off=o, to_off=lay.take(256), extents=[]))
    area = lay.areas(1)[0]
    for form in ("sync", "async"):
        pointer = launches(L, lambda: run(L, Source(b), tasks, area, True, FLAG, form))
        chunk = launches(L, lambda: run(L, Source(b), tasks, area, False, FLAG, form))
        resolve = [n for n in chunk if n.startswith("dir_resolve")]
        assert resolve == ["dir_resolve_chunks_reads_kernel" if kind == "read" else "dir_resolve_chunks_kernel"], resolve
        assert [n for n in chunk if not n.startswith("dir_resolve")] == pointer and chunk[0] == resolve[0]
