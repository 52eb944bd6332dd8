"""-m gpu: pco_gfx_decompress_page_reads_dir / pco_gfx_index_pages_dir (include/pco_gfx.h section 4k) -- page reads and page indexes from a page
directory that lies in DEVICE memory, and pcodec_amd.paged's three functions over them.

Truth is one of two things: the input array, or the POINTER form (pco_gfx_decompress_page_reads_hist, pco_gfx_index_pages_hist: code from before
these entry points) on the same bytes, given the pointers and lengths the directory describes.  Every output of a call -- dst, `to` cursors, history
buffers, cursor slots, histories -- lies in ONE device area between canary bytes; the pointer form runs on a second area of the same layout and the
same first bytes, and the two areas are compared WHOLE, so a refused task that wrote a byte, a stride's tail that was touched or a cursor that differs
in one bit fails.  A third area of that layout is where the decoy tasks point that overwrite the task array as each _dir call returns, beside a
directory whose chunks all read "dropped": it must stay as it was.

Shapes: the chunks of test_gpu_page_directory.py (4608 numbers in pages of 2049 / 1111 / 1448 or of at most 1537) under its eight specs, a Conv1 and
a Dict spec, gaps of 0 and 4 bytes, cursors every 256 and 512 rows; one i64 Lookback page of 2^15 + 2 * 256 + 17 rows -- the smallest whose ring
wraps -- with a cursor every 4096.

Measured on an MI355X: the module takes 90 to 115 s (733 passed, no call above 1.1 s); the -m gpu suite takes 283 to 302 s with it (1751 passed, the
3 skips as before) and 175 to 187 s without it (1018 passed).  Which rows the mutations of the resolve step fail is recorded in DESIGN.md section 2."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
import test_gpu_page_directory as D  # noqa: E402  (SPECS, encoded, Blob, blob_of, edited: the shapes and the compacted blobs)
import test_gpu_page_index as PI  # noqa: E402  (profiled)
import test_gpu_page_ranges as R  # noqa: E402  (numbers)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec, PagingSpec  # noqa: E402
from test_gpu_page_directory import L  # noqa: E402,F401  (module fixture)
from test_gpu_wrapped_writer import Call, handle  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY, PAD, FLAG, TAIL, ALL_ONES = 0xA5, 64, 1, 24, (1 << 64) - 1
_u8, _u4 = "<u8", "<u4"
READ_DT = np.dtype([("meta", _u8), ("meta_len", _u8), ("page", _u8), ("page_len", _u8), ("dst", _u8), ("page_n", _u8), ("first", _u8), ("count", _u8), ("dtype", _u4),
                    ("format_major", _u4), ("from", _u8), ("to", _u8), ("history", _u8), ("history_len", _u8)])
INDEX_DT = np.dtype([("meta", _u8), ("meta_len", _u8), ("page", _u8), ("page_len", _u8), ("cursors", _u8), ("page_n", _u8), ("every_rows", _u8), ("dtype", _u4),
                     ("format_major", _u4), ("histories", _u8), ("history_stride", _u8)])
DIRREAD_DT = np.dtype([("dst", _u8), ("page_n", _u8), ("first", _u8), ("count", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4),
                       ("from", _u8), ("to", _u8), ("history", _u8), ("history_len", _u8)])
DIRINDEX_DT = np.dtype([("cursors", _u8), ("page_n", _u8), ("every_rows", _u8), ("meta_piece", _u4), ("page_piece", _u4), ("dtype", _u4), ("format_major", _u4),
                        ("histories", _u8), ("history_stride", _u8)])
assert (READ_DT.itemsize, INDEX_DT.itemsize, DIRREAD_DT.itemsize, DIRINDEX_DT.itemsize) == (104, 80, 80, 56)
LONG_N, LONG_EVERY = (1 << 15) + 2 * 256 + 17, 4096

SPECS = dict(D.SPECS, conv1=dict(mode=1, delta=G.DELTA_TRY_CONV1, delta_order=3, conv1=True), dict=dict(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1, dict=True))
# (the routes: Classic, Consecutive and float-mult take the two-kernel route, level12 has wide tables, conv1 and dict the general kernel, Lookback histories)
_calls, _blobs = {}, {}


def encoded(L, spec):
    if spec in D.SPECS:
        return D.encoded(L, spec)
    if spec not in _calls:
        rng = np.random.default_rng(77)
        if spec == "conv1":
            import test_gpu_conv1_encode as TC
            arrays, lists = [TC.smooth(D.N, dt, seed=s) for s, dt in enumerate(("int32", "float32", "uint32"))], [D.EXACT, None, D.EXACT]
        elif spec == "dict":
            arrays = [rng.integers(0, 1 << 14, 200).astype(dt)[rng.integers(0, 200, D.N)] for dt in ("uint64", "float32", "int16")]; lists = [D.EXACT, None, D.EXACT]
        else:   # "long": ONE i64 Lookback page longer than its window of 2^15
            arrays, lists = [R.numbers(np.int64, LONG_N, 8, period=365)], [[LONG_N]]
        cfg = G.make_config(max_page_n=D.MAX_PAGE_N, enable_8_bit=True, **(SPECS[spec] if spec != "long" else SPECS["classic+lookback"]))
        c = Call(L, arrays, cfg, lists)
        G.check(c.encode())
        assert (c.infos["status"] == 0).all()
        meta = c.pieces()[0][0]
        if spec == "conv1":
            assert G.chunk_meta_conv1(meta, c.dtb[0]) is not None, "the spec was not taken"
        if spec == "dict":
            assert G.chunk_meta_dict(meta, c.dtb[0]) is not None, "the spec was not taken"
        _calls[spec] = c
    return _calls[spec]


def blob_of(L, spec, gap):
    if (spec, gap) not in _blobs:
        _blobs[spec, gap] = D.Blob(encoded(L, spec), gap)
    return _blobs[spec, gap]


def every_of(spec, gap):
    return LONG_EVERY if spec == "long" else (512 if gap else 256)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the harness: a layout of output extents, three areas of it, the two forms of a call over the same task descriptions
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

    def areas(self, n=3):
        import torch
        img = self.image()
        out = [torch.from_numpy(img.copy()).cuda() for _ in range(n)]
        torch.cuda.synchronize()
        return out


class Source:
    """Where the pieces of a compacted blob lie, for both forms: the PcoGfxDirectory (over `offs`, a device tensor that may be an edited copy) and the
    pointers and lengths the blob's OWN offsets describe."""

    def __init__(self, b, offs=None, blob_len=None):
        self.b, self.c = b, b.c
        self.true = b.offs.cpu().numpy().view(np.uint64)
        self.offs = b.offs if offs is None else offs
        self.blob_len = b.cap if blob_len is None else blob_len

    def directory(self):
        return G.Directory(self.b.blob.data_ptr(), self.blob_len, self.offs.data_ptr(), self.c.n_pieces, self.b.gap, 0)

    def piece(self, k):
        return self.b.blob.data_ptr() + int(self.true[k]) + self.b.gap, int(self.true[k + 1]) - int(self.true[k]) - self.b.gap


def fill(rec, src, t, base, pointer_form):
    """One record of either form from the description `t`: offsets into the area at `base` under *_off keys, absolute device pointers under *_abs keys."""
    c = src.c; i, p = t["i"], t["p"]; k0 = int(c.piece_first[i])
    at = lambda key: (base + t[key + "_off"]) if t.get(key + "_off") is not None else (t.get(key + "_abs") or 0)   # noqa: E731
    if pointer_form:
        (rec["meta"], rec["meta_len"]), (rec["page"], rec["page_len"]) = src.piece(k0), src.piece(k0 + 1 + p)
    else:
        rec["meta_piece"], rec["page_piece"] = k0, k0 + 1 + p
    rec["page_n"], rec["dtype"], rec["format_major"] = c.pages[i][p], c.dtb[i], 4
    if "every" in t:
        rec["every_rows"], rec["cursors"], rec["histories"], rec["history_stride"] = t["every"], at("cursors"), at("histories"), t.get("stride", 0)
    else:
        rec["first"], rec["count"], rec["dst"], rec["from"], rec["to"], rec["history"], rec["history_len"] = t["first"], t["count"], at("dst"), at("from"), at("to"), at("history"), t.get("history_len", 0)


def records(src, tasks, base, pointer_form):
    index = bool(tasks) and "every" in tasks[0]
    rec = np.zeros(len(tasks), (INDEX_DT if index else READ_DT) if pointer_form else (DIRINDEX_DT if index else DIRREAD_DT))
    for j, t in enumerate(tasks):
        fill(rec[j], src, t, base, pointer_form)
    return rec


def run(L, src, tasks, area, pointer_form, flags, form, stream=None, decoy=None, subset=None):
    """One call of either form over `tasks` (the pointer form over tasks[j] for j in `subset` alone).  Returns (code, status, results as RES_DT of
    len(tasks): the device results, which a synchronous call's host results must equal)."""
    import torch
    index = "every" in tasks[0]
    js = list(range(len(tasks))) if subset is None else list(subset)
    rec = records(src, [tasks[j] for j in js], area.data_ptr(), pointer_form)
    d_res = torch.full((max(len(js), 1) * U.RES_DT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    zero_offs = torch.zeros(src.c.n_pieces + 1, dtype=torch.int64, device="cuda")
    host = np.zeros(len(js), U.RES_DT); host["status"] = 99
    torch.cuda.current_stream().synchronize()   # (the two fills; a caller's stream keeps running)
    res_arg = U.ptr(host) if form == "sync" else None
    if pointer_form:
        fn = L.pco_gfx_index_pages_hist if index else L.pco_gfx_decompress_page_reads_hist
        code = fn(len(rec), U.ptr(rec), flags, res_arg, d_res.data_ptr(), handle(stream))
        status = L.pco_gfx_last_status()
    else:
        d = src.directory()
        fn = L.pco_gfx_index_pages_dir if index else L.pco_gfx_decompress_page_reads_dir
        code = fn(len(rec), U.ptr(rec), C.addressof(d), flags, res_arg, d_res.data_ptr(), handle(stream))
        status = L.pco_gfx_last_status()
        # VALID decoys as the call returns: the tasks over another area, a directory whose chunks all read "dropped"
        rec[:] = records(src, [tasks[j] for j in js], (decoy if decoy is not None else area).data_ptr(), False)
        C.memmove(C.addressof(d), C.addressof(G.Directory(d.d_blob, d.blob_len, zero_offs.data_ptr(), d.n_pieces, d.gap, 0)), C.sizeof(G.Directory))
        del d; gc.collect()
    if stream is not None:
        return code, status, (d_res, host, js)
    return code, status, finish(tasks, d_res, host, js, form)


def finish(tasks, d_res, host, js, form):
    import torch
    torch.cuda.synchronize()
    dev = d_res.cpu().numpy().view(U.RES_DT)[: len(js)].copy()
    if form == "sync":
        assert np.array_equal(dev, host), "the host results of a synchronous call are not its device results"
    out = np.zeros(len(tasks), U.RES_DT); out["status"] = 1000   # (a task the pointer form was not given)
    out[js] = dev
    return out


def tuples(res):
    return [(int(r["status"]), int(r["n_out"]), int(r["consumed"]), int(r["aux"])) for r in res]


def both(L, src, tasks, layout, flags, form, failing=None, unspecified=(), areas=None, what=""):
    """The pointer form on area 0 (over the tasks the directory does not fail), the _dir form on area 1 with area 2 for its decoys: results and whole
    areas equal; a task in `failing` = {j: status} answers {status, 0, 0, 0} and leaves every one of its extents as it was; the extents of the tasks in
    `unspecified` (a damaged page: the header calls their bytes unspecified) are masked.  Returns (the areas, the results)."""
    failing = failing or {}
    a = areas or layout.areas()
    ok = [j for j in range(len(tasks)) if j not in failing]
    want = np.zeros(len(tasks), U.RES_DT)
    if ok:
        _, _, want = run(L, src, tasks, a[0], True, flags, form, subset=ok)
    for j, st in failing.items():
        want[j] = (0, 0, st, 0)
    code, status, got = run(L, src, tasks, a[1], False, flags, form, decoy=a[2])
    assert tuples(got) == tuples(want), f"{what}: (status, n_out, consumed, aux) of the _dir form, then of the pointer form"
    bad = [j for j in range(len(tasks)) if want[j]["status"] != 0]
    if form == "sync":
        assert (code, status) == ((G.PcoSuccess, 0) if not bad else (G.PcoDecompressionError, int(want[bad[0]]["status"]))), (code, status)
    else:
        assert code == G.PcoSuccess
    h0, h1, h2 = (x.cpu().numpy() for x in a)
    for j in unspecified:
        for o, n in tasks[j]["extents"]:
            h0[o: o + n] = 0; h1[o: o + n] = 0
    if not np.array_equal(h0, h1):
        at = int(np.flatnonzero(h0 != h1)[0])
        owner = [j for j, t in enumerate(tasks) if any(o - PAD <= at < o + n + PAD for o, n in t["extents"])]
        raise AssertionError(f"{what}: the areas of the two forms differ in {int((h0 != h1).sum())} bytes, first at {at} (task {owner})")
    img = layout.image()
    for j in failing:
        for o, n in tasks[j]["extents"]:
            assert np.array_equal(h1[o - PAD: o + n + PAD], img[o - PAD: o + n + PAD]), f"{what}: the refused task {j} wrote into one of its extents"
    assert np.array_equal(h2, img), f"{what}: the decoy tasks ran: the task array or the directory was read after the call returned"
    return a, got


def window_bytes(L, c, i):
    return L.pco_gfx_lookback_history_bytes(L.pco_gfx_lookback_window_n_log(c.arrays[i].size), c.dtb[i])


def stride_of(L, c, i):
    return (window_bytes(L, c, i) + 7) // 8 * 8 + TAIL


def index_tasks(L, c, layout, every, hist, pages=None):
    """One index task per page: its k cursor slots and -- with `hist` -- k histories of the chunk's window plus TAIL bytes of stride behind each."""
    tasks = []
    for i in range(c.k):
        for p, n in enumerate(c.pages[i]):
            if pages is not None and (i, p) not in pages:
                continue
            k = max((n - 1) // every, 0)
            t = dict(i=i, p=p, every=every, k=k, extents=[])
            if k:
                t["cursors_off"] = layout.take(k * 256); t["extents"].append((t["cursors_off"], k * 256))
            if hist and k:
                t["stride"] = stride_of(L, c, i)
                t["histories_off"] = layout.take(k * t["stride"]); t["extents"].append((t["histories_off"], k * t["stride"]))
            tasks.append(t)
    return tasks


_indexes = {}


def built_index(L, spec, gap, flags, hist):
    """The index of every page of (spec, gap) from the POINTER form, kept: (its tasks, the area as a device tensor, its host copy).  Read-only afterwards."""
    key = (spec, gap, flags, hist)
    if key not in _indexes:
        b = blob_of(L, spec, gap); lay = Layout()
        tasks = index_tasks(L, b.c, lay, every_of(spec, gap), hist)
        area = lay.areas(1)[0]
        code, status, res = run(L, Source(b), tasks, area, True, flags, "sync")
        assert code == G.PcoSuccess and [r[1] for r in tuples(res)] == [t["k"] for t in tasks], tuples(res)
        _indexes[key] = (tasks, area, area.cpu().numpy())
    return _indexes[key]


def segment_tasks(L, c, layout, index, hist, own=False, pages=None):
    """Every page cut at its index's cursors: segment s reads from cursor s - 1 (and history s - 1).  own False: the pair is the index's, read in place,
    and to == NULL leaves it alone.  own True: `to` is a slot of the task's own and the history a copy of the index's in the task's own extent, so
    that a task that runs updates both -- and a refused one must not."""
    itasks, iarea, ihost = index
    by = {(t["i"], t["p"]): t for t in itasks}
    tasks = []; page_dst = {}
    for i in range(c.k):
        w = c.arrays[i].dtype.itemsize
        for p, n in enumerate(c.pages[i]):
            if pages is not None and (i, p) not in pages:
                continue
            it = by[i, p]; every = it["every"]
            page_dst[i, p] = layout.take(n * w)
            for s, row in enumerate(range(0, n, every) if it["k"] else [0]):
                count = min(every, n - row) if it["k"] else n
                t = dict(i=i, p=p, first=row, count=count, dst_off=page_dst[i, p] + row * w, extents=[(page_dst[i, p] + row * w, count * w)])
                if s:
                    t["from_abs"] = iarea.data_ptr() + it["cursors_off"] + (s - 1) * 256
                    if hist and "histories_off" in it:
                        h = it["histories_off"] + (s - 1) * it["stride"]
                        if own:
                            t["history_off"] = layout.take(it["stride"], ihost[h: h + it["stride"]]); t["extents"].append((t["history_off"], it["stride"]))
                        else:
                            t["history_abs"] = iarea.data_ptr() + h
                        t["history_len"] = it["stride"]
                if own:
                    t["to_off"] = layout.take(256); t["extents"].append((t["to_off"], 256))
                tasks.append(t)
    return tasks, page_dst


def rows_equal_the_input(c, area, page_dst, what=""):
    host = area.cpu().numpy()
    for (i, p), o in page_dst.items():
        a = c.arrays[i]; r0 = sum(c.pages[i][:p]); n = c.pages[i][p]
        want = a[r0: r0 + n].view(np.uint8).reshape(-1)
        assert np.array_equal(host[o: o + want.size], want), f"{what}: page {p} of chunk {i} differs from the input"


@pytest.fixture(autouse=True)
def nothing_more_after_a_device_error(L):
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error; nothing more is launched on it: {e}", returncode=3)


ALL_SPECS = sorted(SPECS) + ["long"]
MODES = [(0, False), (FLAG, False), (0, True), (FLAG, True)]
MODE_IDS = ["plain", "general", "hist", "general+hist"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the index
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_the_index_is_the_pointer_form_s_byte_for_byte(L, spec, gap, flags, hist, form):
    b = blob_of(L, spec, gap); c = b.c; lay = Layout()
    tasks = index_tasks(L, c, lay, every_of(spec, gap), hist)
    a, res = both(L, Source(b), tasks, lay, flags, form, what=f"{spec} gap {gap}")
    assert [r[0] for r in tuples(res)] == [0] * len(tasks) and [r[1] for r in tuples(res)] == [t["k"] for t in tasks]
    if hist:   # the stride's tail is nobody's: untouched whatever the page is (and a page without Lookback leaves its histories alone altogether)
        host = a[1].cpu().numpy(); lookback = "lookback" in spec or spec == "long"; stamped = 0
        for t in tasks:
            for s in range(t["k"]):
                o = t["histories_off"] + s * t["stride"]; used = window_bytes(L, c, t["i"]) if lookback else 0
                assert (host[o + used: o + t["stride"]] == CANARY).all(), (t["i"], t["p"], s)
                stamped += int((host[o: o + 64] != CANARY).any())
        assert (stamped > 0) == lookback, f"{stamped} histories were stamped"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. reads: a chain of slices, and all segments side by side
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_a_chain_of_slices_each_from_the_to_of_the_last(L, spec, flags, hist, form):
    """Slice s of every page in call s: from == to == the page's one cursor slot, the page's one history beside it.  (Slices of 256 rows over gap 0 in the
    synchronous form, of 512 over gap 4 in the asynchronous one.)"""
    gap = 0 if form == "sync" else 4
    b = blob_of(L, spec, gap); c = b.c; lay = Layout(); every = every_of(spec, gap) * (2 if spec == "long" else 1)
    pages = []
    for i in range(c.k):
        w = c.arrays[i].dtype.itemsize
        for p, n in enumerate(c.pages[i]):
            pg = dict(i=i, p=p, n=n, w=w, dst=lay.take(n * w), cur=lay.take(256))
            if hist:
                pg["stride"] = stride_of(L, c, i); pg["hist"] = lay.take(pg["stride"])
            pages.append(pg)
    areas = lay.areas(); src = Source(b)
    for s in range(max(-(-pg["n"] // every) for pg in pages)):
        tasks = []
        for pg in pages:
            row = s * every
            if row >= pg["n"]:
                continue
            count = min(every, pg["n"] - row)
            t = dict(i=pg["i"], p=pg["p"], first=row, count=count, dst_off=pg["dst"] + row * pg["w"], to_off=pg["cur"], from_off=pg["cur"] if s else None,
                     extents=[(pg["dst"] + row * pg["w"], count * pg["w"]), (pg["cur"], 256)])
            if hist:
                t["history_off"], t["history_len"] = pg["hist"], pg["stride"]; t["extents"].append((pg["hist"], pg["stride"]))
            tasks.append(t)
        _, res = both(L, src, tasks, lay, flags, form, areas=areas[:2] + [lay.areas(1)[0]], what=f"{spec} gap {gap} slice {s}")
        assert [r[0] for r in tuples(res)] == [0] * len(tasks), tuples(res)
    rows_equal_the_input(c, areas[1], {(pg["i"], pg["p"]): pg["dst"] for pg in pages}, f"{spec} gap {gap}")


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("spec", ALL_SPECS)
def test_all_segments_side_by_side_from_the_index_s_pairs(L, spec, gap, flags, hist, form):
    b = blob_of(L, spec, gap); c = b.c; lay = Layout()
    index = built_index(L, spec, gap, flags, hist)
    tasks, page_dst = segment_tasks(L, c, lay, index, hist)
    a, res = both(L, Source(b), tasks, lay, flags, form, what=f"{spec} gap {gap}")
    assert [r[0] for r in tuples(res)] == [0] * len(tasks), tuples(res)
    rows_equal_the_input(c, a[1], page_dst, f"{spec} gap {gap}")
    assert np.array_equal(index[1].cpu().numpy(), index[2]), "to == NULL leaves the index's pairs as they are"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. directory verdicts
# ---------------------------------------------------------------------------------------------------------------------------------------
def defective(L, spec, defect):
    """(the Source whose directory has the defect, {(chunk, page) it fails: status})"""
    import torch
    b = blob_of(L, spec, 4); c = b.c; n = c.n_pieces
    page_of = {int(c.piece_first[i]) + 1 + p: (i, p) for i in range(c.k) for p in range(len(c.pages[i]))}
    everything = {ip: G.ST_INVALID_ARGUMENT for ip in page_of.values()}
    if defect == "dropped chunk":
        infos = c.infos.copy(); infos["status"][int(c.piece_first[1]) + 1] = G.ST_INVALID_ARGUMENT
        kept = infos.copy(); kept["len"][int(c.piece_first[1]): int(c.piece_first[2])] = 0
        b2 = D.Blob(c, 4, d_infos=torch.from_numpy(infos.view(np.uint8).copy()).cuda(), infos=kept, cap=int((kept["len"] + 4).sum()) - 4 * (1 + len(c.pages[1])))
        return Source(b2), {(1, p): G.ST_INSUFFICIENT_DATA for p in range(len(c.pages[1]))}

    def edit(o):
        if defect == "sentinel":
            o[n] = ALL_ONES
        elif defect == "swapped pair":
            o[n - 1], o[n] = o[n], o[n - 1]
        elif defect == "end beyond blob_len":
            o[n] = b.cap + 1
        elif defect == "extent of gap - 1":
            o[n] = int(o[n - 1]) + 3
        else:   # "chunk meta": chunk 1's ChunkMeta has an extent of gap - 1
            o[int(c.piece_first[1]) + 1] = int(o[int(c.piece_first[1])]) + 3
    failing = everything if defect == "sentinel" else ({(1, p): G.ST_INVALID_ARGUMENT for p in range(len(c.pages[1]))} if defect == "chunk meta" else {page_of[n - 1]: G.ST_INVALID_ARGUMENT})
    return Source(b, offs=D.edited(b, edit)), failing


DEFECTS = ["sentinel", "swapped pair", "end beyond blob_len", "extent of gap - 1", "dropped chunk", "chunk meta"]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("kind", ["read", "index"])
@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("spec", ["classic+consecutive1", "classic+lookback"])
def test_a_directory_defect_fails_the_named_tasks_alone(L, spec, defect, kind, flags, hist, form):
    src, bad_pages = defective(L, spec, defect); c = src.c; lay = Layout()
    if kind == "index":
        tasks = index_tasks(L, c, lay, 512, hist)
    else:   # every segment from the cursor (and a copy of the history) in front of it, leaving a `to` cursor of its own
        tasks, _ = segment_tasks(L, c, lay, built_index(L, spec, 4, flags, hist), hist, own=True)
    failing = {j: bad_pages[t["i"], t["p"]] for j, t in enumerate(tasks) if (t["i"], t["p"]) in bad_pages and t.get("k", 1)}
    assert failing and (defect == "sentinel" or len(failing) < len(tasks))
    both(L, src, tasks, lay, flags, form, failing, what=f"{spec}, {defect}, {kind}")


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("gap", [0, 4])
def test_pages_of_zero_bytes_decode_and_index(L, gap, form):
    """Constant uint32 chunks under Classic without delta: pages of 0 bytes beside a ChunkMeta of a few (the dropped-chunk rule is the ChunkMeta's)."""
    key = ("zero", gap)
    if key not in _blobs:
        const = lambda v: np.full(3000, v, np.uint32)   # noqa: E731
        c = Call(L, [U.synth("c2", 1500, seed=1), const(7), const(0xDEADBEEF), const(0)], G.make_config(**SPECS["classic"]), [None, [1000, 1000, 1000], [1000, 1000, 1000], [1, 2998, 1]])
        G.check(c.encode())
        assert all((c.infos["len"][int(c.piece_first[i]) + 1: int(c.piece_first[i]) + 4] == 0).all() for i in (1, 2, 3))
        _blobs[key] = D.Blob(c, gap)
    b = _blobs[key]; c = b.c
    for flags, hist in MODES:
        lay = Layout(); tasks = index_tasks(L, c, lay, 256, hist)
        _, res = both(L, Source(b), tasks, lay, flags, form, what="index of zero-byte pages")
        assert [r[0] for r in tuples(res)] == [0] * len(tasks)
        lay = Layout(); tasks = []; dsts = {}
        for i in range(c.k):
            for p, n in enumerate(c.pages[i]):
                for f, k in ((0, 1), (0, n), (n - 1, 1)):
                    w = c.arrays[i].dtype.itemsize
                    o = lay.take(k * w); dsts[len(tasks)] = (o, c.arrays[i][sum(c.pages[i][:p]) + f: sum(c.pages[i][:p]) + f + k])
                    t = dict(i=i, p=p, first=f, count=k, dst_off=o, to_off=lay.take(256))
                    t["extents"] = [(o, k * w), (t["to_off"], 256)]; tasks.append(t)
        a, res = both(L, Source(b), tasks, lay, flags, form, what="reads of zero-byte pages")
        assert [r[0] for r in tuples(res)] == [0] * len(tasks)
        host = a[1].cpu().numpy()
        for o, want in dsts.values():
            assert np.array_equal(host[o: o + want.nbytes], want.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. empty tasks over a directory of garbage
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
def test_empty_tasks_are_ok_whatever_the_directory_looks_like(L, flags, hist, form):
    b = blob_of(L, "classic+lookback", 4); c = b.c

    def edit(o): o[1:] = o[1:][::-1].copy()
    src = Source(b, offs=D.edited(b, edit), blob_len=3)
    lay = Layout(); tasks = index_tasks(L, c, lay, 2304, hist)   # every page is shorter than 2304 + 1 rows: k == 0
    assert all(t["k"] == 0 for t in tasks)
    for t in tasks:   # pointers that are judged by the host and never followed
        t["cursors_off"] = lay.take(256); t["extents"].append((t["cursors_off"], 256))
    _, res = both(L, src, tasks, lay, flags, form, what="k == 0")
    assert tuples(res) == [(0, 0, 0, 0)] * len(tasks)
    lay = Layout(); tasks = []
    for i in range(c.k):
        for p, n in enumerate(c.pages[i]):
            for first in (0, 5, n):
                t = dict(i=i, p=p, first=first, count=0, dst_off=lay.take(16), from_off=lay.take(256), to_off=lay.take(256))
                t["extents"] = [(t["dst_off"], 16), (t["from_off"], 256), (t["to_off"], 256)]
                if hist:
                    t["history_len"] = stride_of(L, c, i); t["history_off"] = lay.take(t["history_len"]); t["extents"].append((t["history_off"], t["history_len"]))
                tasks.append(t)
    _, res = both(L, src, tasks, lay, flags, form, what="count == 0")
    assert tuples(res) == [(0, 0, 0, 0)] * len(tasks)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. refused cursors and histories, damaged pages: the pointer form's results
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", ["classic+consecutive2", "classic+lookback", "conv1"])
def test_a_refused_cursor_or_history_is_the_pointer_form_s_refusal(L, spec, flags, hist, form):
    """Per page: segment 1 from ANOTHER page's cursor, from a cursor of canary bytes, from the right cursor beside a history of half its length, and --
    the control -- from the right pair."""
    b = blob_of(L, spec, 4); c = b.c; lay = Layout()
    index = built_index(L, spec, 4, flags, hist)
    good, _ = segment_tasks(L, c, lay, index, hist, own=True)
    ones = [t for t in good if t["first"] == 512]
    assert len(ones) >= 3
    tasks = []
    for j, t in enumerate(ones):
        other = ones[(j + 1) % len(ones)]
        foreign = dict(t, from_abs=other["from_abs"]); junk = dict(t, from_abs=None, from_off=lay.take(256)); short = dict(t)
        if "history_off" in t:
            short["history_len"] = (t["history_len"] // 2) // 8 * 8
        for v in (foreign, junk, short):   # (fresh outputs for each variant)
            w = c.arrays[t["i"]].dtype.itemsize
            v["dst_off"] = lay.take(t["count"] * w); v["to_off"] = lay.take(256); v["extents"] = [(v["dst_off"], t["count"] * w), (v["to_off"], 256)]
            if "history_off" in t:
                h = t["history_off"]; first = lay.image()[h: h + t["history_len"]]
                v["history_off"] = lay.take(t["history_len"], first); v["extents"].append((v["history_off"], t["history_len"]))
        tasks += [foreign, junk, short, t]
    _, res = both(L, Source(b), tasks, lay, flags, form, unspecified=[j for j in range(len(tasks)) if j % 4 == 0], what=spec)
    st = [r[0] for r in tuples(res)]
    assert all(s == 0 for s in st[3::4]) and all(s != 0 for s in st[1::4]), st
    print(f"{spec} flags {flags} hist {hist} {form}: statuses (foreign, junk, short history, control) {st}")


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
def test_a_short_history_stride_refuses_its_index_task_alone(L, flags, hist, form):
    b = blob_of(L, "classic+lookback", 4); c = b.c; lay = Layout()
    tasks = index_tasks(L, c, lay, 512, True)
    for t in tasks[::2]:
        if t["k"]:
            t["stride"] = 64 + 8   # (its extent stays the longer one)
    _, res = both(L, Source(b), tasks, lay, flags, form, what="short stride")
    st = [r[0] for r in tuples(res)]   # (a page that is not resumable -- the u8 chunk's -- ignores its histories, and their stride)
    assert all(x == 0 for x in st[1::2]) and set(st[::2]) <= {0, G.ST_INVALID_ARGUMENT} and st[::2].count(G.ST_INVALID_ARGUMENT) >= 4, tuples(res)


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", ["classic+consecutive1", "classic+lookback"])
def test_a_page_damaged_behind_and_inside_the_walk(L, spec, flags, hist, form):
    """The blob's last page (1536 rows: six batches) is overwritten from its middle on.  Reads and an index that end in front of the damage are OK,
    the ones that walk into it answer what the pointer form answers over the same bytes."""
    import torch
    key = ("damaged", spec)
    if key not in _blobs:
        b = D.Blob(encoded(L, spec), 4); offs = b.offs.cpu().numpy().view(np.uint64); n = b.c.n_pieces
        start, end = int(offs[n - 1]) + 4, int(offs[n])
        b.blob[start + (end - start) // 2: end] = 0xFF
        torch.cuda.synchronize()
        _blobs[key] = b
    b = _blobs[key]; c = b.c; i = c.k - 1; p = len(c.pages[i]) - 1; page_n = c.pages[i][p]; w = c.arrays[i].dtype.itemsize
    assert page_n == 1536
    lay = Layout(); tasks = []
    for f, k in [(0, 1), (0, 256), (17, 100), (0, page_n), (page_n - 1, 1), (page_n - 300, 300), (256, 1024)]:
        o = lay.take(k * w); t = dict(i=i, p=p, first=f, count=k, dst_off=o, to_off=lay.take(256))
        t["extents"] = [(o, k * w), (t["to_off"], 256)]
        if hist:
            t["history_len"] = stride_of(L, c, i); t["history_off"] = lay.take(t["history_len"]); t["extents"].append((t["history_off"], t["history_len"]))
        tasks.append(t)
    _, res = both(L, Source(b), tasks, lay, flags, form, unspecified=range(3, len(tasks)), what=f"{spec}: reads")
    st = [r[0] for r in tuples(res)]
    assert st[:3] == [0, 0, 0] and all(s in (G.ST_INSUFFICIENT_DATA, G.ST_CORRUPTION) for s in st[3:6]), st
    lay = Layout()
    tasks = index_tasks(L, c, lay, 256, hist, pages={(i, p)}) + index_tasks(L, c, lay, 1280, hist, pages={(i, p)})   # k = 5, and k = 1 with its one cursor at row 1280
    _, res = both(L, Source(b), tasks, lay, flags, form, unspecified=range(len(tasks)), what=f"{spec}: index")
    print(f"{spec} flags {flags} hist {hist} {form}: the index tasks over the damaged page answer {tuples(res)}")
    # a directory whose last entry ends the page at its middle: a page whose bytes end inside the walked prefix, for both forms
    n = c.n_pieces; start, end = int(Source(b).true[n - 1]), int(Source(b).true[n])

    def cut(o): o[n] = start + (end - start) // 2
    short = Source(b, offs=D.edited(b, cut)); short.true = short.offs.cpu().numpy().view(np.uint64)
    lay = Layout(); tasks = index_tasks(L, c, lay, 256, hist, pages={(i, p)})
    _, res = both(L, short, tasks, lay, flags, form, unspecified=range(len(tasks)), what=f"{spec}: index of a page that ends early")
    assert [r[:2] for r in tuples(res)] == [(G.ST_INSUFFICIENT_DATA, 0)], tuples(res)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the pipeline: encode -> compact -> index -> every segment, ONE synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,flags,hist", [("classic+consecutive2", 0, False), ("conv1", FLAG, False), ("classic+lookback", 0, True), ("long", 0, True)])
def test_the_pipeline_synchronises_once(L, spec, flags, hist):
    import torch
    src = encoded(L, spec)
    c = Call(L, src.arrays, src.cfg, src.page_lists)   # fresh slots and d_infos: nothing of this call is known on the host
    gap = 4; cap = sum(c.caps) + gap * c.n_pieces; every = every_of(spec, gap)
    blob = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device="cuda"); offs = torch.zeros(c.n_pieces + 1, dtype=torch.int64, device="cuda")
    ilay = Layout(); itasks = index_tasks(L, c, ilay, every, hist); iarea, idecoy = ilay.areas(2)
    lay = Layout(); tasks, page_dst = segment_tasks(L, c, lay, (itasks, iarea, None), hist)
    area, decoy = lay.areas(2)
    b = type("B", (), dict(blob=blob, offs=offs, cap=cap, gap=gap, c=c))()
    dsrc = Source(b)
    s = torch.cuda.Stream()
    U.device_delay(s)
    tk = c.make_tasks()
    G.check(L.pco_gfx_compress_wrapped_chunks_ex(c.k, tk, C.addressof(c.cfg), None, c.d_infos.data_ptr(), handle(s))); D.note("encode", s)
    G.check(L.pco_gfx_compact_wrapped_chunks(c.k, tk, C.addressof(c.cfg), c.d_infos.data_ptr(), gap, blob.data_ptr(), cap, 0, offs.data_ptr(), None, handle(s))); D.note("compact", s)
    code_i, _, pend_i = run(L, dsrc, itasks, iarea, False, flags, "async", stream=s, decoy=idecoy); D.note("index", s)
    code_r, _, pend_r = run(L, dsrc, tasks, area, False, flags, "async", stream=s, decoy=decoy); D.note("reads", s)
    s.synchronize()   # the one synchronisation
    assert code_i == G.PcoSuccess and code_r == G.PcoSuccess
    ri = finish(itasks, *pend_i, "async"); rr = finish(tasks, *pend_r, "async")
    assert [r[:2] for r in tuples(ri)] == [(0, t["k"]) for t in itasks], tuples(ri)
    assert [r[0] for r in tuples(rr)] == [0] * len(tasks) and [r[1] for r in tuples(rr)] == [t["count"] for t in tasks], tuples(rr)
    rows_equal_the_input(c, area, page_dst, spec)
    assert np.array_equal(idecoy.cpu().numpy(), ilay.image()) and np.array_equal(decoy.cpu().numpy(), lay.image())
    if hist:   # the window the histories were sized by, on the host before the ChunkMeta existed, is the one the encoder chose
        info = G.ChunkMetaInfo(); meta = bytes(blob[gap: int(offs[1].item())].cpu().numpy())
        G.check(L.pco_gfx_chunk_meta_info((C.c_uint8 * len(meta)).from_buffer_copy(meta), len(meta), c.dtb[0], 4, C.byref(info)))
        assert info.delta_kind == 2 and info.window_n_log == L.pco_gfx_lookback_window_n_log(c.arrays[0].size)


PAGED = {"classic+consecutive2": (lambda: ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(2), paging_spec=PagingSpec.equal_pages_up_to(D.MAX_PAGE_N), enable_8_bit=True), False, False),
         "conv1": (lambda: ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_conv1(3), paging_spec=PagingSpec.equal_pages_up_to(D.MAX_PAGE_N), enable_conv1=True), True, False),
         "classic+lookback": (lambda: ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_lookback(), paging_spec=PagingSpec.equal_pages_up_to(D.MAX_PAGE_N), enable_8_bit=True), False, True)}


@pytest.mark.parametrize("spec", sorted(PAGED))
def test_the_pipeline_through_paged(L, spec):
    import torch
    src = encoded(L, spec); make, general, history = PAGED[spec]
    s = torch.cuda.Stream()
    tensors = [torch.from_numpy(a.copy()).cuda() for a in src.arrays]
    torch.cuda.synchronize()
    U.device_delay(s)
    comp = paged.compress_chunks(tensors, make(), page_sizes=src.page_lists, gap=4, stream=s); D.note("paged.compress_chunks", s)
    idx = paged.index_pages_async(comp, 512, stream=s, general=general, history=history); D.note("paged.index_pages_async", s)
    outs, res = paged.decompress_chunks_from_async(comp, idx, stream=s, general=general); D.note("paged.decompress_chunks_from_async", s)
    rows = [(0, 1), (2000, 2100), (600, D.N)] + [None] * (len(tensors) - 3)
    routs, rres = paged.decompress_rows_from_async(comp, idx, rows, stream=s, general=general); D.note("paged.decompress_rows_from_async", s)
    s.synchronize()   # the one synchronisation
    assert comp._dir is None, "the host directory was materialised"
    assert (idx.histories is not None) == history and (not history or all(h is not None for h in idx.histories))
    for a, o in zip(src.arrays, outs):
        assert U.bits_equal(o.cpu().numpy(), a)
    for (lo, hi), a, o in zip(rows, src.arrays, routs):
        assert U.bits_equal(o.cpu().numpy(), a[lo: hi])
    ir = idx.results.cpu().numpy().view(paged.RESULT_DT)
    assert (ir["status"] == 0).all() and ir["n_out"].tolist() == [pc.cursors.shape[0] for pc in idx]
    r = res.cpu().numpy().view(paged.RESULT_DT); rr = rres.cpu().numpy().view(paged.RESULT_DT)
    assert (r["status"] == 0).all() and int(r["n_out"].sum()) == sum(a.size for a in src.arrays) and len(r) == sum(-(-n // 512) for pl in comp.page_ns for n in pl)
    assert (rr["status"] == 0).all() and int(rr["n_out"].sum()) == sum(hi - lo for lo, hi in rows[:3])
    # the same keys and the same bytes as the index from the host directory
    ref = paged.index_pages(comp.blob, comp.directory, comp.dtypes, 512, general=general, history=history)
    torch.cuda.synchronize()
    assert [(p.chunk, p.piece, p.every_rows) for p in ref] == [(p.chunk, p.piece, p.every_rows) for p in idx]
    assert all(torch.equal(x.cursors, y.cursors) for x, y in zip(ref, idx))
    if history:   # (index_pages read each ChunkMeta back and gave histories to the chunks under Lookback; the others' were given here, and left alone)
        assert any(x is not None for x in ref.histories)
        assert all(torch.equal(x, y) if x is not None else not bool(y.any()) for x, y in zip(ref.histories, idx.histories))
    assert comp._dir is not None


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8. the work: the pointer form's kernels and one resolve kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("flags,hist", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spec", ["classic+consecutive1", "classic+lookback", "conv1", "level12"])
def test_a_dir_call_launches_the_pointer_form_s_kernels_and_one_resolve_kernel(L, spec, flags, hist, form):
    b = blob_of(L, spec, 4); c = b.c; src = Source(b)
    ilay = Layout(); itasks = index_tasks(L, c, ilay, 512, hist); ia = ilay.areas(2)
    lay = Layout(); tasks, _ = segment_tasks(L, c, lay, built_index(L, spec, 4, flags, hist), hist); a = lay.areas(2)
    for ts, ar, resolve in ((itasks, ia, "dir_resolve_kernel"), (tasks, a, "dir_resolve_reads_kernel")):
        _, names_p, _ = PI.profiled(L, lambda: run(L, src, ts, ar[0], True, flags, form))
        _, names_d, _ = PI.profiled(L, lambda: run(L, src, ts, ar[1], False, flags, form))
        assert names_d.count(resolve) == 1 and sorted(names_d) == sorted(names_p + [resolve]), (names_p, names_d)
        assert [k for k in names_d if k != resolve] == names_p


def test_the_kernel_time_of_the_resolve_step_and_of_a_dir_call(L):
    """One measurement, no threshold: the 2^18-number i64 Lookback page of test_gpu_lookback_index.py's work test as sixteen segments, kernel time from
    the library's profile -- the pointer form, the _dir form, and the resolve kernel inside it.  The claim is structural (the test above)."""
    n = 1 << 18; seg = n // 16
    c = Call(L, [R.numbers(np.int64, n, 8, period=365)], G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK, max_page_n=n))
    G.check(c.encode())
    b = D.Blob(c, 0); src = Source(b)
    ilay = Layout(); itasks = index_tasks(L, c, ilay, seg, True); iarea = ilay.areas(1)[0]
    lay = Layout(); tasks, page_dst = segment_tasks(L, c, lay, (itasks, iarea, None), True); a = lay.areas(2)
    assert len(tasks) == 16
    ms_ip, _, _ = PI.profiled(L, lambda: run(L, src, itasks, iarea, True, 0, "async"))
    ms_id, names, each = PI.profiled(L, lambda: run(L, src, itasks, iarea, False, 0, "async"))
    res_i = [x for k, x in zip(names, each) if k == "dir_resolve_kernel"]
    ms_p, _, _ = PI.profiled(L, lambda: run(L, src, tasks, a[0], True, 0, "async"))
    ms_d, names, each = PI.profiled(L, lambda: run(L, src, tasks, a[1], False, 0, "async"))
    res_r = [x for k, x in zip(names, each) if k == "dir_resolve_reads_kernel"]
    rows_equal_the_input(c, a[0], page_dst); rows_equal_the_input(c, a[1], page_dst)
    assert len(res_i) == 1 and len(res_r) == 1
    print(f"2^18 i64 Lookback page, sixteen segments in one asynchronous call: pointer form {ms_p:.3f} ms, _dir form {ms_d:.3f} ms, its resolve kernel {res_r[0]:.4f} ms; "
          f"the index call: pointer form {ms_ip:.3f} ms, _dir form {ms_id:.3f} ms, its resolve kernel {res_i[0]:.4f} ms")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. two streams on one workspace
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_streams_share_one_workspace(L):
    """Stream A, behind a delay: the index of a Lookback blob with histories, then its segments.  Stream B, at once: index and segments of a Conv1 blob
    under the flag.  One thread, one workspace; the decoys of every call stay as they were."""
    import torch
    jobs = []
    for spec, flags, hist in (("classic+lookback", 0, True), ("conv1", FLAG, False)):
        b = blob_of(L, spec, 4); c = b.c
        ilay = Layout(); itasks = index_tasks(L, c, ilay, 512, hist); iarea, idecoy = ilay.areas(2)
        lay = Layout(); tasks, page_dst = segment_tasks(L, c, lay, (itasks, iarea, None), hist); area, decoy = lay.areas(2)
        jobs.append(dict(src=Source(b), c=c, flags=flags, itasks=itasks, iarea=iarea, idecoy=idecoy, ilay=ilay, tasks=tasks, area=area, decoy=decoy, lay=lay, page_dst=page_dst,
                         stream=torch.cuda.Stream()))
    torch.cuda.synchronize()
    U.device_delay(jobs[0]["stream"], 10)
    pend = []
    for step in ("index", "reads"):
        for j in jobs:
            ts, ar, dc = (j["itasks"], j["iarea"], j["idecoy"]) if step == "index" else (j["tasks"], j["area"], j["decoy"])
            code, _, p = run(L, j["src"], ts, ar, False, j["flags"], "async", stream=j["stream"], decoy=dc)
            assert code == G.PcoSuccess
            pend.append((ts, p))
    torch.cuda.synchronize()
    for ts, p in pend:
        assert [r[0] for r in tuples(finish(ts, *p, "async"))] == [0] * len(ts)
    for j in jobs:
        rows_equal_the_input(j["c"], j["area"], j["page_dst"])
        assert np.array_equal(j["idecoy"].cpu().numpy(), j["ilay"].image()) and np.array_equal(j["decoy"].cpu().numpy(), j["lay"].image())
