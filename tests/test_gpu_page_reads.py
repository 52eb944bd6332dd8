"""-m gpu: pco_gfx_decompress_page_reads (include/pco_gfx.h section 4f) -- a page read in slices from the cursor the last read left, and from
saved cursors side by side.  Streams come from the library's own wrapped writer and, for what no encoder writes (a delta'd secondary variable, a
table only the 4-chunk walker takes, float-mult on float16), from the test-only generator; truth is the input array.  Every dst and every cursor
sits between canary bytes that are checked after every call; a cursor slot nobody wrote is canary bytes itself."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import gpu_util as U  # noqa: E402
import tans_model as TM  # noqa: E402
import test_gpu_foreign_tables as FT  # noqa: E402  (the walkers' table thresholds, read from the sources)
import test_gpu_page_ranges as R  # noqa: E402  (Stream, write_pages, Pool, run_ranges: the unchanged entry point is the yardstick)
import test_page_reads_abi as A  # noqa: E402  (the cursor's layout restated, the stepped tANS model)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec, PagingSpec  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 0xA5
GUARD = 64
UNWRITTEN = bytes([CANARY]) * 256
N_LONG, N_EVEN = 3000, 2816   # 12 batches with a partial last one; exactly 11


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


class Cursors:
    """k cursor slots in one device tensor, each between guard bytes; everything starts as canary bytes."""
    STRIDE = 256 + GUARD

    def __init__(self, k):
        import torch
        self.k = k
        self.dev = torch.full((GUARD + k * self.STRIDE,), CANARY, dtype=torch.uint8, device="cuda")

    def ptr(self, i):
        return None if i is None else self.dev.data_ptr() + GUARD + i * self.STRIDE

    def put(self, i, words):
        import torch
        o = GUARD + i * self.STRIDE
        self.dev[o: o + 256] = torch.from_numpy(np.array([int(x) for x in words], np.uint64).view(np.uint8).copy()).cuda()

    def snapshot(self):
        """(the slots' bytes, after checking the guards)"""
        import torch
        torch.cuda.synchronize()
        host = self.dev.cpu().numpy()
        mask = np.ones(host.size, bool)
        for i in range(self.k):
            mask[GUARD + i * self.STRIDE: GUARD + i * self.STRIDE + 256] = False
        assert (host[mask] == CANARY).all(), "bytes around a cursor were written"
        return [host[GUARD + i * self.STRIDE: GUARD + i * self.STRIDE + 256].tobytes() for i in range(self.k)]


def words_of(raw):
    return [int(x) for x in np.frombuffer(raw, np.uint64)]


class Call:
    """One pco_gfx_decompress_page_reads call over jobs [(Stream, page bytes or None for the stream's own, first, count, from slot, to slot)]."""

    def __init__(self, L, jobs, cur, form="sync", stream=None):
        import torch
        self.L, self.jobs, self.form = L, jobs, form
        blobs = []; index = {}
        for s, page, *_ in jobs:
            for key, b in ((("m", id(s)), s.meta), (("p", id(s), id(page)), s.page if page is None else page)):
                if key not in index:
                    index[key] = len(blobs); blobs.append(b)
        self.pool = R.Pool(blobs)
        self.spans = []; at = 0
        for s, _, _, count, _, _ in jobs:
            at += GUARD; self.spans.append(at); at += (count * s.nums.dtype.itemsize + 15) // 16 * 16
        self.total = at + GUARD
        self.out = torch.full((self.total,), CANARY, dtype=torch.uint8, device="cuda")
        self.tasks = (G.PageReadTask * len(jobs))()
        for j, (s, page, first, count, fr, to) in enumerate(jobs):
            pg = s.page if page is None else page
            self.tasks[j] = G.PageReadTask(self.pool.ptr(index[("m", id(s))]), len(s.meta), self.pool.ptr(index[("p", id(s), id(page))]), len(pg),
                                           (self.out.data_ptr() + self.spans[j]) if count else None, s.n, first, count, G.DTYPE_BYTE[s.nums.dtype.name], 4,
                                           cur.ptr(fr), cur.ptr(to))
        if form == "sync":
            self.res = (G.TaskResult * len(jobs))()
            self.code = L.pco_gfx_decompress_page_reads(len(jobs), self.tasks, self.res, None, None if stream is None else C.c_void_p(stream.cuda_stream))
        else:
            self.d_res = torch.zeros(len(jobs) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
            if stream is None:   # d_results on a non-blocking stream of the call's own, behind everything set up so far
                torch.cuda.synchronize()
            else:
                stream.wait_stream(torch.cuda.current_stream())
            self.stream = stream or torch.cuda.Stream()
            self.code = L.pco_gfx_decompress_page_reads(len(jobs), self.tasks, None, self.d_res.data_ptr(), C.c_void_p(self.stream.cuda_stream))

    def finish(self):
        """(code, results as a numpy record array, [decoded rows per job, or None where the dst was left untouched]) after checking every canary"""
        import torch
        torch.cuda.synchronize()
        rec = np.frombuffer(bytes(self.res), U.RES_DT).copy() if self.form == "sync" else self.d_res.cpu().numpy().view(U.RES_DT).copy()
        host = self.out.cpu().numpy()
        mask = np.ones(self.total, bool); got = []
        for j, (s, _, _, count, _, _) in enumerate(self.jobs):
            w = s.nums.dtype.itemsize
            mask[self.spans[j]: self.spans[j] + count * w] = False
            raw = host[self.spans[j]: self.spans[j] + count * w]
            got.append(None if count and (raw == CANARY).all() else raw.view(s.nums.dtype))
        assert (host[mask] == CANARY).all(), "bytes outside dst[0 .. count * width) were written"
        return self.code, rec, got


def run_reads(L, jobs, cur, form="sync"):
    return Call(L, jobs, cur, form).finish()


def check_ok(jobs, rec, got, what=""):
    for j, (s, page, first, count, _, _) in enumerate(jobs):
        tag = (what, s.label, first, count)
        assert rec["status"][j] == G.ST_OK, (tag, int(rec["status"][j]))
        assert rec["n_out"][j] == count and rec["aux"][j] == 0, tag
        last = count > 0 and (first + count + 255) // 256 >= (s.n + 255) // 256
        assert rec["consumed"][j] == (len(s.page if page is None else page) if last else 0), (tag, int(rec["consumed"][j]))
        if count:
            assert got[j] is not None and U.bits_equal(got[j], s.nums[first: first + count]), tag


# ---------------------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------------------
def per(**kw):
    return G.make_config(enable_8_bit=True, max_page_n=1 << 20, **kw)


def from_generator(label, x, **kw):
    meta, pages = O.test_encode(x, pages=[x.size], **kw)
    return R.Stream(label, x, meta, pages[0])


def k4_table_log():
    """the smallest ans_size_log whose table (4 bytes a state, 8 for bin 0's offset bits) the 8-chunk walker's slice cannot hold and the 4-chunk walker's can"""
    a = next(a for a in range(15) if (4 << a) + 8 > FT.K8_TABLE_BYTES)
    assert (4 << a) + 8 <= FT.K4_TABLE_BYTES
    return a


@pytest.fixture(scope="module")
def route1(L):
    """Every stream of the two-kernel route, written once: [Stream] with .kind, .order (primary delta order) and .two (a secondary variable)."""
    out = []

    def add(kind, order, two, cfg, items):
        for s in R.write_pages(L, [(f"{kind} {a.dtype.name} n={a.size}", a) for a in items], cfg):
            s.kind, s.order, s.two = kind, order, two
            out.append(s)

    num = R.numbers
    add("classic", 0, False, per(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP),
        [num(dt, N_LONG, 3 + i) for i, dt in enumerate((np.uint8, np.uint16, np.uint32, np.uint64, np.int64))] + [num(np.uint32, N_EVEN, 9), num(np.uint64, N_EVEN, 10)])
    add("consecutive1", 1, False, per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), [num(np.uint32, N_LONG, 11), num(np.int64, N_EVEN, 12), num(np.uint8, N_LONG, 13)])
    add("consecutive2", 2, False, per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=2), [num(np.uint16, N_LONG, 14), num(np.uint64, N_EVEN, 15)])
    add("consecutive7", 7, False, per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7), [num(np.uint32, N_EVEN, 16), num(np.int64, N_LONG, 17)])
    add("int_mult", 0, True, per(mode=G.MODE_TRY_INT_MULT, mode_u64=10, delta=G.DELTA_NOOP), [(num(np.uint64, N_LONG, 18) // 10 * 10 + 3).astype(np.uint64)])
    add("int_mult+delta", 1, True, per(mode=G.MODE_TRY_INT_MULT, mode_u64=10, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1),
        [(num(dt, n, 19) // 10 * 10 + 3).astype(dt) for dt, n in ((np.uint32, N_LONG), (np.int64, N_EVEN))])
    fm = lambda dt, n: (np.cumsum(np.random.default_rng(n).integers(-5, 7, n)) / 100.0).astype(dt)   # noqa: E731
    add("float_mult", 0, True, per(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=G.DELTA_NOOP), [fm(np.float64, N_LONG)])
    add("float_mult+delta", 1, True, per(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), [fm(np.float32, N_EVEN), fm(np.float64, N_EVEN)])
    add("float_quant", 0, True, per(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=8, delta=G.DELTA_NOOP),
        [np.random.default_rng(n).normal(size=n).astype(dt) for dt, n in ((np.float32, N_LONG), (np.float64, N_EVEN))])
    # what no encoder writes: float-mult on float16, a delta'd secondary variable, a table only the 4-chunk walker takes
    h = (np.random.default_rng(5).integers(-2000, 2000, N_LONG) * 0.25).astype(np.float16)
    for s, kind, order in ((from_generator("float_mult float16", h, mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25), "float_mult16", 0),
                           (from_generator("secondary delta float32", fm(np.float32, N_LONG), mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=O.TE_DELTA_CONSECUTIVE, order=1,
                                           secondary_uses_delta=True), "secondary_delta", 1),
                           (from_generator("k4 table uint32", np.random.default_rng(6).integers(0, 5000, N_LONG).astype(np.uint32), mode=O.MODE_CLASSIC, tbl_vars=O.TBL_PRIMARY,
                                           tbl_ans_size_log=k4_table_log(), tbl_n_bins=65, tbl_seed=10), "k4", 0)):
        s.kind, s.order, s.two = kind, order, kind != "k4"
        out.append(s)
    return out


def test_the_streams_are_what_they_are_called(L, route1):
    kinds = {}
    for s in route1:
        i = R.meta_info(L, s)
        kinds.setdefault(s.kind, set()).add((i.mode_kind, i.delta_kind, i.delta_order if i.delta_kind == 1 else 0, i.present[2]))
        if s.kind == "secondary_delta":
            assert i.secondary_uses_delta == 1 and i.present[2] == 1
        if s.kind == "k4":
            assert FT.K8_TABLE_BYTES < (4 << i.ans_size_log[1]) + 8 <= FT.K4_TABLE_BYTES
    assert kinds["classic"] == {(0, 0, 0, 0)} and kinds["consecutive1"] == {(0, 1, 1, 0)} and kinds["consecutive2"] == {(0, 1, 2, 0)} and kinds["consecutive7"] == {(0, 1, 7, 0)}
    assert kinds["int_mult"] == {(1, 0, 0, 1)} and kinds["int_mult+delta"] == {(1, 1, 1, 1)} and kinds["float_mult"] == {(2, 0, 0, 1)} and kinds["float_mult+delta"] == {(2, 1, 1, 1)}
    assert kinds["float_quant"] == {(3, 0, 0, 1)} and kinds["float_mult16"] == {(2, 0, 0, 1)} and kinds["secondary_delta"] == {(2, 1, 1, 1)} and kinds["k4"] == {(0, 0, 0, 0)}
    assert {s.nums.dtype.name for s in route1} >= {"uint8", "uint16", "uint32", "uint64", "int64", "float16", "float32", "float64"}
    assert {s.n for s in route1} == {N_LONG, N_EVEN}


# ---------------------------------------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------------------------------------
CHAINS = ["256", "512", "mixed", "one"]


def chain_sizes(n, chain):
    if chain in ("256", "512"):
        k = int(chain)
        return [k] * (n // k) + ([n % k] if n % k else [])
    return [256, 1024, n - 1280] if chain == "mixed" else [n]


def whole_pages(L, streams):
    """pco_gfx_decompress_pages over every stream: [numbers]"""
    import torch
    pool = R.Pool([b for s in streams for b in (s.meta, s.page)])
    outs = [torch.zeros(s.n * s.nums.dtype.itemsize + 64, dtype=torch.uint8, device="cuda") for s in streams]
    t = (G.PageTask * len(streams))(*[G.PageTask(pool.ptr(2 * i), len(s.meta), pool.ptr(2 * i + 1), len(s.page), outs[i].data_ptr(), s.n, G.DTYPE_BYTE[s.nums.dtype.name], 4)
                                      for i, s in enumerate(streams)])
    res = (G.TaskResult * len(streams))()
    G.check(L.pco_gfx_decompress_pages(len(streams), t, res, None, None))
    return [o[: s.n * s.nums.dtype.itemsize].cpu().numpy().view(s.nums.dtype) for o, s in zip(outs, streams)]


def walk_chains(L, streams, form, want_kind=A.FULL):
    """Every stream through every chain, step t of all of them in call t.  Chain "256" reads and writes ONE slot (to == from); the others
    alternate between two.  Returns {(stream index, row): the cursor's 256 bytes}, the same bytes whichever chain reached the row."""
    lanes = [(si, c) for si in range(len(streams)) for c in CHAINS]
    cur = Cursors(2 * len(lanes))
    sizes = {ln: chain_sizes(streams[ln[0]].n, ln[1]) for ln in lanes}
    pos = {ln: 0 for ln in lanes}; parts = {ln: [] for ln in lanes}
    seen = {}
    for t in range(max(len(v) for v in sizes.values())):
        jobs = []; who = []
        for k, ln in enumerate(lanes):
            if t >= len(sizes[ln]):
                continue
            a, b = (2 * k, 2 * k) if ln[1] == "256" else (2 * k + (t + 1) % 2, 2 * k + t % 2)
            jobs.append((streams[ln[0]], None, pos[ln], sizes[ln][t], None if t == 0 else a, b)); who.append((ln, b))
        code, rec, got = run_reads(L, jobs, cur, form)
        assert code == G.PcoSuccess, L.pco_gfx_last_error()
        check_ok(jobs, rec, got, (form, t))   # (consumed == page_len on a chain's last read only)
        slots = cur.snapshot()
        for (ln, b), job, g in zip(who, jobs, got):
            s = streams[ln[0]]
            parts[ln].append(g); pos[ln] += job[3]
            row = min((pos[ln] + 255) // 256 * 256, s.n)
            c = A.unpack_cursor(words_of(slots[b]))
            assert (c["version"], c["kind"], c["row"], c["page_n"], c["dtype"]) == (A.VERSION, want_kind, row, s.n, G.DTYPE_BYTE[s.nums.dtype.name]), (s.label, ln[1], t, c)
            assert c["tail"] == [0] * 6
            assert seen.setdefault((ln[0], row), slots[b]) == slots[b], ("the cursor of a row differs between two chains", s.label, ln[1], row)
    for ln in lanes:
        assert pos[ln] == streams[ln[0]].n and U.bits_equal(np.concatenate(parts[ln]), streams[ln[0]].nums), (streams[ln[0]].label, ln[1])
    return seen


@pytest.fixture(scope="module")
def walked(L, route1):
    return walk_chains(L, route1, "sync")


def test_chains_concatenate_to_the_input_and_to_the_whole_page_decode(L, route1, walked):
    for s, w in zip(route1, whole_pages(L, route1)):
        assert U.bits_equal(w, s.nums), s.label   # (walk_chains compared every chain with the input)
    rows = {si: sorted(r for i, r in walked if i == si) for si in range(len(route1))}
    for si, s in enumerate(route1):
        assert rows[si] == [min(r + 256, s.n) for r in range(0, s.n, 256)], s.label


def test_the_asynchronous_form_reaches_the_same_cursors(L, route1, walked):
    again = walk_chains(L, route1, "async")
    assert again.keys() == walked.keys() and all(again[k] == walked[k] for k in walked)


def test_cursor_fields_are_the_tans_model_s(route1, walked):
    """Classic pages without delta: row, bit position and the four states of the primary at every batch boundary are what tests/tans_model.py,
    stepped batch by batch, says; everything else in the cursor is zero."""
    n_checked = 0
    for si, s in enumerate(route1):
        if s.kind != "classic":
            continue
        body, marks, latents, size_log = A.model_cursors(s.meta, s.page, s.n, s.nums.dtype.itemsize * 8)
        assert [int(v) for v in TM.to_latent(s.nums)] == latents
        for row, bit, states in marks:
            c = A.unpack_cursor(words_of(walked[(si, row)]))
            assert (c["row"], c["bit"], c["states"][1]) == (row, bit, list(states)), (s.label, row, c)
            assert c["states"][0] == [0] * 4 and c["states"][2] == [0] * 4 and c["moments"] == [[0] * 8, [0] * 8] and bit >= body
            n_checked += 1
    assert n_checked >= 7 * 11


def test_moments_are_the_differences_at_the_row(route1, walked):
    """Under Classic with a consecutive delta of order k the state in front of row r is the 0th .. (k - 1)th forward differences of the latents
    at r (delta/consecutive.rs:35-50); entries beyond the order are zero."""
    n_checked = 0
    for si, s in enumerate(route1):
        if not s.kind.startswith("consecutive"):
            continue
        bits = s.nums.dtype.itemsize * 8
        lat = [int(v) for v in TM.to_latent(s.nums)]
        for row in range(256, s.n, 256):
            if row + s.order > s.n:
                continue
            d = lat[row: row + s.order]; want = []
            for _ in range(s.order):
                want.append(d[0]); d = [(b - a) % (1 << bits) for a, b in zip(d, d[1:])]
            c = A.unpack_cursor(words_of(walked[(si, row)]))
            assert c["moments"] == [want + [0] * (8 - s.order), [0] * 8], (s.label, row)
            n_checked += 1
    assert n_checked > 50


# ---------------------------------------------------------------------------------------------------------------------------------------
# skipping ahead, aliasing, reuse
# ---------------------------------------------------------------------------------------------------------------------------------------
def pick(route1, kind, n=N_LONG):
    return next((i, s) for i, s in enumerate(route1) if s.kind == kind and s.n == n)


@pytest.mark.parametrize("form", ["sync", "async"])
def test_skipping_ahead_from_a_cursor_far_behind_the_read(L, route1, walked, form):
    picks = [pick(route1, k) for k in ("classic", "consecutive1", "consecutive2", "int_mult+delta", "float_quant", "secondary_delta", "k4")]
    cur = Cursors(2 * len(picks))
    for k, (si, s) in enumerate(picks):
        cur.put(2 * k, words_of(walked[(si, 512)]))
    jobs = [(s, None, 1500, 700, 2 * k, 2 * k + 1) for k, (si, s) in enumerate(picks)]
    code, rec, got = run_reads(L, jobs, cur, form)
    assert code == G.PcoSuccess
    check_ok(jobs, rec, got, form)
    slots = cur.snapshot()
    for k, (si, s) in enumerate(picks):
        assert slots[2 * k] == walked[(si, 512)] and slots[2 * k + 1] == walked[(si, 2304)], s.label   # ceil(2200 / 256) * 256


def test_aliasing_and_reuse(L, route1, walked):
    si, s = pick(route1, "consecutive1")
    cur = Cursors(4)
    cur.put(0, words_of(walked[(si, 512)])); cur.put(1, words_of(walked[(si, 512)])); cur.put(2, words_of(walked[(si, s.n)]))
    # to == from; to == NULL; one cursor in two tasks of one call
    jobs = [(s, None, 512, 512, 0, 0), (s, None, 600, 100, 1, None), (s, None, 512, 2488, 1, None)]
    code, rec, got = run_reads(L, jobs, cur)
    assert code == G.PcoSuccess
    check_ok(jobs, rec, got)
    slots = cur.snapshot()
    assert slots[0] == walked[(si, 1024)] and slots[1] == walked[(si, 512)] and slots[3] == UNWRITTEN
    # ... and the same cursor again in two later calls
    for first, count in ((512, 256), (1000, 1000)):
        jobs = [(s, None, first, count, 1, 3)]
        code, rec, got = run_reads(L, jobs, cur)
        check_ok(jobs, rec, got)
        slots = cur.snapshot()
        assert slots[1] == walked[(si, 512)] and slots[3] == walked[(si, min((first + count + 255) // 256 * 256, s.n))]
    # a finished cursor: nothing left to read is fine and writes nothing; more is refused by the host as before
    cur = Cursors(4); cur.put(2, words_of(walked[(si, s.n)]))
    jobs = [(s, None, s.n, 0, 2, 3), (s, None, 100, 0, None, 1)]
    code, rec, got = run_reads(L, jobs, cur)
    assert code == G.PcoSuccess and (rec["status"] == 0).all() and (rec["n_out"] == 0).all() and (rec["consumed"] == 0).all()
    slots = cur.snapshot()
    assert slots[3] == UNWRITTEN and slots[1] == UNWRITTEN and slots[2] == walked[(si, s.n)]
    c = Call(L, [(s, None, s.n, 1, 2, 3)], cur)
    assert c.code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT
    assert cur.snapshot()[3] == UNWRITTEN


# ---------------------------------------------------------------------------------------------------------------------------------------
# route 2: position-only cursors
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def route2(L):
    import torch
    out = R.write_pages(L, [("lookback uint32", R.numbers(np.uint32, N_LONG, 7, period=365)), ("lookback int64", R.numbers(np.int64, N_EVEN, 8, period=365))],
                        per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK))
    d = np.random.default_rng(1).integers(0, 1 << 15, 50).astype(np.uint32)[np.random.default_rng(2).integers(0, 50, N_LONG)]
    out += R.write_pages(L, [("dict uint32", d)], per(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True))
    kinds = [R.meta_info(L, s) for s in out]
    assert kinds[0].delta_kind == 2 and kinds[1].delta_kind == 2 and kinds[2].mode_kind == 4
    # 3000 distinct values, 21 apart and sixteen times each, at level 12 (up to 4096 bins) in six pages of 8000: at that many repeats a bin of its own
    # saves a value more offset bits than its metadata costs, so the table has far more than the walkers' 256 bins and they hand the pages back
    x = (np.arange(N_LONG, dtype=np.uint16) * 21 + 7)[np.random.default_rng(12).integers(0, N_LONG, 48000)]
    cc = paged.compress_chunks([torch.from_numpy(x.view(np.int16)).cuda()], ChunkConfig(compression_level=12, mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.no_op()),
                               page_sizes=[[8000] * 6])
    pieces = cc.directory; blob = cc.blob.cpu().numpy()
    meta = blob[pieces[0].offset: pieces[0].offset + pieces[0].length].tobytes()
    for p in pieces[1:]:
        out.append(R.Stream(f"level12 page {p.piece}", x.view(np.int16)[8000 * (p.piece - 1): 8000 * p.piece], meta, blob[p.offset: p.offset + p.length].tobytes()))
    assert R.meta_info(L, out[-1]).n_bins[1] > 256
    return out


@contextlib.contextmanager
def small_passes():
    """PCO_GFX_WORKSPACE_GB=0.0001 inside the block: 100 KB of scratch per pass, so the scratch route of a synchronous call runs in passes."""
    os.environ["PCO_GFX_WORKSPACE_GB"] = "0.0001"
    try:
        yield
    finally:
        os.environ.pop("PCO_GFX_WORKSPACE_GB", None)


@pytest.mark.parametrize("form", ["sync", "async", "sync in passes"])
def test_route_2_chains_equal_the_input_with_position_only_cursors(L, route2, form):
    assert len(route2) == 9
    if form == "sync in passes":   # 36 tasks of up to 3000 numbers a call: several passes each, and the cursors of the unrestricted run
        whole = walk_chains(L, route2, "sync", want_kind=A.POSITION)
        with small_passes():
            seen = walk_chains(L, route2, "sync", want_kind=A.POSITION)
        assert seen.keys() == whole.keys() and all(seen[k] == whole[k] for k in whole)
    else:
        seen = walk_chains(L, route2, form, want_kind=A.POSITION)
    for raw in seen.values():
        assert sum(1 for w in words_of(raw) if w) == 3   # version | kind, row, page_n | dtype: nothing else


@pytest.mark.parametrize("form", ["sync", "async", "sync in passes"])
def test_lookback_with_a_delta_d_secondary_variable_in_two_reads(L, form):
    """The stream of test_gpu_page_ranges.py's test of the same name, read in two reads from a position-only cursor at row 1024, ten times side by
    side.  Synchronous: a second history buffer, taken when asked for (18 KB and 24 KB a task with it, ten tasks a call: under 100 KB a pass that
    round runs in passes too); asynchronous: UNSUPPORTED, dst and `to` untouched."""
    x = (np.cumsum(np.random.default_rng(3).integers(-5, 7, 3000)) / 4.0).astype(np.float32)
    meta, pages = O.test_encode(x, pages=[x.size], mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1,
                                secondary_uses_delta=True, lookback_seed=5)
    s = R.Stream("lookback+secondary float32", x, meta, pages[0])
    info = R.meta_info(L, s)
    assert info.delta_kind == 2 and info.secondary_uses_delta == 1 and info.present[2] == 1
    lanes = 10; dtype = G.DTYPE_BYTE["float32"]
    cur = Cursors(4 * lanes)   # a lane's slots: the first read's from and to, the second read's from (asynchronous only) and to
    for k in range(lanes):
        cur.put(4 * k, A.pack_cursor(A.POSITION, 1024, 0, s.n, dtype))
    first = [(s, None, 1100, 700, 4 * k, 4 * k + 1) for k in range(lanes)]   # rows [1100, 1800): `to` in front of row 2048
    if form == "async":   # (no first read leaves a cursor: the second reads start from written-out ones, in the same call)
        for k in range(lanes):
            cur.put(4 * k + 2, A.pack_cursor(A.POSITION, 2048, 0, s.n, dtype))
        before = cur.snapshot()
        jobs = first + [(s, None, 2100, 900, 4 * k + 2, 4 * k + 3) for k in range(lanes)] + [(s, None, 2000, 0, 0, 1)]
        code, rec, got = run_reads(L, jobs, cur, "async")
        assert code == G.PcoSuccess
        assert list(rec["status"]) == [G.ST_UNSUPPORTED] * (2 * lanes) + [G.ST_OK] and (rec["n_out"] == 0).all()
        assert all(g is None for g in got[:-1]), "dst was written"
        assert cur.snapshot() == before and all(before[4 * k + j] == UNWRITTEN for k in range(lanes) for j in (1, 3))
        return
    second = [(s, None, 2100, 900, 4 * k + 1, 4 * k + 3) for k in range(lanes)]   # rows [2100, 3000): `to` at the page's end
    for jobs, row in ((first, 2048), (second, s.n)):
        if form == "sync in passes":
            with small_passes():
                code, rec, got = run_reads(L, jobs, cur, "sync")
        else:
            code, rec, got = run_reads(L, jobs, cur, "sync")
        assert code == G.PcoSuccess, L.pco_gfx_last_error()
        check_ok(jobs, rec, got, form)
        slots = cur.snapshot()
        for _, _, _, _, _, to in jobs:
            assert words_of(slots[to]) == A.pack_cursor(A.POSITION, row, 0, s.n, dtype), (form, row)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the verdict, on the device
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_a_refused_cursor_refuses_its_task_alone(L, route1, route2, walked, form):
    si, s = pick(route1, "float_mult+delta", N_EVEN)
    info = R.meta_info(L, s)
    base = A.unpack_cursor(words_of(walked[(si, 512)]))
    ci, cs = next((i, x) for i, x in enumerate(route1) if x.kind == "classic" and x.nums.dtype == np.uint32 and x.n == N_LONG)
    body = A.model_cursors(cs.meta, cs.page, cs.n, cs.nums.dtype.itemsize * 8)[0]
    assert body > 0   # (four states of ans_size_log bits each, padded to a byte: a bit position in front of them exists)
    cbase = A.unpack_cursor(words_of(walked[(ci, 512)]))

    def edit(b=base, **kw):
        d = {k: b[k] for k in ("kind", "row", "bit", "page_n", "dtype", "states", "moments", "version")}
        d.update(kw)
        return A.pack_cursor(**d)

    def state(v, j, x):
        st = [list(r) for r in base["states"]]; st[v][j] = x
        return edit(states=st)

    lb = route2[0]
    rows = [("version", s, edit(version=2), 600), ("kind", s, edit(kind=A.POSITION), 600), ("kind 0", s, edit(kind=0), 600), ("page_n", s, edit(page_n=s.n - 1), 600),
            ("dtype", s, edit(dtype=base["dtype"] ^ 3), 600), ("at > first", s, edit(row=768), 600), ("at unaligned", s, edit(row=300), 600),
            ("bit before the body", cs, edit(cbase, bit=body - 1), 600), ("bit beyond the page", s, edit(bit=8 * len(s.page) + 1), 600),
            ("primary state 2^asl", s, state(1, 2, 1 << info.ans_size_log[1]), 600), ("secondary state 2^asl", s, state(2, 0, 1 << info.ans_size_log[2]), 600),
            ("a state for a variable the page does not have", s, state(0, 3, 1), 600),
            ("full state on a page of route 2", lb, edit(page_n=lb.n, dtype=G.DTYPE_BYTE[lb.nums.dtype.name]), 600),
            ("position only, at > first, on route 2", lb, A.pack_cursor(A.POSITION, 768, 0, lb.n, G.DTYPE_BYTE[lb.nums.dtype.name]), 600)]
    cur = Cursors(2 * len(rows) + 4)
    jobs = []
    for k, (_, st, words, first) in enumerate(rows):
        cur.put(2 * k, words); jobs.append((st, None, first, 300, 2 * k, 2 * k + 1))
    g0 = 2 * len(rows)
    cur.put(g0, words_of(walked[(si, 512)])); cur.put(g0 + 2, A.pack_cursor(A.POSITION, 512, 0, lb.n, G.DTYPE_BYTE[lb.nums.dtype.name]))
    good = [(s, None, 600, 300, g0, g0 + 1), (lb, None, 600, 300, g0 + 2, g0 + 3), (cs, None, 0, cs.n, None, None)]
    before = cur.snapshot()
    code, rec, got = run_reads(L, jobs[:5] + good[:1] + jobs[5:] + good[1:], cur, form)
    order = list(range(5)) + [len(rows)] + list(range(5, len(rows))) + [len(rows) + 1, len(rows) + 2]   # position in the call -> index into rows + good
    if form == "sync":
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT
    after = cur.snapshot()
    for at, k in enumerate(order):
        if k < len(rows):
            assert (rec["status"][at], rec["n_out"][at], rec["consumed"][at], rec["aux"][at]) == (G.ST_INVALID_ARGUMENT, 0, 0, 0), rows[k][0]
            assert got[at] is None, ("dst was written", rows[k][0])
            assert after[2 * k] == before[2 * k] and after[2 * k + 1] == UNWRITTEN, rows[k][0]
    gj = [order.index(len(rows) + i) for i in range(3)]
    check_ok(good, rec[gj], [got[j] for j in gj], form)
    assert after[g0 + 1] == walked[(si, 1024)] and A.unpack_cursor(words_of(after[g0 + 3]))["row"] == 1024


def test_a_cursor_of_another_page_of_the_same_shape_stays_inside_dst(L, route1, walked):
    """Status OK or INSUFFICIENT_DATA, canaries intact, nothing else asserted: the verdict cannot know whose cursor it is, and does not have to."""
    (ai, a), (bi, b) = [(i, s) for i, s in enumerate(route1) if s.kind == "classic" and s.nums.dtype == np.uint32 and s.n == N_LONG][0], pick(route1, "k4")
    assert a.nums.dtype == b.nums.dtype and a.n == b.n and a.page != b.page
    c = A.unpack_cursor(words_of(walked[(bi, 512)]))
    info = R.meta_info(L, a)
    cur = Cursors(2)
    cur.put(0, A.pack_cursor(A.FULL, 512, min(c["bit"], 8 * len(a.page)), a.n, c["dtype"], [[0] * 4, [x % (1 << info.ans_size_log[1]) for x in c["states"][1]], [0] * 4]))
    code, rec, got = run_reads(L, [(a, None, 512, 2488, 0, 1)], cur)
    cur.snapshot()
    assert rec["status"][0] in (G.ST_OK, G.ST_INSUFFICIENT_DATA)


def test_a_page_cut_inside_the_read_and_behind_it(L, route1, walked):
    """Statuses, n_out and consumed equal those of pco_gfx_decompress_page_ranges on the same page, first and count."""
    for kind in ("consecutive1", "float_mult", "classic"):
        si, s = pick(route1, kind)
        page = s.page[: len(s.page) // 2]
        ok_nums, err, in_meta = O.wrapped_page_prefix(s.meta, page, s.nums.dtype, s.n)
        w = ok_nums.size
        assert not in_meta and err == G.ST_INSUFFICIENT_DATA and w % 256 == 0 and 512 <= w < s.n
        spans = [(256, 256), (w - 256, 256), (300, w - 300), (w, 1), (256, s.n - 256), (s.n - 1, 1), (w - 1, 2)]
        cur = Cursors(2)
        cur.put(0, words_of(walked[(si, 256)]))
        for form in ("sync", "async"):
            for fr in (0, None):
                jobs = [(s, page, f, c, fr, None) for f, c in spans]
                code, rec, got = run_reads(L, jobs, cur, form)
                rcode, rrec, rgot = R.run_ranges(L, [(s, page, f, c) for f, c in spans], form)
                assert code == rcode and (rec == rrec).all(), (kind, form, fr, rec, rrec)
                assert list(rec["status"]) == [0, 0, 0, 2, 2, 2, 2]
                for j in range(3):
                    assert U.bits_equal(got[j], rgot[j]) and U.bits_equal(got[j], s.nums[spans[j][0]: spans[j][0] + spans[j][1]])
        assert cur.snapshot()[1] == UNWRITTEN


# ---------------------------------------------------------------------------------------------------------------------------------------
# wider calls
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_one_call_mixing_every_spec_with_one_bad_task(L, route1, route2, walked, form):
    rng = np.random.default_rng(5)
    big = [s for s in route2 if s.n > 1280]
    cur = Cursors(2 * (len(route1) + len(big)))
    jobs = []
    for k, s in enumerate(route1 + big):
        row = int(rng.integers(1, s.n // 256)) * 256
        cur.put(2 * k, words_of(walked[(k, row)]) if k < len(route1) else A.pack_cursor(A.POSITION, row, 0, s.n, G.DTYPE_BYTE[s.nums.dtype.name]))
        first = row + int(rng.integers(0, 300)); first = min(first, s.n - 1)
        jobs.append((s, None, first, int(rng.integers(1, s.n - first + 1)), 2 * k, 2 * k + 1))
        jobs.append((s, None, int(rng.integers(0, s.n)), 0, None, None))
    vi, victim = pick(route1, "consecutive2")
    bad_at = 2 * vi
    jobs[bad_at] = (victim, victim.page[: len(victim.page) // 3], victim.n - 10, 10, None, 2 * vi + 1)   # (from the page's start: the cut page ends in front of the cursor's bit)
    code, rec, got = run_reads(L, jobs, cur, form)
    if form == "sync":
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INSUFFICIENT_DATA
    assert rec["status"][bad_at] == G.ST_INSUFFICIENT_DATA and rec["n_out"][bad_at] == 0
    keep = [j for j in range(len(jobs)) if j != bad_at]
    check_ok([jobs[j] for j in keep], rec[keep], [got[j] for j in keep], form)
    slots = cur.snapshot()
    assert slots[2 * vi + 1] == UNWRITTEN
    for k, s in enumerate(route1):
        if k != vi:
            f, c = jobs[2 * k][2], jobs[2 * k][3]
            assert slots[2 * k + 1] == walked[(k, min((f + c + 255) // 256 * 256, s.n))], s.label


def test_two_streams_on_one_workspace(L, route1, walked):
    import torch
    half = len(route1) // 2
    cur = Cursors(2 * len(route1))
    for k in range(len(route1)):
        cur.put(2 * k, words_of(walked[(k, 256)]))
    jobs = [(s, None, 256, s.n - 256, 2 * k, 2 * k + 1) for k, s in enumerate(route1)]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    U.device_delay(sa)   # stream A is still busy when stream B's call arrives
    a = Call(L, jobs[:half], cur, "async", sa)
    b = Call(L, jobs[half:], cur, "async", sb)
    for call, part in ((a, jobs[:half]), (b, jobs[half:])):
        code, rec, got = call.finish()
        assert code == G.PcoSuccess
        check_ok(part, rec, got)
    slots = cur.snapshot()
    assert all(slots[2 * k + 1] == walked[(k, s.n)] for k, s in enumerate(route1))


def test_the_three_paged_functions_against_numpy(L):
    import torch
    a = (np.cumsum(np.random.default_rng(1).integers(-5, 7, 4500)) / 4.0).astype(np.float32)
    b = U.synth("c4", 10000)
    c = U.synth("c2", 9000).view(np.int64)
    arrays = [a, b, c]; names = ["float32", "int64", "int64"]
    blobs = []
    for x, delta, sizes in ((a, DeltaSpec.try_consecutive(1), [1000, 3000, 500]), (b, DeltaSpec.try_lookback(), None), (c, DeltaSpec.try_consecutive(2), [4096, 4904])):
        cfg = ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=delta, paging_spec=PagingSpec.equal_pages_up_to(4096))
        blobs.append(paged.compress_chunks([torch.from_numpy(x).cuda()], cfg, page_sizes=[sizes]))
    for k, (x, cc) in enumerate(zip(arrays, blobs)):
        d = cc.directory
        for sizes in ([256] * 3 + [1024, 512], [x.size], [2048, 256]):
            r = paged.ChunkReader(cc.blob, d, [names[k]], 0)
            got = [r.read(n).cpu().numpy() for n in sizes]
            got.append(r.read(x.size - r.pos).cpu().numpy())
            assert r.pos == x.size and U.bits_equal(np.concatenate(got), x), (names[k], sizes)
            assert r.read(0).numel() == 0
        r = paged.ChunkReader(cc.blob, d, [names[k]], 0)
        with pytest.raises(ValueError):
            r.read(100)
        with pytest.raises(ValueError):
            r.read(x.size + 256)
        for every in (256, 1024):
            saved = paged.save_cursors(cc.blob, d, [names[k]], every)
            assert [pc.cursors.shape[0] for pc in saved] == [(p.n - 1) // every for p in d if p.piece]
            got = paged.decompress_chunks_from(cc.blob, d, [names[k]], saved)
            assert len(got) == 1 and U.bits_equal(got[0].cpu().numpy(), x), (names[k], every)
    with pytest.raises(ValueError):
        paged.save_cursors(blobs[0].blob, blobs[0].directory, ["float32"], 100)
    # the segments really are tasks of ONE call, and of the resume kernels
    saved = paged.save_cursors(blobs[2].blob, blobs[2].directory, ["int64"], 1024)
    L.pco_gfx_profile_begin()
    paged.decompress_chunks_from(blobs[2].blob, blobs[2].directory, ["int64"], saved)
    kernels = U.profile_names(L)
    assert sorted(kernels) == ["dec_expand_resume_kernel<u64>", "dec_walk4_resume_kernel<u64>", "dec_walk_resume_kernel<u64>", "reads_rows_kernel"], kernels


# ---------------------------------------------------------------------------------------------------------------------------------------
# work follows the slice
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_work_of_a_read_follows_its_slice(L):
    """One u64 delta-1 page of 2^20 numbers, as in test_the_work_of_a_range_follows_its_prefix.  (a) rows [15 * 2^16, 2^20) from a saved cursor walk
    256 of the page's 4096 batches, where the same rows through pco_gfx_decompress_page_ranges walk all of them; (b) all sixteen segments from
    sixteen cursors in ONE call are sixteen chains of 256 batches side by side in two walker waves, against one chain of 4096 in
    pco_gfx_decompress_pages.  Both are 1/16 by construction; 1/4 leaves room for launch floors, the table build and a busy device.  The
    yardsticks are the two unchanged entry points."""
    import torch
    n = 1 << 20; seg = 1 << 16
    s = R.write_pages(L, [("c2 2^20", U.synth("c2", n))], G.make_config(mode=1, delta=2, delta_order=1, max_page_n=n))[0]
    pool = R.Pool([s.meta, s.page])
    whole = torch.zeros(n * 8 + 64, dtype=torch.uint8, device="cuda")
    part = torch.zeros(seg * 8 + 64, dtype=torch.uint8, device="cuda")
    curs = torch.zeros((16, 256), dtype=torch.uint8, device="cuda")   # row k: the cursor in front of row k * 2^16 (row 0 unused)
    cptr = lambda k: curs.data_ptr() + 256 * k   # noqa: E731

    def reads(tasks):
        t = (G.PageReadTask * len(tasks))(*tasks)
        res = (G.TaskResult * len(tasks))()
        G.check(L.pco_gfx_decompress_page_reads(len(tasks), t, res, None, None))
        return res

    def task(dst, first, count, fr, to):
        return G.PageReadTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), dst, n, first, count, 2, 4, fr, to)

    for k in range(15):   # one walk of the page, a cursor every 2^16 rows
        reads([task(part.data_ptr(), k * seg, seg, cptr(k) if k else None, cptr(k + 1))])

    def last_from_cursor(k=1):
        res = reads([task(part.data_ptr(), 15 * seg, seg, cptr(15), None)] * k)
        assert all(r.n_out == seg and r.consumed == len(s.page) for r in res)

    def last_as_range(k=1):
        t = (G.PageRangeTask * k)(*[G.PageRangeTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), part.data_ptr(), n, 15 * seg, seg, 2, 4)] * k)
        res = (G.TaskResult * k)()
        G.check(L.pco_gfx_decompress_page_ranges(k, t, res, None, None))

    def sixteen():
        reads([task(whole.data_ptr() + 8 * k * seg, k * seg, seg, cptr(k) if k else None, None) for k in range(16)])

    def one_page():
        t = (G.PageTask * 1)(G.PageTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), whole.data_ptr(), n, 2, 4))
        res = (G.TaskResult * 1)()
        G.check(L.pco_gfx_decompress_pages(1, t, res, None, None))

    ms_range = R.profiled_ms(L, last_as_range)
    part.zero_()
    ms_read = R.profiled_ms(L, last_from_cursor)
    assert U.bits_equal(part[: seg * 8].cpu().numpy().view(np.uint64), s.nums[15 * seg:])
    ms_page = R.profiled_ms(L, one_page)
    whole.zero_()
    ms_sixteen = R.profiled_ms(L, sixteen)
    assert U.bits_equal(whole[: n * 8].cpu().numpy().view(np.uint64), s.nums)
    print(f"(a) rows [15 * 2^16, 2^20): as a range {ms_range:.3f} ms, from a saved cursor {ms_read:.3f} ms; (b) the page: pco_gfx_decompress_pages {ms_page:.3f} ms, "
          f"sixteen segments in one call {ms_sixteen:.3f} ms")
    torch.cuda.synchronize(); L.pco_gfx_release_workspace()
    last_from_cursor(2048); ws_read = L.pco_gfx_workspace_bytes()
    torch.cuda.synchronize(); L.pco_gfx_release_workspace()
    last_as_range(2048); ws_range = L.pco_gfx_workspace_bytes()
    torch.cuda.synchronize(); L.pco_gfx_release_workspace()
    print(f"workspace: 2048 reads from a cursor {ws_read} B, 2048 equal ranges {ws_range} B")
    assert ms_read <= ms_range / 4, (ms_read, ms_range)
    assert ms_sixteen <= ms_page / 4, (ms_sixteen, ms_page)
    assert 0 < ws_read < ws_range, (ws_read, ws_range)
