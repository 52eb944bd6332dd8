"""-m gpu: pco_gfx_take_rows (include/pco_gfx.h section 4n) -- rows of indexed pages by row ids that live on the device.

Every page kind and number width of the section on the shapes and id lists of tests/take_model.py: the bytes against the SOURCE numbers and against
pco_gfx_decompress_pages, the work (n_out, aux, consumed) against the model's plan, canaries around dst and in the entries of ids no page owns;
pages damaged behind and inside the wanted batches; two pages sharing one id list; the cursor refusals the device makes; the asynchronous
filter -> take pipeline on a stream of its own.  A test is one call (or a few) of many tasks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
import take_model as M  # noqa: E402
import test_gpu_page_ranges as R  # noqa: E402  (Stream, write_pages, Pool, numbers, meta_info)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY, GUARD = R.CANARY, R.GUARD
OK, INSUFFICIENT, INVALID = G.ST_OK, G.ST_INSUFFICIENT_DATA, G.ST_INVALID_ARGUMENT
STRIDES = tuple(e for e in M.EVERY_ROWS if e)


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------------
# pages, indexes and the one way to the entry point
# ---------------------------------------------------------------------------------------------------------------------------------------
per = lambda **kw: G.make_config(enable_8_bit=True, max_page_n=1 << 24, **kw)   # noqa: E731
WIDE = (np.uint8, np.uint16, np.int32, np.float32, np.uint64, np.float64)
LONG_NS = tuple(n for n in M.PAGE_NS if n > 256)   # (the kinds whose encoders want a page of some length)


def dict_numbers(dt, n, seed):
    return np.random.default_rng(1).integers(0, 1 << 15, 50).astype(dt)[np.random.default_rng(seed).integers(0, 50, n)]


def float_mult_numbers(dt, n):
    """multiples of 0.01, every seventh one ULP off: the secondary variable has more than one value"""
    x = (np.cumsum(np.random.default_rng(n).integers(-5, 7, n)) / 100.0).astype(dt)
    x[::7] = np.nextafter(x[::7], np.dtype(dt).type(np.inf))
    return x


# kind -> (config, number types, page sizes, numbers, the call's flags, whether the page has cursors to resume from)
KINDS = {
    "classic": (per(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), WIDE, M.PAGE_NS, lambda dt, n: R.numbers(dt, n, n + 1), 0, True),
    "consecutive2": (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=2), WIDE, M.PAGE_NS, lambda dt, n: R.numbers(dt, n, n + 2), 0, True),
    "float_mult": (per(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), (np.float32, np.float64), LONG_NS,
                   lambda dt, n: float_mult_numbers(dt, n), 0, True),
    "conv1": (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=8, conv1=True), (np.uint8, np.uint16, np.int32, np.float32), LONG_NS,
              lambda dt, n: R.numbers(dt, n, 3), G.CURSOR_GENERAL, True),
    "dict": (per(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True), (np.uint16, np.int32, np.float32, np.uint64, np.float64), LONG_NS,
             lambda dt, n: dict_numbers(dt, n, n), G.CURSOR_GENERAL, True),
    "lookback": (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK), WIDE, M.PAGE_NS, lambda dt, n: R.numbers(dt, n, n + 7, period=365 if n >= 1000 else 100), 0, False),
}
EXPECT = {"classic": (0, 0), "consecutive2": (0, 1), "float_mult": (2, 1), "conv1": (0, 3), "dict": (4, 0), "lookback": (0, 2)}   # (mode_kind, delta_kind) of the ChunkMeta


class Pages:
    """The pages of one kind on the device: streams, their bytes in a Pool (meta 2 i, page 2 i + 1), and an index per (stream, stride) made by
    pco_gfx_index_pages_ex under the kind's flags."""

    def __init__(self, L, kind):
        import torch
        cfg, types, ns, make, self.flags, self.indexed = KINDS[kind]
        self.kind = kind
        self.streams = R.write_pages(L, [(f"{kind} {np.dtype(dt).name} n={n}", make(dt, n)) for dt in types for n in ns], cfg)
        self.pool = R.Pool([b for s in self.streams for b in (s.meta, s.page)])
        self.cursors = {}
        if not self.indexed:
            return
        want = [(i, e) for i, s in enumerate(self.streams) for e in STRIDES if (s.n - 1) // e > 0]
        tasks = (G.PageIndexTask * len(want))()
        for j, (i, e) in enumerate(want):
            s = self.streams[i]
            self.cursors[(i, e)] = torch.zeros(((s.n - 1) // e, G.CURSOR_BYTES), dtype=torch.uint8, device="cuda")
            tasks[j] = G.PageIndexTask(self.pool.ptr(2 * i), len(s.meta), self.pool.ptr(2 * i + 1), len(s.page), self.cursors[(i, e)].data_ptr(), s.n, e,
                                       G.DTYPE_BYTE[s.nums.dtype.name], 4)
        res = (G.TaskResult * len(want))()
        G.check(L.pco_gfx_index_pages_ex(len(want), tasks, self.flags, res, None, None))
        assert all(r.status == OK and r.n_out == (self.streams[i].n - 1) // e for r, (i, e) in zip(res, want))

    def job(self, i, every_rows, row_base, ids, page=None, cursors="own"):
        """One take task: stream i under stride every_rows (0, or a stride the page is too short for: no index)."""
        cur = self.cursors.get((i, every_rows)) if cursors == "own" else cursors
        return dict(s=self.streams[i], meta=self.pool.ptr(2 * i), page=self.pool.ptr(2 * i + 1) if page is None else page[0],
                    page_len=len(self.streams[i].page) if page is None else page[1], cursors=cur, every_rows=every_rows if cur is not None else 0,
                    row_base=row_base, ids=np.asarray(ids, dtype=np.uint64))


@pytest.fixture(scope="module")
def pages(L):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Pages(L, kind)
        return cache[kind]
    return get


def run_take(L, jobs, flags=0, form="sync"):
    """One pco_gfx_take_rows call over `jobs` (Pages.job).  Every job has an id list and a canary-filled dst of its own between guards; the id lists lie at
    8-byte addresses that alternate between 16-byte aligned and not.  Returns (code, results, [dst per job as the stream's numbers]) after checking
    that no byte outside the dsts was written."""
    import torch
    id_at = []; at = 0
    for j, job in enumerate(jobs):
        at += 16 + 8 * (j & 1); id_at.append(at); at += 8 * len(job["ids"])
    ids_host = np.zeros(at // 8 + 2, np.uint64)
    for a, job in zip(id_at, jobs):
        ids_host[a // 8: a // 8 + len(job["ids"])] = job["ids"]
    d_ids = torch.from_numpy(ids_host.view(np.int64)).cuda()
    spans = []; at = 0
    for job in jobs:
        at += GUARD; spans.append(at); at += (len(job["ids"]) * job["s"].nums.dtype.itemsize + 15) // 16 * 16
    total = at + GUARD
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    tasks = (G.TakeTask * max(len(jobs), 1))()
    for j, job in enumerate(jobs):
        s, n = job["s"], len(job["ids"])
        tasks[j] = G.TakeTask(job["meta"], len(s.meta), job["page"], job["page_len"], s.n, job["row_base"], None if job["cursors"] is None else job["cursors"].data_ptr(),
                              job["every_rows"], d_ids.data_ptr() + id_at[j] if n else None, n, out.data_ptr() + spans[j] if n else None, G.DTYPE_BYTE[s.nums.dtype.name], 4)
    if form == "sync":
        res = (G.TaskResult * max(len(jobs), 1))()
        code = L.pco_gfx_take_rows(len(jobs), tasks, flags, res, None, None)
        rec = np.frombuffer(bytes(res), U.RES_DT).copy()[: len(jobs)]
    else:   # d_results on a stream of its own
        st = torch.cuda.Stream()
        d_res = torch.zeros(max(len(jobs), 1) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        code = L.pco_gfx_take_rows(len(jobs), tasks, flags, None, d_res.data_ptr(), C.c_void_p(st.cuda_stream))
        st.synchronize()
        rec = d_res.cpu().numpy().view(U.RES_DT).copy()[: len(jobs)]
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    mask = np.ones(total, bool); got = []
    for j, job in enumerate(jobs):
        nbytes = len(job["ids"]) * job["s"].nums.dtype.itemsize
        mask[spans[j]: spans[j] + nbytes] = False
        got.append(host[spans[j]: spans[j] + nbytes].view(job["s"].nums.dtype))
    assert (host[mask] == CANARY).all(), "bytes outside dst[0 .. n_rows * width) were written"
    return code, rec, got


def expected(job, reference=None):
    """(the dst the call must leave, the model's plan): the source's numbers at the ids the page owns, the canary everywhere else."""
    s = job["s"]
    plan = M.plan(s.n, job["every_rows"], job["row_base"], [int(i) for i in job["ids"]])
    want = np.frombuffer(bytes([CANARY]) * (len(job["ids"]) * s.nums.dtype.itemsize), s.nums.dtype).copy()
    src = s.nums if reference is None else reference
    mine = np.array([r is not None for r in plan.local], bool)
    want[mine] = src[np.array([r for r in plan.local if r is not None], np.int64)]
    return want, plan


def check_exact(jobs, rec, got, what=""):
    for j, job in enumerate(jobs):
        want, plan = expected(job)
        tag = (what, job["s"].label, job["every_rows"], job["row_base"], job.get("name"))
        assert rec["status"][j] == OK, (tag, int(rec["status"][j]))
        assert (int(rec["n_out"][j]), int(rec["aux"][j]), int(rec["consumed"][j])) == (plan.n_out, plan.aux, plan.consumed), tag
        assert U.bits_equal(got[j], want), tag


def lists_of(s, every_rows, row_base, big):
    """The model's id lists for a page; with `big`, a seeded random 5 % and a full permutation as well."""
    out = dict(M.id_lists(s.n, every_rows, row_base))
    if big:
        rng = np.random.default_rng(s.n + every_rows)
        out["random 5 %"] = row_base + rng.integers(0, s.n, max(s.n // 20, 1))
        out["permutation"] = row_base + rng.permutation(s.n)
    return out


def jobs_of(pg, strides=M.EVERY_ROWS):
    jobs = []
    for i, s in enumerate(pg.streams):
        for e in (strides if pg.indexed else (0,)):
            if e and (i, e) not in pg.cursors:
                continue   # (the page is shorter than the stride: the same task as stride 0)
            for b, row_base in enumerate(M.ROW_BASES):
                for name, ids in lists_of(s, e, row_base, big=b == (i + e // 256) % 2).items():
                    jobs.append(dict(pg.job(i, e, row_base, ids), name=name))
    return jobs


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the bytes and the work
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decoded(L, pages):
    """kind -> every stream of it through pco_gfx_decompress_pages, once: the second reference, which must be the source bit for bit."""
    import torch
    cache = {}

    def get(kind):
        if kind in cache:
            return cache[kind]
        pg = pages(kind)
        outs = [torch.zeros(s.n * s.nums.dtype.itemsize + 64, dtype=torch.uint8, device="cuda") for s in pg.streams]
        tasks = (G.PageTask * len(outs))(*[G.PageTask(pg.pool.ptr(2 * i), len(s.meta), pg.pool.ptr(2 * i + 1), len(s.page), o.data_ptr(), s.n, G.DTYPE_BYTE[s.nums.dtype.name], 4)
                                           for i, (s, o) in enumerate(zip(pg.streams, outs))])
        res = (G.TaskResult * len(outs))()
        G.check(L.pco_gfx_decompress_pages(len(outs), tasks, res, None, None))
        cache[kind] = [o.cpu().numpy()[: s.n * s.nums.dtype.itemsize].view(s.nums.dtype) for s, o in zip(pg.streams, outs)]
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_pages_are_what_they_are_called_and_decode_to_their_source(L, pages, decoded, kind):
    """(a Try spec may fall back on a short or an unsuitable page: every number type of the kind has pages that kept it, the longest among them)"""
    kept = set()
    for s, d in zip(pages(kind).streams, decoded(kind)):
        info = R.meta_info(L, s)
        assert U.bits_equal(d, s.nums), s.label
        if (info.mode_kind, info.delta_kind) == EXPECT[kind] and (kind != "float_mult" or (info.present[2] == 1 and info.n_bins[2] > 1)):   # (FloatMult: a real secondary variable)
            kept.add((s.nums.dtype.name, s.n))
    narrow = ("uint8",) if kind == "lookback" else ()   # (the encoder finds no gain in a lookback over these 8-bit numbers and writes no delta)
    assert {(np.dtype(dt).name, 70000) for dt in KINDS[kind][1] if np.dtype(dt).name not in narrow} <= kept, sorted(kept)


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_id_list_of_the_model_takes_the_source_s_rows_and_walks_what_the_model_plans(L, pages, decoded, kind):
    """Each page under every stride and without an index, each with every id list of the model (and a random 5 % and a full permutation), as the tasks of
    one call per stride (symbol scratch is per segment and sized by the call's longest): dst against numpy indexing of the source (test above: the whole decode equals it), out-of-page entries and guards untouched, and
    (n_out, aux, consumed) the model's -- so indexed and un-indexed calls give the same bytes and differ in their work alone."""
    pg = pages(kind)
    by_page = {}
    for e in (M.EVERY_ROWS if pg.indexed else (0,)):
        jobs = jobs_of(pg, (e,))
        assert len(jobs) >= 40 and all(j["every_rows"] == e for j in jobs)
        code, rec, got = run_take(L, jobs, pg.flags)
        assert code == G.PcoSuccess, (L.pco_gfx_last_error() or b"").decode()
        check_exact(jobs, rec, got, kind)
        for job, g in zip(jobs, got):   # the same (page, list) under every stride: the same bytes
            by_page.setdefault((job["s"].label, job["ids"].tobytes()), []).append(g)
    assert all(U.bits_equal(g, gs[0]) for gs in by_page.values() for g in gs)
    assert not pg.indexed or max(len(gs) for gs in by_page.values()) >= len(M.EVERY_ROWS)   # (some list was taken under every stride and without an index)


def test_one_segment_of_137_is_one_walk(L, pages):
    pg = pages("classic")
    i = next(i for i, s in enumerate(pg.streams) if s.n == 70000 and s.nums.dtype == np.uint64)
    jobs = [pg.job(i, 512, 0, [77 * 512 + 5, 77 * 512 + 300, 77 * 512 + 5]), pg.job(i, 512, 9, [9 + 136 * 512 + 367]), pg.job(i, 512, 0, [70000, 1 << 40])]
    code, rec, got = run_take(L, jobs)
    assert code == G.PcoSuccess and M.n_segments(70000, 512) == 137
    check_exact(jobs, rec, got)
    assert [(int(r["n_out"]), int(r["aux"]), int(r["consumed"])) for r in rec] == [(3, 1, 2), (1, 1, 2), (0, 0, 0)]


def cursor_bit(cur, k):
    return int(cur.cpu().numpy().view(np.uint64).reshape(-1, 32)[k, 2])


@pytest.mark.parametrize("kind", ["classic", "consecutive2"])
def test_damage_behind_the_last_wanted_batch_is_ok_and_damage_inside_is_the_read_task_s_status(L, pages, kind):
    import torch
    pg = pages(kind)
    i = next(i for i, s in enumerate(pg.streams) if s.n == 70000 and s.nums.dtype == np.int32)
    s = pg.streams[i]; cur = pg.cursors[(i, 512)]
    ids = [40 * 512 + 3, 40 * 512 + 200, 3 * 512 + 1]   # segments 3 and 40, the latter to its batch 0 only
    # zeros from the first bit of segment 41 on: behind every wanted batch
    cut = (cursor_bit(cur, 40) + 7) // 8
    behind = np.frombuffer(s.page, np.uint8).copy(); behind[cut:] = 0
    # the page ends inside segment 40's first batch
    short_len = cursor_bit(cur, 39) // 8 + 2
    pool = R.Pool([behind.tobytes(), s.page[:short_len]])
    jobs = [pg.job(i, 512, 0, ids, page=(pool.ptr(0), len(s.page))), pg.job(i, 512, 0, ids, page=(pool.ptr(1), short_len)), pg.job(i, 512, 0, ids),
            pg.job(i, 512, 0, [3 * 512 + 1, 7], page=(pool.ptr(1), short_len))]   # (the short page again, its damage behind what is wanted)
    code, rec, got = run_take(L, jobs)
    assert code == G.PcoDecompressionError and b"take rows task 1 failed" in L.pco_gfx_last_error()
    check_exact([jobs[0], jobs[2], jobs[3]], rec[[0, 2, 3]], [got[0], got[2], got[3]], kind)
    # the read task of the failing segment, on the same bytes
    dst = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    read = (G.PageReadTask * 1)(G.PageReadTask(pg.pool.ptr(2 * i), len(s.meta), pool.ptr(1), short_len, dst.data_ptr(), s.n, 40 * 512, 201, G.DTYPE_BYTE[s.nums.dtype.name], 4,
                                               cur.data_ptr() + 39 * G.CURSOR_BYTES, None))
    rres = (G.TaskResult * 1)()
    assert L.pco_gfx_decompress_page_reads(1, read, rres, None, None) == G.PcoDecompressionError
    assert rres[0].status == INSUFFICIENT
    assert (int(rec["status"][1]), int(rec["n_out"][1])) == (rres[0].status, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3: the pages of a chunk share one id list
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_pages_of_one_chunk_share_the_ids_and_the_output(L):
    import torch
    x = R.numbers(np.int32, 5049, 5); y = R.numbers(np.float64, 1000, 6)
    cc = paged.compress_chunks([torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()], ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(1)),
                               page_sizes=[[3000, 2049], None])
    dtypes = ["int32", "float64"]
    index = paged.index_pages(cc.blob, cc.directory, dtypes, 512)
    rng = np.random.default_rng(3)
    ids = np.concatenate([rng.permutation(5049)[:700], [2999, 3000, 0, 5048, 3000]]).astype(np.int64)
    rows = [torch.from_numpy(ids).cuda(), None]
    for ix in (index, None):
        out, = paged.take_rows(cc.blob, cc.directory, dtypes, rows, index=ix)
        assert np.array_equal(out.cpu().numpy(), x[ids])
    (out,), res = paged.take_rows_async(cc, rows, index=index)
    torch.cuda.synchronize()
    rec = res.cpu().numpy().view(U.RES_DT)
    assert np.array_equal(out.cpu().numpy(), x[ids]) and len(rec) == 2 and (rec["status"] == OK).all()
    assert [int(n) for n in rec["n_out"]] == [int((ids < 3000).sum()), int((ids >= 3000).sum())] and int(rec["n_out"].sum()) == len(ids)
    # an id beyond the chunk is nobody's: the sum is short, its entry keeps what it held, and take_rows says so
    beyond = np.concatenate([ids, [5049]]).astype(np.int64)
    (out,), res = paged.take_rows_async(cc, [torch.from_numpy(beyond).cuda(), None], index=index)
    torch.cuda.synchronize()
    assert int(res.cpu().numpy().view(U.RES_DT)["n_out"].sum()) == len(beyond) - 1 and np.array_equal(out.cpu().numpy()[:-1], x[ids])
    with pytest.raises(IndexError, match="1 of the 706 row ids of chunk 0"):
        paged.take_rows(cc.blob, cc.directory, dtypes, [torch.from_numpy(beyond).cuda(), None], index=index)
    with pytest.raises(IndexError):
        paged.take_rows(cc.blob, cc.directory, dtypes, [torch.tensor([-1], dtype=torch.int64, device="cuda"), None])
    out0, out1 = paged.take_rows(cc.blob, cc.directory, dtypes, [torch.zeros(0, dtype=torch.int64, device="cuda"), torch.tensor([999, 0], dtype=torch.int64, device="cuda")], index=index)
    assert out0.numel() == 0 and U.bits_equal(out1.cpu().numpy(), y[[999, 0]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4: the refusals the device makes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_cursor_that_is_not_the_segment_s_is_refused_on_the_device(L, pages):
    import torch
    pg = pages("classic")
    i = next(i for i, s in enumerate(pg.streams) if s.n == 70000 and s.nums.dtype == np.uint16)
    twin = next(k for k, s in enumerate(pg.streams) if s.n == 70000 and s.nums.dtype == np.int32)   # (for the good neighbour)
    s = pg.streams[i]
    ids = [600, 5000, 69999]
    roomy = torch.zeros((274, G.CURSOR_BYTES), dtype=torch.uint8, device="cuda"); roomy[:136] = pg.cursors[(i, 512)]   # the stride-512 index, with room for a stride-256 reader
    jobs = [pg.job(i, 256, 0, ids, cursors=roomy),                # read at stride 256: cursor s - 1 stands at row 512 s, beyond the segment's first row
            pg.job(i, 4096, 0, ids, cursors=pg.cursors[(i, 512)]),   # read at stride 4096: the walk from row 512 s is longer than the scratch of a segment
            pg.job(twin, 512, 0, ids), pg.job(i, 512, 0, [5])]    # good neighbours; segment 0 needs no cursor
    code, rec, got = run_take(L, jobs)
    assert code == G.PcoDecompressionError
    assert [int(x) for x in rec["status"]] == [INVALID, INVALID, OK, OK] and int(rec["n_out"][0]) == int(rec["n_out"][1]) == 0
    check_exact(jobs[2:], rec[2:], got[2:])
    # a kind-3 index read without the flag
    cv = pages("conv1")
    c = next(k for k, s in enumerate(cv.streams) if s.n == 2049)
    jobs = [cv.job(c, 512, 0, [1500, 3]), pg.job(twin, 512, 0, ids)]
    code, rec, got = run_take(L, jobs, flags=0)
    assert [int(x) for x in rec["status"]] == [INVALID, OK] and int(rec["n_out"][0]) == 0
    check_exact(jobs[1:], rec[1:], got[1:])
    code, rec, got = run_take(L, jobs, flags=G.CURSOR_GENERAL)   # ... and with it
    assert code == G.PcoSuccess
    check_exact(jobs, rec, got)


def test_the_index_of_another_page_of_the_same_shape_writes_nothing_outside_dst(L, pages):
    """Cursors that pass every check but belong to another page: wrong numbers or a status, and run_take's canaries say that nothing else was written."""
    pg = pages("classic"); other = pages("consecutive2")
    i = next(i for i, s in enumerate(pg.streams) if s.n == 70000 and s.nums.dtype == np.uint64)
    o = next(k for k, s in enumerate(other.streams) if s.n == 70000 and s.nums.dtype == np.uint64)
    c2 = next(k for k, s in enumerate(pg.streams) if s.n == 70000 and s.nums.dtype == np.float64)
    ids = [100, 700, 33000, 69999, 70000]
    jobs = [pg.job(i, 512, 0, ids, cursors=other.cursors[(o, 512)]), pg.job(i, 512, 0, ids, cursors=pg.cursors[(c2, 512)]), pg.job(i, 512, 0, ids)]
    code, rec, got = run_take(L, jobs)
    check_exact(jobs[2:], rec[2:], got[2:])
    for j in (0, 1):
        assert int(rec["status"][j]) in (OK, INSUFFICIENT, INVALID, G.ST_CORRUPTION)
        assert got[j][4:].tobytes() == bytes([CANARY]) * 8   # the id no page owns
        if rec["status"][j] == OK:
            assert got[j][0] == pg.streams[i].nums[100]   # (segment 0 starts at the page's start)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5: the asynchronous pipeline
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_filter_then_take_on_one_stream(L):
    """encode -> compact -> index -> a mask's nonzero -> take, issued on one non-default stream; the take call is the asynchronous form."""
    import torch
    key = R.numbers(np.int32, 70000, 21); val = R.numbers(np.float64, 70000, 22)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_key = torch.from_numpy(key).cuda(); d_val = torch.from_numpy(val).cuda()
        cc = paged.compress_chunks([d_key, d_val], ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(1)), stream=st)
        cc.directory   # (the tasks carry addresses: the one read-back, in front of the pipeline)
        index = paged.index_pages_async(cc, 4096, stream=st)
        ids = torch.nonzero(d_key % 97 == 3).reshape(-1)
        (taken,), res = paged.take_rows_async(cc, [None, ids], index=index, stream=st)
    st.synchronize()
    want = np.flatnonzero(key % 97 == 3)
    assert len(want) > 100 and np.array_equal(ids.cpu().numpy(), want)
    assert U.bits_equal(taken.cpu().numpy(), val[want])
    rec = res.cpu().numpy().view(U.RES_DT)
    plan = M.plan(70000, 4096, 0, [int(i) for i in want])
    assert len(rec) == 1 and (int(rec["status"][0]), int(rec["n_out"][0]), int(rec["aux"][0]), int(rec["consumed"][0])) == (OK, plan.n_out, plan.aux, plan.consumed)


def test_a_mixed_asynchronous_call_of_every_kind_and_width_in_shuffled_order(L, pages):
    jobs = []
    for kind in KINDS:
        pg = pages(kind)
        for i, s in enumerate(pg.streams):
            if s.n not in (257, 2049, 70000):
                continue
            e = 512 if (i, 512) in pg.cursors else 0
            if e == 0 and s.n == 70000:
                continue   # (an un-indexed long page would size every segment's symbol scratch in the call)
            lists = lists_of(s, e, 1000003, big=s.n == 2049)
            for name in ("boundaries", "reversed", "outside_and_inside", "random 5 %", "permutation"):
                if name in lists:
                    jobs.append(dict(pg.job(i, e, 1000003, lists[name]), name=name))
    order = np.random.default_rng(5).permutation(len(jobs))
    jobs = [jobs[k] for k in order]
    assert len({j["s"].nums.dtype.itemsize for j in jobs}) == 4 and len(jobs) > 60
    code, rec, got = run_take(L, jobs, flags=G.CURSOR_GENERAL, form="async")
    assert code == G.PcoSuccess
    check_exact(jobs, rec, got, "mixed")
