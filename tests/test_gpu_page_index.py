"""-m gpu: pco_gfx_index_pages (include/pco_gfx.h section 4g) -- the cursors in front of rows every_rows, 2 every_rows, ... of a wrapped page from
one walk of it.  The truth is the unchanged pco_gfx_decompress_page_reads: the cursor a chain of reads leaves in front of a row is a function of
the page and the row only, so an index has exactly one right answer, byte for byte.  Streams, chains and guards are test_gpu_page_reads.py's;
every cursor array sits between canary bytes that are checked after every call, and a slot nobody wrote is canary bytes itself."""
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
import test_gpu_page_ranges as R  # noqa: E402  (Stream, write_pages, Pool, run_ranges, profiled_ms)
import test_gpu_page_reads as PR  # noqa: E402  (the streams, the Cursors guards, walk_chains)
import test_page_reads_abi as A  # noqa: E402  (the cursor's layout restated)
from test_gpu_page_reads import L, route1, route2, walked  # noqa: E402,F401  (module-scoped fixtures: the chained cursors are computed once here)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec, PagingSpec  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY, GUARD = PR.CANARY, PR.GUARD
EVERY = [256, 512, 1024, 2816, 3072]
INDEX_WALKERS = ("dec_walk_index_kernel", "dec_walk4_index_kernel", "dec_expand_index_kernel")


def index_len(n, every):
    return (n - 1) // every


class IndexCall:
    """One pco_gfx_index_pages call over jobs [(Stream, page bytes or None for the stream's own, every_rows)].  Each task's k cursors are one
    array between guard bytes; a task with k == 0 passes NULL."""

    def __init__(self, L, jobs, form="sync", stream=None):
        import torch
        self.L, self.jobs, self.form = L, jobs, form
        blobs = []; index = {}
        for s, page, _ in jobs:
            for key, b in ((("m", id(s)), s.meta), (("p", id(s), id(page)), s.page if page is None else page)):
                if key not in index:
                    index[key] = len(blobs); blobs.append(b)
        self.pool = R.Pool(blobs)
        self.ks = [index_len(s.n, every) for s, _, every in jobs]
        self.spans = []; at = 0
        for k in self.ks:
            at += GUARD; self.spans.append(at); at += 256 * k
        self.total = at + GUARD
        self.dev = torch.full((self.total,), CANARY, dtype=torch.uint8, device="cuda")
        self.tasks = (G.PageIndexTask * len(jobs))()
        for j, (s, page, every) in enumerate(jobs):
            pg = s.page if page is None else page
            self.tasks[j] = G.PageIndexTask(self.pool.ptr(index[("m", id(s))]), len(s.meta), self.pool.ptr(index[("p", id(s), id(page))]), len(pg),
                                            (self.dev.data_ptr() + self.spans[j]) if self.ks[j] else None, s.n, every, G.DTYPE_BYTE[s.nums.dtype.name], 4)
        if form == "sync":
            self.res = (G.TaskResult * len(jobs))()
            self.code = L.pco_gfx_index_pages(len(jobs), self.tasks, self.res, None, None if stream is None else C.c_void_p(stream.cuda_stream))
        else:   # d_results on a non-blocking stream of the call's own (or the caller's), behind everything set up so far
            self.d_res = torch.zeros(len(jobs) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
            if stream is None:
                torch.cuda.synchronize()
            else:
                stream.wait_stream(torch.cuda.current_stream())
            self.stream = stream or torch.cuda.Stream()
            self.code = L.pco_gfx_index_pages(len(jobs), self.tasks, None, self.d_res.data_ptr(), C.c_void_p(self.stream.cuda_stream))

    def ptr(self, j, i):
        """cursor i of job j, as a `from` pointer"""
        return self.dev.data_ptr() + self.spans[j] + 256 * i

    def finish(self):
        """(code, results as a numpy record array, [[the 256 bytes of cursor i] per job]) after checking every guard"""
        import torch
        torch.cuda.synchronize()
        rec = np.frombuffer(bytes(self.res), U.RES_DT).copy() if self.form == "sync" else self.d_res.cpu().numpy().view(U.RES_DT).copy()
        host = self.dev.cpu().numpy()
        mask = np.ones(self.total, bool); got = []
        for j, k in enumerate(self.ks):
            mask[self.spans[j]: self.spans[j] + 256 * k] = False
            got.append([host[self.spans[j] + 256 * i: self.spans[j] + 256 * (i + 1)].tobytes() for i in range(k)])
        assert (host[mask] == CANARY).all(), "bytes outside cursors[0 .. k) were written"
        return self.code, rec, got


def run_index(L, jobs, form="sync"):
    return IndexCall(L, jobs, form).finish()


def check_index(jobs, rec, got, truth, aux=0, what=""):
    """truth(job index, row) -> the chained cursor's 256 bytes"""
    for j, (s, _, every) in enumerate(jobs):
        k = index_len(s.n, every); tag = (what, s.label, every)
        assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j], rec["aux"][j]) == (G.ST_OK, k, 0, aux if k else 0), (tag, rec[j])
        assert len(got[j]) == k
        for i in range(k):
            assert got[j][i] == truth(j, (i + 1) * every), (tag, "cursor", i, A.unpack_cursor(PR.words_of(got[j][i])), A.unpack_cursor(PR.words_of(truth(j, (i + 1) * every))))


def read_segments(L, call, jobs_at, form="sync"):
    """Every segment of every job of `call` listed in jobs_at, as tasks of ONE pco_gfx_decompress_page_reads call that start from the index's own
    cursors: [(job index, the page's numbers)]"""
    import torch
    tasks = []; outs = []
    for j in jobs_at:
        s, page, every = call.jobs[j]
        pg = s.page if page is None else page
        w = s.nums.dtype.itemsize
        out = torch.zeros(s.n * w + 64, dtype=torch.uint8, device="cuda"); outs.append(out)
        m, p = call.tasks[j].meta, call.tasks[j].page
        for i, row in enumerate(range(0, s.n, every) if call.ks[j] else [0]):
            count = min(every, s.n - row) if call.ks[j] else s.n
            tasks.append(G.PageReadTask(m, len(s.meta), p, len(pg), out.data_ptr() + row * w, s.n, row, count, G.DTYPE_BYTE[s.nums.dtype.name], 4,
                                        call.ptr(j, i - 1) if i else None, None))
    arr = (G.PageReadTask * len(tasks))(*tasks)
    res = (G.TaskResult * len(tasks))()
    G.check(L.pco_gfx_decompress_page_reads(len(tasks), arr, res, None, None))
    assert all(r.status == 0 for r in res)
    return [(j, o[: call.jobs[j][0].n * call.jobs[j][0].nums.dtype.itemsize].cpu().numpy().view(call.jobs[j][0].nums.dtype)) for j, o in zip(jobs_at, outs)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# index = chain
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_the_index_is_the_chain_of_reads(L, route1, walked, form):
    """Every stream of the two-kernel route at every every_rows, one call: cursor i is the cursor the chained reads left in front of row
    (i + 1) * every_rows, byte for byte; the tasks with k == 0 (2816 numbers at 2816, anything at 3072) pass a NULL cursor array."""
    jobs = [(s, None, every) for s in route1 for every in EVERY]
    owner = [si for si in range(len(route1)) for _ in EVERY]
    assert any(index_len(s.n, e) == 0 and s.n == PR.N_EVEN and e == 2816 for s, _, e in jobs) and any(index_len(s.n, e) == 1 and e == 2816 for s, _, e in jobs)
    # a call of as many order-7 tasks first: every task's plan in the workspace then holds seven moments, and what lies beyond a later page's
    # order is not zero by luck
    si7, s7 = PR.pick(route1, "consecutive7")
    code, rec, got = run_index(L, [(s7, None, 256)] * len(jobs), form)
    assert code == G.PcoSuccess and all(g == [walked[(si7, (i + 1) * 256)] for i in range(11)] for g in got)
    assert all(x != 0 for x in A.unpack_cursor(PR.words_of(got[0][5]))["moments"][0][:7])
    code, rec, got = run_index(L, jobs, form)
    assert code == G.PcoSuccess, L.pco_gfx_last_error()
    check_index(jobs, rec, got, lambda j, row: walked[(owner[j], row)], 0, form)
    assert sum(len(g) for g in got) > 300


def test_segments_from_the_index_in_one_reads_call_equal_the_input(L, route1):
    jobs = [(s, None, every) for s in route1 for every in (256, 1024, 2816)]
    call = IndexCall(L, jobs, "async")   # (the reads below are ordered behind it by finish()'s synchronisation)
    code, rec, got = call.finish()
    assert code == G.PcoSuccess and (rec["status"] == 0).all()
    for j, nums in read_segments(L, call, range(len(jobs))):
        assert U.bits_equal(nums, jobs[j][0].nums), (jobs[j][0].label, jobs[j][2])
    call.finish()   # (the reads left the cursors and their guards alone)


# ---------------------------------------------------------------------------------------------------------------------------------------
# edges of the boundary rule
# ---------------------------------------------------------------------------------------------------------------------------------------
def chain_to(L, s, stops):
    """The cursors chained reads of s leave at `stops` (ascending rows): reads [0, stops[0]), [stops[0], stops[1]), ...; {row: 256 bytes}"""
    cur = PR.Cursors(len(stops)); out = {}; at = 0
    for i, row in enumerate(stops):
        code, rec, got = PR.run_reads(L, [(s, None, at, row - at, i - 1 if i else None, i)], cur)
        assert code == G.PcoSuccess and rec["status"][0] == 0 and U.bits_equal(got[0], s.nums[at: row])
        at = row
    slots = cur.snapshot()
    return {row: slots[i] for i, row in enumerate(stops)}


def test_edges_the_last_cursor_in_front_of_a_batch_of_one_number_and_of_one_shorter_than_the_order(L):
    per = PR.per
    a = R.write_pages(L, [("consecutive1 uint32 n=2817", R.numbers(np.uint32, 2817, 31))], per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))[0]
    b = R.write_pages(L, [("consecutive7 uint64 n=2819", R.numbers(np.uint64, 2819, 32))], per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7))[0]
    assert R.meta_info(L, a).delta_order == 1 and R.meta_info(L, b).delta_order == 7
    truth = [chain_to(L, s, list(range(256, s.n, 256))) for s in (a, b)]
    jobs = [(a, None, 256), (b, None, 256), (a, None, 2816), (b, None, 1280)]
    for form in ("sync", "async"):
        call = IndexCall(L, jobs, form)
        code, rec, got = call.finish()
        assert code == G.PcoSuccess and [len(g) for g in got] == [11, 11, 1, 2]
        check_index(jobs, rec, got, lambda j, row: truth[j % 2][row], 0, form)
        for j, nums in read_segments(L, call, range(len(jobs))):
            assert U.bits_equal(nums, jobs[j][0].nums), (form, j)


def test_edges_an_index_of_257_cursors(L):
    """65 793 numbers at every_rows 256: more cursors than a block has threads.  Chained truth for cursors 0, 1, 255 and 256; all 258 segments
    decoded from the index in one reads call."""
    n = 65793
    s = R.write_pages(L, [("consecutive1 uint32 n=65793", R.numbers(np.uint32, n, 33))], PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))[0]
    c = R.write_pages(L, [("classic uint16 n=65793", R.numbers(np.uint16, n, 34))], PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP))[0]
    truth = [chain_to(L, x, [256, 512, 65536, 65792]) for x in (s, c)]
    jobs = [(s, None, 256), (c, None, 256)]
    for form in ("sync", "async"):
        call = IndexCall(L, jobs, form)
        code, rec, got = call.finish()
        assert code == G.PcoSuccess and list(rec["n_out"]) == [257, 257] and (rec["status"] == 0).all() and (rec["aux"] == 0).all() and (rec["consumed"] == 0).all()
        for j in range(2):
            for i in (0, 1, 255, 256):
                assert got[j][i] == truth[j][(i + 1) * 256], (form, j, i)
            for i in range(257):
                cw = A.unpack_cursor(PR.words_of(got[j][i]))
                assert (cw["version"], cw["kind"], cw["row"], cw["page_n"], cw["tail"]) == (A.VERSION, A.FULL, (i + 1) * 256, n, [0] * 6), (form, j, i)
        for j, nums in read_segments(L, call, [0, 1]):
            assert U.bits_equal(nums, jobs[j][0].nums), (form, j)


# ---------------------------------------------------------------------------------------------------------------------------------------
# route 2: position-only cursors
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_route_2_pages_get_position_only_cursors_without_a_walk(L, route2, form):
    assert len(route2) == 9
    chained = PR.walk_chains(L, route2, "sync", want_kind=A.POSITION)
    jobs = [(s, None, every) for s in route2 for every in (256, 1024, 8192)]
    owner = [si for si in range(len(route2)) for _ in range(3)]
    L.pco_gfx_profile_begin()
    call = IndexCall(L, jobs, form)
    kernels = U.profile_names(L)
    code, rec, got = call.finish()
    assert code == G.PcoSuccess, L.pco_gfx_last_error()
    check_index(jobs, rec, got, lambda j, row: chained[(owner[j], row)], 1, form)
    for g in got:
        for raw in g:
            assert sum(1 for w in PR.words_of(raw) if w) == 3   # version | kind, row, page_n | dtype: nothing else
    # the walkers ran once per number width to hand the pages back, the scratch route decoded first batches and copied nothing
    widths = {"u" + str(8 * s.nums.dtype.itemsize) for s in route2}
    assert [k for k in kernels if k.startswith(INDEX_WALKERS)] == sorted(f"{w}<{t}>" for w in INDEX_WALKERS for t in widths), kernels
    assert "index_finish_kernel" in kernels and not any(k.startswith("range_copy_kernel") for k in kernels), kernels
    assert {k for k in kernels if k.startswith("pco_decode_prefix_kernel")} == {f"pco_decode_prefix_kernel<{t}>" for t in widths}, kernels
    for j, nums in read_segments(L, call, range(len(jobs))):
        assert U.bits_equal(nums, jobs[j][0].nums), (jobs[j][0].label, jobs[j][2])


# ---------------------------------------------------------------------------------------------------------------------------------------
# one mixed call
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_mixed_call_reports_each_bad_task_alone(L, route1, route2, walked):
    """About 40 tasks over all four widths in shuffled order.  The yardstick for every status is pco_gfx_decompress_page_ranges on the same bytes
    in the same form: {0, k * every_rows} for a page of the two-kernel route, {0, 1} for one the walkers hand back."""
    rng = np.random.default_rng(9)
    chained2 = PR.walk_chains(L, route2, "sync", want_kind=A.POSITION)
    jobs = []; truth = []; yard = []
    for si, s in enumerate(route1):
        every = int(rng.choice([256, 512, 768, 1024]))
        jobs.append((s, None, every)); truth.append(("r1", si)); yard.append((s, None, 0, index_len(s.n, every) * every))
    for si, s in enumerate(route2):
        every = int(rng.choice([256, 1024]))
        jobs.append((s, None, every)); truth.append(("r2", si)); yard.append((s, None, 0, 1))
    for s in (route1[0], route1[8], route2[0]):   # k == 0
        jobs.append((s, None, 3072 if s.n <= 3072 else 1 << 20)); truth.append(None); yard.append((s, None, 0, 0))
    vi, victim = PR.pick(route1, "consecutive2")
    cut_inside = victim.page[: len(victim.page) // 3]
    jobs.append((victim, cut_inside, 256)); truth.append("bad"); yard.append((victim, cut_inside, 0, 11 * 256))
    ci, cs = PR.pick(route1, "float_mult")
    cut_behind = cs.page[: len(cs.page) - 3]
    jobs.append((cs, cut_behind, 1024)); truth.append(("r1", ci)); yard.append((cs, cut_behind, 0, 2048))
    di, ds = PR.pick(route1, "consecutive1")
    damaged = R.Stream("damaged ChunkMeta", ds.nums, ds.meta[: len(ds.meta) // 2], ds.page)
    jobs.append((damaged, None, 512)); truth.append("bad"); yard.append((damaged, None, 0, 2560))
    # lookback with a delta'd secondary variable (test_gpu_page_reads.py's stream): OK from a second history buffer in the synchronous form, UNSUPPORTED in the other
    x = (np.cumsum(np.random.default_rng(3).integers(-5, 7, 3000)) / 4.0).astype(np.float32)
    meta, pages = O.test_encode(x, pages=[x.size], mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1,
                                secondary_uses_delta=True, lookback_seed=5)
    lb2 = R.Stream("lookback+secondary float32", x, meta, pages[0])
    jobs.append((lb2, None, 1024)); truth.append("lb2"); yard.append((lb2, None, 0, 1))
    assert {s.nums.dtype.itemsize for s, _, _ in jobs} == {1, 2, 4, 8} and 35 <= len(jobs) <= 45
    order = rng.permutation(len(jobs))
    jobs = [jobs[i] for i in order]; truth = [truth[i] for i in order]; yard = [yard[i] for i in order]

    def want(j, row):
        kind, si = truth[j]
        return walked[(si, row)] if kind == "r1" else chained2[(si, row)]

    for form in ("sync", "async"):
        rcode, rrec, _ = R.run_ranges(L, yard, form)
        code, rec, got = run_index(L, jobs, form)   # (checks the guards around every cursor array, the failing tasks' included)
        assert code == rcode and (rec["status"] == rrec["status"]).all(), (form, rec["status"], rrec["status"])
        bad = [j for j, t in enumerate(truth) if t == "bad"]
        assert len(bad) == 2 and all(rec["status"][j] != 0 and rec["n_out"][j] == 0 and rec["consumed"][j] == 0 for j in bad), (form, rec[bad])
        assert rec["status"][[j for j in bad if jobs[j][1] is not None][0]] == G.ST_INSUFFICIENT_DATA
        if form == "sync":
            assert code == G.PcoDecompressionError and "page index task" in (L.pco_gfx_last_error() or b"").decode()
        keep = [j for j in range(len(jobs)) if truth[j] != "bad"]
        for j in keep:
            if truth[j] == "lb2":
                want_lb2 = (G.ST_OK, 2, 0, 1) if form == "sync" else (G.ST_UNSUPPORTED, 0, 0, 0)
                assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j], rec["aux"][j]) == want_lb2, (form, rec[j])
                if form == "sync":
                    assert [PR.words_of(c) for c in got[j]] == [A.pack_cursor(A.POSITION, row, 0, 3000, G.DTYPE_BYTE["float32"]) for row in (1024, 2048)]
            elif truth[j] is None:
                assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j], rec["aux"][j]) == (0, 0, 0, 0) and got[j] == []
            else:
                check_index([jobs[j]], rec[[j]], [got[j]], lambda _, row: want(j, row), 1 if truth[j][0] == "r2" else 0, form)


# ---------------------------------------------------------------------------------------------------------------------------------------
# two streams on one workspace
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_streams_on_one_workspace(L, route1, walked):
    import torch
    half = len(route1) // 2
    jobs = [(s, None, 256) for s in route1]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    U.device_delay(sa)   # stream A is still busy when stream B's call arrives
    a = IndexCall(L, jobs[:half], "async", sa)
    b = IndexCall(L, jobs[half:], "async", sb)
    for call, part, base in ((a, jobs[:half], 0), (b, jobs[half:], half)):
        code, rec, got = call.finish()
        assert code == G.PcoSuccess
        check_index(part, rec, got, lambda j, row: walked[(base + j, row)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# Python
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_index_pages_is_save_cursors_in_one_call(L):
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
        for every in (256, 1024):
            saved = paged.save_cursors(cc.blob, d, [names[k]], every)
            index = paged.index_pages(cc.blob, d, [names[k]], every)
            torch.cuda.synchronize()
            res = index.results.cpu().numpy().view(paged.RESULT_DT)
            assert [(pc.chunk, pc.piece, pc.every_rows, tuple(pc.cursors.shape)) for pc in index] == [(pc.chunk, pc.piece, pc.every_rows, tuple(pc.cursors.shape)) for pc in saved]
            assert (res["status"] == 0).all() and list(res["n_out"]) == [(p.n - 1) // every for p in d if p.piece]
            for pi, ps in zip(index, saved):
                assert pi.cursors.cpu().numpy().tobytes() == ps.cursors.cpu().numpy().tobytes(), (names[k], every, pi.piece)
            got = paged.decompress_chunks_from(cc.blob, d, [names[k]], index)
            assert len(got) == 1 and U.bits_equal(got[0].cpu().numpy(), x), (names[k], every)
            # windows that start on, just behind and just in front of a cursor, and that cross a page boundary
            first_page = next(p.n for p in d if p.piece == 1)
            for start, stop in ((every, every + 300), (every + 1, every + 2), (every - 1, every + 1), (first_page - 100, first_page + every + 100), (0, x.size),
                                (x.size - 1, x.size), (5, 5)):
                want = paged.decompress_rows(cc.blob, d, [names[k]], [(start, stop)])[0].cpu().numpy()
                have = paged.decompress_rows_from(cc.blob, d, [names[k]], index, [(start, stop)])[0].cpu().numpy()
                assert U.bits_equal(have, want) and U.bits_equal(have, x[start: stop]), (names[k], every, start, stop)
    with pytest.raises(ValueError):
        paged.index_pages(blobs[0].blob, blobs[0].directory, ["float32"], 100)
    with pytest.raises(ValueError):
        paged.index_pages(blobs[0].blob, blobs[0].directory, ["float32"], 0)
    # one call's kernels, whatever the number of cursors
    L.pco_gfx_profile_begin()
    paged.index_pages(blobs[2].blob, blobs[2].directory, ["int64"], 256)
    kernels = U.profile_names(L)
    assert kernels == ["dec_expand_index_kernel<u64>", "dec_walk4_index_kernel<u64>", "dec_walk_index_kernel<u64>", "index_finish_kernel", "pco_decode_prefix_kernel<u64>"], kernels


# ---------------------------------------------------------------------------------------------------------------------------------------
# work: one walk
# ---------------------------------------------------------------------------------------------------------------------------------------
def profiled(L, fn):
    """(summed milliseconds, every name in launch order with repeats, the milliseconds of each) of fn's second run"""
    import torch
    fn()   # untimed
    torch.cuda.synchronize()
    L.pco_gfx_profile_begin()
    fn()
    torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 16); ms = (C.c_float * 4096)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 4096)
    raw = names.raw; out = []; pos = 0
    for _ in range(nk):
        e = raw.index(b"\0", pos); out.append(raw[pos:e].decode()); pos = e + 1
    return float(sum(ms[:nk])), out, [float(x) for x in ms[:nk]]


def test_the_work_of_an_index_is_one_walk(L):
    """The 2^20-number u64 delta-1 page of test_the_work_of_a_read_follows_its_slice at a cursor every 2^16 rows: the one index call against the
    fifteen chained reads that build the same cursors (the unchanged entry point).  Both walk batches [0, 3840) once; the index stores no rows
    and builds its tables once, which is a few per cent of a walk.  An index that walked twice, or decoded prefixes, would take 2x and more;
    the walker's chain varies by 10 to 25 % from run to run: 1.5 separates the two.
    Measured on the MI355X: 24.1 / 19.4 / 23.8 / 20.1 ms for the index against 21.8 / 21.1 / 21.9 / 22.1 ms for the chain."""
    import torch
    n = 1 << 20; seg = 1 << 16
    s = R.write_pages(L, [("c2 2^20", U.synth("c2", n))], G.make_config(mode=1, delta=2, delta_order=1, max_page_n=n))[0]
    pool = R.Pool([s.meta, s.page])
    part = torch.zeros(seg * 8 + 64, dtype=torch.uint8, device="cuda")
    chained = torch.zeros((15, 256), dtype=torch.uint8, device="cuda")
    index = torch.zeros((15, 256), dtype=torch.uint8, device="cuda")

    def one_read(k):
        t = (G.PageReadTask * 1)(G.PageReadTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), part.data_ptr(), n, k * seg, seg, 2, 4,
                                                chained.data_ptr() + 256 * (k - 1) if k else None, chained.data_ptr() + 256 * k))
        res = (G.TaskResult * 1)()
        G.check(L.pco_gfx_decompress_page_reads(1, t, res, None, None))

    def one_index():
        t = (G.PageIndexTask * 1)(G.PageIndexTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), index.data_ptr(), n, seg, 2, 4))
        res = (G.TaskResult * 1)()
        G.check(L.pco_gfx_index_pages(1, t, res, None, None))
        assert (res[0].n_out, res[0].consumed, res[0].status, res[0].aux) == (15, 0, 0, 0)

    ms_chain = sum(R.profiled_ms(L, lambda k=k: one_read(k)) for k in range(15))   # (read k's first, untimed run leaves the cursor its second run and read k + 1 start from)
    ms_index, names, each = profiled(L, one_index)
    print(f"fifteen cursors of a 2^20-number page: one index call {ms_index:.3f} ms, fifteen chained reads {ms_chain:.3f} ms")
    print("  the index call's kernels: " + ", ".join(f"{k} {x:.3f} ms" for k, x in zip(names, each)))
    print("  the last chained read's: " + ", ".join(f"{k} {x:.3f} ms" for k, x in zip(*profiled(L, lambda: one_read(14))[1:])))
    assert index.cpu().numpy().tobytes() == chained.cpu().numpy().tobytes()
    # each index walker once, whatever k; beside them only the scratch route every index call takes up front (nothing for it to do here) and the finish
    assert sorted(k for k in names if k.startswith(INDEX_WALKERS)) == ["dec_expand_index_kernel<u64>", "dec_walk4_index_kernel<u64>", "dec_walk_index_kernel<u64>"], names
    assert sorted(k for k in names if not k.startswith(INDEX_WALKERS)) == ["index_finish_kernel", "pco_decode_prefix_kernel<u64>"], names
    assert ms_index <= 1.5 * ms_chain, (ms_index, ms_chain)
