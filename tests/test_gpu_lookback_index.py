"""-m gpu: pco_gfx_index_pages_hist (include/pco_gfx.h section 4j) -- a Lookback page indexed in one walk, a history snapshot beside each kind-4
cursor.  The streams and the `walked` pairs are tests/test_gpu_lookback_history.py's: pages of 2816 and 3000 numbers, windows of 2 to 4096 rows,
states of 1 to 256, u8 to u64 and f64, Classic / IntMult / FloatMult, one foreign 2^14 table -- the smallest shapes where the ring wraps, the reach
hits page_n and the window exceeds the page.  Truth is the pair a chain of pco_gfx_decompress_page_reads_hist calls leaves at the same row, byte for
byte.  Every cursor array and every history array sits between canary bytes, the histories start as canary bytes, and so does the tail of each stride."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
import test_gpu_page_ranges as R  # noqa: E402  (Stream, write_pages, Pool, meta_info, numbers, profiled_ms)
import test_page_reads_abi as A  # noqa: E402
import test_gpu_page_reads as PR  # noqa: E402  (the canaries, small_passes)
import test_gpu_page_index as PI  # noqa: E402  (index_len, profiled)
import test_gpu_lookback_history as LH  # noqa: E402  (streams, walked, others, hist_bytes, dtype_of)
from test_gpu_lookback_history import L, streams, walked, others  # noqa: E402,F401  (module fixtures)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY, GUARD = PR.CANARY, PR.GUARD
LOOKBACK, POSITION = LH.LOOKBACK, A.POSITION
EVERY = [256, 512, 768, 2816]
TAIL = 24   # bytes of stride behind a history's own: never written


class IndexHistCall:
    """One pco_gfx_index_pages_hist call over jobs [(Stream, page bytes or None, every_rows, stride or None for no histories)].  A task's k cursors
    are one array between guard bytes, and so are its k histories, history i at i * stride; everything starts as canary bytes.  entry: "hist", or
    "ex" -- the same jobs through pco_gfx_index_pages_ex, the yardstick."""

    def __init__(self, L, jobs, form="sync", flags=0, entry="hist"):
        import torch
        self.L, self.jobs, self.form = L, jobs, form
        blobs = []; index = {}
        for s, page, *_ in jobs:
            for key, b in ((("m", id(s)), s.meta), (("p", id(s), id(page)), s.page if page is None else page)):
                if key not in index:
                    index[key] = len(blobs); blobs.append(b)
        self.pool = R.Pool(blobs)
        self.ks = [PI.index_len(s.n, every) for s, _, every, _ in jobs]
        self.spans = []; self.hspans = []; at = 0; hat = 0
        for k, (_, _, _, stride) in zip(self.ks, jobs):
            at += GUARD; self.spans.append(at); at += 256 * k
            hat += GUARD; self.hspans.append(hat); hat += (stride or 0) * k
        self.total, self.htotal = at + GUARD, hat + GUARD
        self.dev = torch.full((self.total,), CANARY, dtype=torch.uint8, device="cuda")
        self.hdev = torch.full((self.htotal,), CANARY, dtype=torch.uint8, device="cuda")
        kind = G.PageIndexHistTask if entry == "hist" else G.PageIndexTask
        self.tasks = (kind * len(jobs))()
        for j, (s, page, every, stride) in enumerate(jobs):
            pg = s.page if page is None else page
            head = (self.pool.ptr(index[("m", id(s))]), len(s.meta), self.pool.ptr(index[("p", id(s), id(page))]), len(pg),
                    (self.dev.data_ptr() + self.spans[j]) if self.ks[j] else None, s.n, every, LH.dtype_of(s), 4)
            self.tasks[j] = kind(*head, *(((self.hdev.data_ptr() + self.hspans[j]) if stride else None, stride or 0) if entry == "hist" else ()))
        fn = (lambda *a: L.pco_gfx_index_pages_hist(a[0], a[1], flags, *a[2:])) if entry == "hist" else (lambda *a: L.pco_gfx_index_pages_ex(a[0], a[1], flags, *a[2:]))
        if form == "sync":
            self.res = (G.TaskResult * len(jobs))()
            self.code = fn(len(jobs), self.tasks, self.res, None, None)
        else:
            self.d_res = torch.zeros(len(jobs) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            self.stream = torch.cuda.Stream()
            self.code = fn(len(jobs), self.tasks, None, self.d_res.data_ptr(), C.c_void_p(self.stream.cuda_stream))

    def ptr(self, j, i):
        return self.dev.data_ptr() + self.spans[j] + 256 * i

    def hptr(self, j, i):
        return self.hdev.data_ptr() + self.hspans[j] + i * self.jobs[j][3]

    def finish(self):
        """(code, results, [[cursor i's 256 bytes] per job], [[history i's stride bytes] per job]) after checking every guard"""
        import torch
        torch.cuda.synchronize()
        rec = np.frombuffer(bytes(self.res), U.RES_DT).copy() if self.form == "sync" else self.d_res.cpu().numpy().view(U.RES_DT).copy()
        host, hhost = self.dev.cpu().numpy(), self.hdev.cpu().numpy()
        mask = np.ones(self.total, bool); hmask = np.ones(self.htotal, bool); got = []; hgot = []
        for j, k in enumerate(self.ks):
            stride = self.jobs[j][3] or 0
            mask[self.spans[j]: self.spans[j] + 256 * k] = False
            hmask[self.hspans[j]: self.hspans[j] + stride * k] = False
            got.append([host[self.spans[j] + 256 * i: self.spans[j] + 256 * (i + 1)].tobytes() for i in range(k)])
            hgot.append([hhost[self.hspans[j] + stride * i: self.hspans[j] + stride * (i + 1)].tobytes() for i in range(k)] if stride else [])
        assert (host[mask] == CANARY).all(), "bytes outside cursors[0 .. k) were written"
        assert (hhost[hmask] == CANARY).all(), "bytes outside the k history extents were written"
        return self.code, rec, got, hgot


def stride_of(L, s, tail=TAIL):
    return (LH.hist_bytes(L, s) + 7) // 8 * 8 + tail


def check_pairs(L, jobs, sis, rec, got, hgot, walked, what=""):
    """every task of `jobs` (stream sis[j] of the streams) ended OK with the chain's pairs, the stride's tail on canaries"""
    for j, (s, _, every, stride) in enumerate(jobs):
        k = PI.index_len(s.n, every); hb = LH.hist_bytes(L, s); tag = (what, s.label, every)
        assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j], rec["aux"][j]) == (G.ST_OK, k, 0, 0), (tag, rec[j])
        assert len(got[j]) == k and len(hgot[j]) == k
        for i in range(k):
            cur, ring = walked[(sis[j], (i + 1) * every)]
            assert got[j][i] == cur, (tag, "cursor", i, A.unpack_cursor(PR.words_of(got[j][i])), A.unpack_cursor(PR.words_of(cur)))
            assert len(ring) == hb and hgot[j][i][:hb] == ring, (tag, "history", i)
            assert hgot[j][i][hb:] == bytes([CANARY]) * (stride - hb), (tag, "the stride's tail", i)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. pairs
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async", "sync in passes"])
@pytest.mark.parametrize("every", EVERY)
def test_the_index_leaves_the_pairs_of_the_chain(L, streams, walked, every, form):
    jobs = [(s, None, every, stride_of(L, s)) for s in streams]
    if form == "sync in passes":
        with PR.small_passes():
            code, rec, got, hgot = IndexHistCall(L, jobs, "sync").finish()
    else:
        code, rec, got, hgot = IndexHistCall(L, jobs, form).finish()
    assert code == G.PcoSuccess, L.pco_gfx_last_error()
    check_pairs(L, jobs, list(range(len(streams))), rec, got, hgot, walked, form)
    assert sum(len(g) for g in got) >= (1 if every == 2816 else len(streams))   # (2816 indexes the pages of 3000 numbers only: k == 0 for the others)


def test_the_flag_changes_nothing_on_a_lookback_page(L, streams, walked):
    jobs = [(s, None, 512, stride_of(L, s)) for s in streams[:4]]
    code, rec, got, hgot = IndexHistCall(L, jobs, "sync", G.CURSOR_GENERAL).finish()
    check_pairs(L, jobs, [0, 1, 2, 3], rec, got, hgot, walked)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2., 3. without histories, and beside pages that take none
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, G.CURSOR_GENERAL])
def test_without_histories_every_task_is_the_ex_task(L, streams, others, flags):
    jobs = [(s, None, 512 if k % 2 else 256, None) for k, s in enumerate(streams[:6] + others)]
    jobs.append((streams[0], streams[0].page[:40], 512, None))   # ... and a task that fails
    jobs.append((streams[1], None, 4096, None))                  # ... and one with k == 0
    for form in ("sync", "async"):
        a = IndexHistCall(L, jobs, form, flags, entry="ex").finish(); b = IndexHistCall(L, jobs, form, flags).finish()
        assert a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2], (form, a[1], b[1])
        lb = [A.unpack_cursor(PR.words_of(c))["kind"] for g in b[2][:6] for c in g]
        assert lb and set(lb) == {POSITION} and all(b[1]["aux"][:6] == 1)   # Lookback pages keep kind 2 and aux bit 0


@pytest.mark.parametrize("form", ["sync", "async"])
def test_one_mixed_call_leaves_the_histories_of_the_other_pages_alone(L, streams, others, walked, form):
    """a resumable Lookback page, Dict under Lookback, a Conv1 page, a two-kernel page and a page with k == 0, all with histories: only the first
    writes its histories, the others are the _ex tasks"""
    pages = [streams[10], others[2], others[1], others[0], streams[0]]
    every = [512, 512, 512, 512, 4096]
    jobs = [(s, None, e, 64 + (s.nums.dtype.itemsize << s.wl) + TAIL) for s, e in zip(pages, every)]
    code, rec, got, hgot = IndexHistCall(L, jobs, form, G.CURSOR_GENERAL).finish()
    ex = IndexHistCall(L, [j[:3] + (None,) for j in jobs], form, G.CURSOR_GENERAL, entry="ex").finish()
    assert code == G.PcoSuccess and [int(x) for x in rec["status"]] == [0] * 5 and int(rec["n_out"][4]) == 0
    check_pairs(L, jobs[:1], [10], rec[:1], got[:1], hgot[:1], walked, form)
    assert (rec[1:] == ex[1][1:]).all() and got[1:] == ex[2][1:], (rec, ex[1])
    kinds = [A.unpack_cursor(PR.words_of(g[0]))["kind"] for g in got[:4]]
    assert kinds == [LOOKBACK, POSITION, 3, A.FULL]
    for j in (1, 2, 3):
        assert all(h == bytes([CANARY]) * len(h) for h in hgot[j]) and len(hgot[j]) == len(got[j]) > 0, pages[j].label


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_a_short_stride_refuses_its_task_alone(L, streams, walked, form):
    picks = [0, 3, 10]   # the writer's page, a ring of 8 bytes, int-mult's three variables
    jobs = []
    for si in picks:
        s = streams[si]; hb = LH.hist_bytes(L, s)
        assert hb % 8 == 0
        jobs += [(s, None, 512, hb - 8), (s, None, 512, hb)]   # one 8-byte step short; exactly history_bytes
    code, rec, got, hgot = IndexHistCall(L, jobs, form).finish()
    if form == "sync":
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT
    for t, si in enumerate(picks):
        bad, good = 2 * t, 2 * t + 1
        assert (rec["status"][bad], rec["n_out"][bad], rec["consumed"][bad], rec["aux"][bad]) == (G.ST_INVALID_ARGUMENT, 0, 0, 0), rec[bad]
        assert all(c == PR.UNWRITTEN for c in got[bad]) and all(h == bytes([CANARY]) * len(h) for h in hgot[bad]) and len(got[bad]) == 5
        check_pairs(L, [jobs[good]], [si], rec[good: good + 1], [got[good]], [hgot[good]], walked, form)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. damage
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_a_page_damaged_inside_the_walked_prefix_and_behind_the_last_cursor(L, streams, walked, form):
    for si in (0, 5, 10):   # the writer's page, a window beyond the page, int-mult
        s = streams[si]
        bit = lambda row: A.unpack_cursor(PR.words_of(walked[(si, row)][0]))["bit"]   # noqa: E731
        k = PI.index_len(s.n, 512); last = k * 512
        behind = s.page[: bit(last) // 8 + 1]    # every batch in front of the last cursor is whole; what follows is gone
        inside = s.page[: bit(last - 256) // 8 + 1]     # the last walked batch is gone
        jobs = [(s, inside, 512, stride_of(L, s)), (s, behind, 512, stride_of(L, s)), (s, None, 512, stride_of(L, s))]
        code, rec, got, hgot = IndexHistCall(L, jobs, form).finish()   # (finish: nothing outside the tasks' extents is written)
        assert list(rec["status"]) == [G.ST_INSUFFICIENT_DATA, G.ST_OK, G.ST_OK] and int(rec["n_out"][0]) == 0, (s.label, form, rec)
        check_pairs(L, jobs[1:], [si, si], rec[1:], got[1:], hgot[1:], walked, form)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the point: segments side by side from the index's pairs
# ---------------------------------------------------------------------------------------------------------------------------------------
def segments(L, call, js):
    """every segment of jobs `js` of `call` as tasks of ONE pco_gfx_decompress_page_reads_hist call with to == NULL: [the page's numbers per job]"""
    import torch
    tasks = []; outs = []
    for j in js:
        s, page, every, stride = call.jobs[j]
        w = s.nums.dtype.itemsize; t = call.tasks[j]
        out = torch.zeros(s.n * w + 64, dtype=torch.uint8, device="cuda"); outs.append(out)
        for i, row in enumerate(range(0, s.n, every) if call.ks[j] else [0]):
            count = min(every, s.n - row) if call.ks[j] else s.n
            tasks.append(G.PageReadHistTask(t.meta, t.meta_len, t.page, t.page_len, out.data_ptr() + row * w, s.n, row, count, LH.dtype_of(s), 4,
                                            call.ptr(j, i - 1) if i else None, None, call.hptr(j, i - 1) if i else None, stride if i else 0))
    arr = (G.PageReadHistTask * len(tasks))(*tasks); res = (G.TaskResult * len(tasks))()
    G.check(L.pco_gfx_decompress_page_reads_hist(len(tasks), arr, 0, res, None, None))
    assert all(r.status == 0 for r in res)
    return [o[: call.jobs[j][0].n * call.jobs[j][0].nums.dtype.itemsize].cpu().numpy().view(call.jobs[j][0].nums.dtype) for j, o in zip(js, outs)]


@pytest.mark.parametrize("every", [256, 768])
def test_every_page_decodes_as_segments_in_one_call_from_the_index_s_pairs(L, streams, every):
    jobs = [(s, None, every, stride_of(L, s)) for s in streams]
    call = IndexHistCall(L, jobs, "async")
    code, rec, got, hgot = call.finish()
    assert (rec["status"] == 0).all()
    js = list(range(len(streams)))
    for _ in range(2):   # the pairs are left as they are: a second call gives the same rows
        for s, x in zip(streams, segments(L, call, js)):
            assert U.bits_equal(x, s.nums), (s.label, every)
        again = call.finish()
        assert again[2] == got and again[3] == hgot


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. paged
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_paged_index_with_histories_returns_the_rows_of_the_plain_functions(L):
    import torch
    lb = R.numbers(np.int64, 9000, 8, period=365)
    cd = R.numbers(np.int64, 5000, 9)
    a = paged.compress_chunks([torch.from_numpy(lb).cuda()], ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_lookback()), page_sizes=[[5000, 4000]])
    b = paged.compress_chunks([torch.from_numpy(cd).cuda()], ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(1)), page_sizes=[[3000, 2000]])
    # one blob of two chunks: chunk 0 under Lookback, chunk 1 under Consecutive
    da, db = a.directory, b.directory
    ta, tb = (a.total + 63) // 64 * 64, b.total
    blob = torch.cat([a.blob[:ta], b.blob[:tb], torch.zeros(64, dtype=torch.uint8, device="cuda")])
    directory = list(da) + [paged.Piece(1, p.piece, p.n, p.offset + ta, p.length) for p in db]
    dtypes = ["int64", "int64"]
    idx = paged.index_pages(blob, directory, dtypes, 1024, history=True)
    torch.cuda.synchronize()
    res = idx.results.cpu().numpy().view(paged.RESULT_DT)
    assert (res["status"] == 0).all() and list(res["n_out"]) == [4, 3, 2, 1]
    assert [h is not None for h in idx.histories] == [True, True, False, False] and [tuple(h.shape)[0] for h in idx.histories[:2]] == [4, 3]
    kinds = [int(pc.cursors[0].cpu().numpy().view(np.uint64)[0]) >> 32 for pc in idx]
    assert kinds == [LOOKBACK, LOOKBACK, A.FULL, A.FULL]
    before = [h.clone() for h in idx.histories[:2]]
    L.pco_gfx_profile_begin()
    got = paged.decompress_chunks_from(blob, directory, dtypes, idx, histories=idx.histories)
    names = U.profile_names(L)
    assert any(n.startswith("pco_decode_general_resume_kernel") for n in names) and not any(n.startswith("pco_decode_prefix_kernel") for n in names), names
    want = paged.decompress_chunks(blob, directory, dtypes)
    assert all(U.bits_equal(g.cpu().numpy(), w.cpu().numpy()) for g, w in zip(got, want)) and U.bits_equal(got[0].cpu().numpy(), lb) and U.bits_equal(got[1].cpu().numpy(), cd)
    rows = [(1500, 8200), (100, 4900)]
    got = paged.decompress_rows_from(blob, directory, dtypes, idx, rows, histories=idx.histories)
    want = paged.decompress_rows(blob, directory, dtypes, rows)
    assert all(U.bits_equal(g.cpu().numpy(), w.cpu().numpy()) for g, w in zip(got, want)) and U.bits_equal(got[0].cpu().numpy(), lb[1500:8200])
    assert all(torch.equal(x, y) for x, y in zip(before, idx.histories[:2]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8. the work
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_work_of_a_lookback_index_is_one_walk_and_its_segments_run_side_by_side(L):
    """The one i64 periodic Lookback page of 2^18 numbers of test_the_work_of_a_lookback_read_follows_its_slice, a pair every n / 16 rows.  Kernel time
    from pco_gfx_profile_*: (a) the sixteen segments from the index's pairs in ONE pco_gfx_decompress_page_reads_hist call against the whole page
    through pco_gfx_decompress_pages: 1/16 of the chain's length by construction, at most 1/4 (one-wave chains move 25 % between runs: the margin
    the 4h and 4i tests give the same construction); (b) the index call against the range task {0, 15 n / 16} through
    pco_gfx_decompress_page_ranges: the same walk, minus join and store, plus fifteen ring copies -- at most 1.5 x, as 4g and 4h assert.
    Measured on the MI355X: segments 1.87 ms against 11.85 ms for the page (0.158); the index 25.30 ms against 25.77 ms for the range
    (0.98), its snapshot kernel 0.008 ms."""
    import torch
    n = 1 << 18; seg = n // 16; w = 8; dt = G.DTYPE_BYTE["int64"]
    s = R.write_pages(L, [("lookback int64 2^18", R.numbers(np.int64, n, 8, period=365))], G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK, max_page_n=n))[0]
    info = R.meta_info(L, s)
    assert info.delta_kind == 2
    hb = L.pco_gfx_lookback_history_bytes(int(info.window_n_log), dt)
    pool = R.Pool([s.meta, s.page])
    whole = torch.zeros(n * w + 64, dtype=torch.uint8, device="cuda")
    curs = torch.zeros((15, 256), dtype=torch.uint8, device="cuda")
    rings = torch.zeros((15, (hb + 7) // 8 * 8), dtype=torch.uint8, device="cuda")
    head = (pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page))

    def index():
        t = (G.PageIndexHistTask * 1)(G.PageIndexHistTask(*head, curs.data_ptr(), n, seg, dt, 4, rings.data_ptr(), rings.shape[1])); res = (G.TaskResult * 1)()
        G.check(L.pco_gfx_index_pages_hist(1, t, 0, res, None, None))
        assert (res[0].n_out, res[0].consumed, res[0].status, res[0].aux) == (15, 0, 0, 0)

    def sixteen():
        t = (G.PageReadHistTask * 16)(*[G.PageReadHistTask(*head, whole.data_ptr() + w * k * seg, n, k * seg, seg, dt, 4, curs.data_ptr() + 256 * (k - 1) if k else None, None,
                                                          rings.data_ptr() + (k - 1) * rings.shape[1] if k else None, rings.shape[1] if k else 0) for k in range(16)])
        res = (G.TaskResult * 16)()
        G.check(L.pco_gfx_decompress_page_reads_hist(16, t, 0, res, None, None))

    def one_page():
        t = (G.PageTask * 1)(G.PageTask(*head, whole.data_ptr(), n, dt, 4)); res = (G.TaskResult * 1)()
        G.check(L.pco_gfx_decompress_pages(1, t, res, None, None))

    def prefix_as_range():
        t = (G.PageRangeTask * 1)(G.PageRangeTask(*head, whole.data_ptr(), n, 0, 15 * seg, dt, 4)); res = (G.TaskResult * 1)()
        G.check(L.pco_gfx_decompress_page_ranges(1, t, res, None, None))

    ms_index, names, each = PI.profiled(L, index)
    ms_range = R.profiled_ms(L, prefix_as_range)
    ms_page = R.profiled_ms(L, one_page)
    assert U.bits_equal(whole[: n * w].cpu().numpy().view(np.int64), s.nums)
    whole.zero_()
    ms_segments = R.profiled_ms(L, sixteen)
    assert U.bits_equal(whole[: n * w].cpu().numpy().view(np.int64), s.nums)
    snap = sum(x for k, x in zip(names, each) if k.startswith("index_history_snapshot_kernel"))
    print(f"{s.label}: sixteen segments in one call {ms_segments:.3f} ms, the whole page {ms_page:.3f} ms; the index call {ms_index:.3f} ms "
          f"(its snapshot kernel {snap:.3f} ms), the range {{0, 15 n / 16}} {ms_range:.3f} ms")
    print("  the index call's kernels: " + ", ".join(f"{k} {x:.3f} ms" for k, x in zip(names, each)))
    assert [k for k in names if k.startswith(("pco_decode_general_index_hist_kernel", "index_history_snapshot_kernel"))] == \
        ["pco_decode_general_index_hist_kernel<u64>", "index_history_snapshot_kernel<u64>"] * 2, names   # (two batches up front, then the pass with the prefix)
    assert ms_segments <= ms_page / 4, (ms_segments, ms_page)
    assert ms_index <= 1.5 * ms_range, (ms_index, ms_range)
