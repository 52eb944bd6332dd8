"""-m gpu: the ORDERED list of launches, repeats kept, of the entry points that decode PART of a page, against
tests/golden/partial_launch_sequences.json.

test_gpu_launch_sequences.py records launch_decode and the encoder; this module is the same guard for the partial-decode driver of
pco_gfx_ranges.hip: pco_gfx_decompress_page_ranges[_dir], pco_gfx_decompress_page_reads[_ex, _hist, _dir], pco_gfx_index_pages[_ex, _hist, _dir]
and the two standalone-chunk forms.  That driver decides from the form, the flags, the histories, the directory and the synchronous / asynchronous
form which kernels a call launches, in which order and how often.  Each case of the matrix below takes one of its branches; every case runs in its
synchronous and its asynchronous form (results null, d_results given) where it has both, and the names pco_gfx_profile_end reports must be the
recorded list, entry for entry.  A refactor of the driver must leave the file as it is.

Every call's rows are also compared with the input, and every cursor (and history) with the chain of reads that reaches its row, by the helpers of
the modules the streams come from: a recording of wrong output pins nothing.  The calls run in ONE child process whose environment holds no
PCO_GFX_* variable (the budget case narrows PCO_GFX_WORKSPACE_GB inside its call and drops it again).

The golden file is a recording: `python tests/test_gpu_partial_launch_sequences.py` runs the same child and rewrites it (do that only with a library
whose launch sequences are known to be the intended ones, and say in the commit why they changed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "partial_launch_sequences.json")
pytestmark = pytest.mark.gpu

BOTH = ("sync", "async")
# case -> the forms it runs in
CASES = {
    "ranges_u64": BOTH, "ranges_all_widths": BOTH, "ranges_k4": BOTH,
    "reads_u64": BOTH, "reads_all_widths": BOTH, "reads_k4": BOTH,
    "index_u64": BOTH, "index_all_widths": BOTH, "index_k4": BOTH,
    "reads_handed_back_flags0": BOTH, "reads_handed_back_general": BOTH, "index_handed_back_flags0": BOTH, "index_handed_back_general": BOTH,
    "reads_hist_some": BOTH, "reads_hist_none": BOTH, "reads_ex_of_hist_none": BOTH,
    "index_hist_some": BOTH, "index_hist_none": BOTH, "index_ex_of_hist_none": BOTH,
    "second_round_reads": BOTH, "second_round_index": BOTH,
    "reads_in_budget_passes": ("sync",),
    "ranges_dir": BOTH, "ranges_dir_one_refused": BOTH, "reads_dir": BOTH, "reads_dir_one_refused": BOTH, "index_dir": BOTH,
    "chunk_reads_dir": BOTH, "chunk_index_dir": BOTH,
}
EVERY = 256


class Matrix:
    """The streams, the chains that are the truth of every cursor, and one method per case: method(form) -> {call name: [launches]}."""

    def __init__(self, L):
        import oracle_lib as O
        import test_gpu_general_cursors as GC
        import test_gpu_lookback_history as LH
        import test_gpu_page_ranges as R
        import test_gpu_page_reads as PR
        import test_page_reads_abi as A
        from pcodec_amd import _lib as G
        self.L = L
        c1 = PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1)
        # the two-kernel route: Classic + Consecutive(1) at every width, pages of 1024 to 4096 rows; then the page only the 4-chunk walker takes
        self.fast = R.write_pages(L, [("c1 uint64 3000", R.numbers(np.uint64, 3000, 1)), ("c1 uint64 2048", R.numbers(np.uint64, 2048, 2)), ("c1 uint64 4096", R.numbers(np.uint64, 4096, 3)),
                                      ("c1 uint32 3000", R.numbers(np.uint32, 3000, 4)), ("c1 uint16 2816", R.numbers(np.uint16, 2816, 5)), ("c1 uint8 3000", R.numbers(np.uint8, 3000, 6))], c1)
        self.fast.append(PR.from_generator("k4 table uint32", np.random.default_rng(6).integers(0, 5000, 3000).astype(np.uint32), mode=O.MODE_CLASSIC, tbl_vars=O.TBL_PRIMARY,
                                           tbl_ans_size_log=PR.k4_table_log(), tbl_n_bins=65, tbl_seed=10))
        self.u64, self.widths, self.k4 = [0, 1, 2], [0, 3, 4, 5], [6, 3]
        # pages the walkers hand back to the scratch route: Lookback, Conv1, Dict
        self.back = R.write_pages(L, [("lookback uint32", R.numbers(np.uint32, 3000, 7, period=365))], PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK))
        self.back.append(PR.from_generator("conv1 uint16", R.numbers(np.uint16, 2816, 2), mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=4, bias=5, weights=[-16, 32]))
        rng = np.random.default_rng(7)
        self.back.append(PR.from_generator("dict uint32", rng.integers(0, 1 << 30, 50).astype(np.uint32)[rng.integers(0, 50, 3000)], mode=O.MODE_TRY_DICT))
        for s, kind in zip(self.back, ("lookback", "conv1", "dict")):
            s.kind, s.order = kind, 0
        infos = [R.meta_info(L, s) for s in self.back]
        assert infos[0].delta_kind == 2 and infos[1].delta_kind == 3 and infos[2].mode_kind == 4
        # resumable Lookback pages for the histories: the writer's, and a generated one with a ring of 16 rows
        self.hist = R.write_pages(L, [("writer int64 periodic", R.numbers(np.int64, 3000, 8, period=365))], PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK))
        self.hist.append(PR.from_generator("lookback uint32 window 2^4", LH.seasonal(np.uint32, 2816, 47), delta=O.TE_DELTA_LOOKBACK, window_n_log=4, state_n_log=4, lookback_seed=7,
                                           mode=O.MODE_CLASSIC))
        for s in self.hist:
            i = R.meta_info(L, s)
            assert i.delta_kind == 2 and i.secondary_uses_delta == 0
            s.wl, s.sl = int(i.window_n_log), int(i.state_n_log)
        # the one stream that takes the second round: Lookback with a delta'd secondary variable
        x = (np.cumsum(np.random.default_rng(3).integers(-5, 7, 3000)) / 4.0).astype(np.float32)
        meta, pages = O.test_encode(x, pages=[x.size], mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1, secondary_uses_delta=True,
                                    lookback_seed=5)
        self.second = R.Stream("lookback+secondary float32", x, meta, pages[0])
        i = R.meta_info(L, self.second)
        assert i.delta_kind == 2 and i.secondary_uses_delta == 1 and i.present[2] == 1
        # the truth of every cursor: chains of synchronous reads (each checks its rows against the input)
        self.chain_fast = PR.walk_chains(L, self.fast, "sync")
        self.chain_back0 = PR.walk_chains(L, self.back, "sync", want_kind=A.POSITION)
        self.chain_backg = GC.walk_all(GC.Flagged(L), self.back, "sync")
        self.chain_hist = LH.walk_chains(L, self.hist, "sync")

    def profiled(self, fn):
        import gpu_util as U
        self.L.pco_gfx_profile_begin()
        out = fn()
        return out, U.profile_launches(self.L)

    # ---- pointer tasks on the two-kernel route ----
    def ranges(self, form, picks):
        import test_gpu_page_ranges as R
        from pcodec_amd import _lib as G
        jobs = [(self.fast[i], None, f, c) for i in picks for f, c in ((0, self.fast[i].n), (300, 500), (self.fast[i].n - 1, 1), (7, 0))]
        (code, rec, got), names = self.profiled(lambda: R.run_ranges(self.L, jobs, form))
        assert code == G.PcoSuccess
        R.check_ok(jobs, rec, got, form)
        return {"ranges": names}

    def reads(self, form, streams, chain, lib=None, kinds=None):
        """two calls: rows [0, 1024) without a `from` (no row read-back), then the rest of the page from the cursors the first left"""
        import test_gpu_page_reads as PR
        import test_page_reads_abi as A
        from pcodec_amd import _lib as G
        lib = lib or self.L
        cur = PR.Cursors(2 * len(streams))
        out = {}
        for name, jobs in (("first", [(s, None, 0, 1024, None, 2 * k) for k, s in enumerate(streams)]),
                           ("second", [(s, None, 1024, s.n - 1024, 2 * k, 2 * k + 1) for k, s in enumerate(streams) if s.n > 1024] + [(streams[0], None, 5, 0, None, None)])):
            (code, rec, got), out[name] = self.profiled(lambda: PR.run_reads(lib, jobs, cur, form))
            assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
            PR.check_ok(jobs, rec, got, (form, name))
            slots = cur.snapshot()
            for s, _, first, count, _, to in jobs:
                if to is not None:
                    row = min((first + count + 255) // 256 * 256, s.n)
                    assert slots[to] == chain[(streams.index(s), row)], (s.label, row, A.unpack_cursor(PR.words_of(slots[to])))
        return out

    def index(self, form, streams, chain, lib=None, every=EVERY):
        import test_gpu_page_index as PI
        from pcodec_amd import _lib as G
        jobs = [(s, None, every) for s in streams] + [(streams[0], None, 8192)]   # (the last: k == 0)
        (code, rec, got), names = self.profiled(lambda: PI.run_index(lib or self.L, jobs, form))
        assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
        for j, (s, _, e) in enumerate(jobs):
            k = PI.index_len(s.n, e)
            assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j]) == (G.ST_OK, k, 0) and len(got[j]) == k, (s.label, rec[j])
            for i in range(k):
                assert got[j][i] == chain[(streams.index(s), (i + 1) * e)], (s.label, "cursor", i)
        return {"index": names}

    def ranges_u64(self, form): return self.ranges(form, self.u64)
    def ranges_all_widths(self, form): return self.ranges(form, self.widths)
    def ranges_k4(self, form): return self.ranges(form, self.k4)

    def pick(self, picks):
        return [self.fast[i] for i in picks], {(k, row): raw for k, i in enumerate(picks) for (si, row), raw in self.chain_fast.items() if si == i}

    def reads_u64(self, form): return self.reads(form, *self.pick(self.u64))
    def reads_all_widths(self, form): return self.reads(form, *self.pick(self.widths))
    def reads_k4(self, form): return self.reads(form, *self.pick(self.k4))
    def index_u64(self, form): return self.index(form, *self.pick(self.u64))
    def index_all_widths(self, form): return self.index(form, *self.pick(self.widths))
    def index_k4(self, form): return self.index(form, *self.pick(self.k4))

    # ---- pages the walkers hand back ----
    def reads_handed_back_flags0(self, form): return self.reads(form, self.back, self.chain_back0)

    def reads_handed_back_general(self, form):
        """(the second call's `from` cursors are kind 3 on the Conv1 and the Dict page)"""
        import test_gpu_general_cursors as GC
        return self.reads(form, self.back, self.chain_backg, GC.Flagged(self.L))

    def index_handed_back_flags0(self, form): return self.index(form, self.back, self.chain_back0)

    def index_handed_back_general(self, form):
        import test_gpu_general_cursors as GC
        return self.index(form, self.back, self.chain_backg, GC.Flagged(self.L))

    # ---- histories ----
    def reads_hist(self, form, with_hist, entry="hist"):
        """tasks 0 and 1 with a history (where the call has any), task 2 -- the same page as task 0 -- without, a two-kernel page, and one without rows"""
        import test_gpu_general_cursors as GC
        import test_gpu_lookback_history as LH
        import test_gpu_page_reads as PR
        import test_page_reads_abi as A
        from pcodec_amd import _lib as G
        pages = [self.hist[0], self.hist[1], self.hist[0], self.fast[3]]
        hists = LH.Histories([LH.hist_bytes(self.L, s) for s in self.hist])
        cur = PR.Cursors(2 * len(pages))
        slot = [0, 1, None, None] if with_hist else [None] * 4
        out = {}
        for name, jobs in (("first", [(s, None, 0, 1024, None, 2 * k, slot[k]) for k, s in enumerate(pages)]),
                           ("second", [(s, None, 1024, s.n - 1024, 2 * k, 2 * k + 1, slot[k]) for k, s in enumerate(pages)] + [(pages[0], None, 9, 0, None, None, None)])):
            if entry == "hist":
                (code, rec, got), out[name] = self.profiled(lambda: LH.run_hist(self.L, jobs, cur, hists, form))
            else:
                (code, rec, got), out[name] = self.profiled(lambda: PR.run_reads(GC.Flagged(self.L, 0), [j[:6] for j in jobs], cur, form))
            assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
            PR.check_ok([j[:6] for j in jobs], rec, got, (form, name))
            slots = cur.snapshot(); rings = hists.snapshot()
            for k, (s, _, first, count, _, to, h) in enumerate(jobs):
                if to is None:
                    continue
                row = min((first + count + 255) // 256 * 256, s.n)
                if h is not None:
                    assert (slots[to], rings[h]) == self.chain_hist[(self.hist.index(s), row)], (s.label, row)
                elif s in self.hist:
                    assert PR.words_of(slots[to]) == A.pack_cursor(A.POSITION, row, 0, s.n, LH.dtype_of(s)), (s.label, row)
                else:
                    assert slots[to] == self.chain_fast[(self.fast.index(s), row)], (s.label, row)
        return out

    def reads_hist_some(self, form): return self.reads_hist(form, True)
    def reads_hist_none(self, form): return self.reads_hist(form, False)
    def reads_ex_of_hist_none(self, form): return self.reads_hist(form, False, "ex")

    def index_hist(self, form, with_hist, entry="hist"):
        import test_gpu_lookback_history as LH
        import test_gpu_lookback_index as LI
        import test_gpu_page_index as PI
        import test_gpu_page_reads as PR
        import test_page_reads_abi as A
        from pcodec_amd import _lib as G
        pages = [self.hist[0], self.hist[1], self.hist[0], self.fast[3], self.hist[1]]
        every = [512, 512, 512, 512, 4096]   # (the last: k == 0)
        stride = [LI.stride_of(self.L, s) if with_hist and k in (0, 1, 4) else None for k, s in enumerate(pages)]
        jobs = [(s, None, e, st) for s, e, st in zip(pages, every, stride)]
        (code, rec, got, hgot), names = self.profiled(lambda: LI.IndexHistCall(self.L, jobs, form, 0, entry).finish())
        assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
        with_pairs = [j for j in range(len(jobs)) if stride[j]]
        if with_pairs:
            LI.check_pairs(self.L, [jobs[j] for j in with_pairs], [self.hist.index(pages[j]) for j in with_pairs], rec[with_pairs], [got[j] for j in with_pairs],
                           [hgot[j] for j in with_pairs], self.chain_hist, form)
        for j, (s, _, e, st) in enumerate(jobs):
            if st:
                continue
            k = PI.index_len(s.n, e)
            assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j]) == (G.ST_OK, k, 0) and len(got[j]) == k, (s.label, rec[j])
            for i in range(k):
                if s in self.hist:
                    assert PR.words_of(got[j][i]) == A.pack_cursor(A.POSITION, (i + 1) * e, 0, s.n, LH.dtype_of(s)), (s.label, i)
                else:
                    assert got[j][i] == self.chain_fast[(self.fast.index(s), (i + 1) * e)], (s.label, i)
        return {"index": names}

    def index_hist_some(self, form): return self.index_hist(form, True)
    def index_hist_none(self, form): return self.index_hist(form, False)
    def index_ex_of_hist_none(self, form): return self.index_hist(form, False, "ex")

    # ---- the second round, and the passes under a narrowed budget ----
    def second_round_reads(self, form):
        """test_gpu_page_reads.py's test_lookback_with_a_delta_d_secondary_variable_in_two_reads with two lanes: synchronous -- a second history buffer, taken
        when asked for; asynchronous -- PCO_GFX_UNSUPPORTED, dst and `to` untouched"""
        import test_gpu_page_reads as PR
        import test_page_reads_abi as A
        from pcodec_amd import _lib as G
        s = self.second; lanes = 2; dtype = G.DTYPE_BYTE["float32"]
        cur = PR.Cursors(2 * lanes)
        for k in range(lanes):
            cur.put(2 * k, A.pack_cursor(A.POSITION, 1024, 0, s.n, dtype))
        jobs = [(s, None, 1100, 700, 2 * k, 2 * k + 1) for k in range(lanes)]
        before = cur.snapshot()
        (code, rec, got), names = self.profiled(lambda: PR.run_reads(self.L, jobs, cur, form))
        slots = cur.snapshot()
        if form == "async":
            assert code == G.PcoSuccess and list(rec["status"]) == [G.ST_UNSUPPORTED] * lanes and (rec["n_out"] == 0).all()
            assert all(g is None for g in got) and slots == before
        else:
            assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
            PR.check_ok(jobs, rec, got, form)
            assert all(PR.words_of(slots[2 * k + 1]) == A.pack_cursor(A.POSITION, 2048, 0, s.n, dtype) for k in range(lanes))
        return {"reads": names}

    def second_round_index(self, form):
        import test_gpu_page_index as PI
        import test_gpu_page_reads as PR
        import test_page_reads_abi as A
        from pcodec_amd import _lib as G
        s = self.second; jobs = [(s, None, 512), (s, None, 1024)]
        (code, rec, got), names = self.profiled(lambda: PI.run_index(self.L, jobs, form))
        if form == "async":
            assert code == G.PcoSuccess and list(rec["status"]) == [G.ST_UNSUPPORTED] * 2 and (rec["n_out"] == 0).all()
            assert all(raw == PR.UNWRITTEN for g in got for raw in g)
        else:
            assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
            for j, (_, _, e) in enumerate(jobs):
                assert (rec["status"][j], rec["n_out"][j]) == (G.ST_OK, PI.index_len(s.n, e))
                assert [PR.words_of(raw) for raw in got[j]] == [A.pack_cursor(A.POSITION, (i + 1) * e, 0, s.n, G.DTYPE_BYTE["float32"]) for i in range(len(got[j]))]
        return {"index": names}

    def reads_in_budget_passes(self, form):
        """twelve whole-page reads of the Lookback page, 13 KB of scratch each, under 100 KB a pass: two passes"""
        import test_gpu_page_reads as PR
        from pcodec_amd import _lib as G
        s = self.back[0]; jobs = [(s, None, 0, s.n, None, k) for k in range(12)]
        cur = PR.Cursors(12)
        with PR.small_passes():
            (code, rec, got), names = self.profiled(lambda: PR.run_reads(self.L, jobs, cur, form))
        assert code == G.PcoSuccess, self.L.pco_gfx_last_error()
        PR.check_ok(jobs, rec, got, form)
        assert all(raw == self.chain_back0[(0, s.n)] for raw in cur.snapshot())
        return {"reads": names}

    # ---- directory forms ----
    def ranges_dir(self, form, defect=False):
        import test_gpu_page_directory as D
        from pcodec_amd import _lib as G
        b = D.blob_of(self.L, "classic+consecutive1", 4); c = b.c; n = c.n_pieces
        want = [(i, p, f, cnt) for i in range(c.k) for p, page_n in enumerate(c.pages[i]) for f, cnt in ((0, page_n), (255, 2), (page_n // 2, 0))]

        def swap(o): o[n - 1], o[n] = o[n], o[n - 1]   # (the last page of the last chunk loses its pair; every other piece keeps its extent)
        failing = {j: G.ST_INVALID_ARGUMENT for j, (i, p, _, cnt) in enumerate(want) if int(c.piece_first[i]) + 1 + p == n - 1 and cnt} if defect else {}
        assert len(failing) == (2 if defect else 0)
        job = D.Job(c, want, ranges=True)
        directory = b.directory(offs=D.edited(b, swap)) if defect else b.directory()
        (code, status), names = self.profiled(lambda: job.launch(directory, form))
        job.check(c.infos, code, status, form, failing)
        return {"ranges_dir": names}

    def ranges_dir_one_refused(self, form): return self.ranges_dir(form, True)

    def reads_dir(self, form, defect=False):
        """every page of the classic+lookback chunks cut at the cursors (and histories) of its index: the pointer form's call, then the _dir form's"""
        import test_gpu_page_reads_dir as RD
        from pcodec_amd import _lib as G
        b = RD.blob_of(self.L, "classic+lookback", 4); lay = RD.Layout()
        index = RD.built_index(self.L, "classic+lookback", 4, 0, True)
        if defect:
            src, bad_pages = RD.defective(self.L, "classic+lookback", "swapped pair")
            tasks, _ = RD.segment_tasks(self.L, b.c, lay, index, True, own=True)
            failing = {j: bad_pages[t["i"], t["p"]] for j, t in enumerate(tasks) if (t["i"], t["p"]) in bad_pages}
            assert 0 < len(failing) < len(tasks)
            (a, res), names = self.profiled(lambda: RD.both(self.L, src, tasks, lay, 0, form, failing=failing, what="reads_dir, one pair refused"))
            assert [r[0] for r in RD.tuples(res)] == [failing.get(j, 0) for j in range(len(tasks))]
        else:
            tasks, page_dst = RD.segment_tasks(self.L, b.c, lay, index, True)
            (a, res), names = self.profiled(lambda: RD.both(self.L, RD.Source(b), tasks, lay, 0, form, what="reads_dir"))
            assert [r[0] for r in RD.tuples(res)] == [0] * len(tasks)
            RD.rows_equal_the_input(b.c, a[1], page_dst, "reads_dir")
        return {"pointer form, then _dir form": names}

    def reads_dir_one_refused(self, form): return self.reads_dir(form, True)

    def index_dir(self, form):
        import test_gpu_page_reads_dir as RD
        b = RD.blob_of(self.L, "classic+lookback", 4); lay = RD.Layout()
        tasks = RD.index_tasks(self.L, b.c, lay, 512, True)
        (a, res), names = self.profiled(lambda: RD.both(self.L, RD.Source(b), tasks, lay, 0, form, what="index_dir"))
        assert [r[:2] for r in RD.tuples(res)] == [(0, t["k"]) for t in tasks]
        return {"pointer form, then _dir form": names}

    def chunk_reads_dir(self, form):
        """the standalone Lookback chunks in two slices, each chunk's one cursor and one history beside it"""
        import test_gpu_chunk_directory as CD
        b = CD.blob_of(self.L, "lookback", 4); e = b.e; lay = CD.Layout(); pages = []
        for i, a in enumerate(e.arrays):
            pages.append(dict(i=i, n=a.size, w=a.itemsize, dst=lay.take(a.nbytes), cur=lay.take(256), stride=CD.stride_of(self.L, e, i)))
            pages[-1]["hist"] = lay.take(pages[-1]["stride"])
        areas = lay.areas(); out = {}
        for s, (row, upto) in enumerate(((0, 512), (512, 1 << 20))):
            tasks = []
            for pg in pages:
                count = min(upto, pg["n"]) - row
                tasks.append(dict(i=pg["i"], first=row, count=count, dst_off=pg["dst"] + row * pg["w"], to_off=pg["cur"], from_off=pg["cur"] if s else None, history_off=pg["hist"],
                                  history_len=pg["stride"], extents=[(pg["dst"] + row * pg["w"], count * pg["w"]), (pg["cur"], 256), (pg["hist"], pg["stride"])]))
            (_, res), out[f"slice {s}: pointer form, then _dir form"] = self.profiled(lambda: CD.both(self.L, CD.Source(b), tasks, lay, 0, form, areas=areas, what=f"chunk slice {s}"))
            assert [r[0] for r in CD.tuples(res)] == [0] * len(tasks)
        CD.rows_equal_the_input(e, areas[1], [(pg["i"], 0, pg["n"], pg["dst"]) for pg in pages], "chunk_reads_dir")
        return out

    def chunk_index_dir(self, form):
        import test_gpu_chunk_directory as CD
        b = CD.blob_of(self.L, "lookback", 4); lay = CD.Layout()
        tasks = CD.index_tasks(self.L, b.e, lay, 512, True)
        (a, res), names = self.profiled(lambda: CD.both(self.L, CD.Source(b), tasks, lay, 0, form, what="chunk_index_dir"))
        assert [r[:2] for r in CD.tuples(res)] == [(0, t["k"]) for t in tasks]
        return {"pointer form, then _dir form": names}


def child():
    """Every case in its forms, up to the first that fails; prints `REPORT {case: {form: {call name: [launches]} or {"error": text}}}`."""
    import traceback
    sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
    from pcodec_amd import _lib as G
    L = G.lib()
    assert L.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    m = Matrix(L)
    rep = {}; failed = None
    for name, forms in CASES.items():
        rep[name] = {}
        for form in forms:
            if failed:   # (nothing more is started on a device after a call on it went wrong)
                rep[name][form] = {"error": f"not run: {failed} failed before it"}
                continue
            try:
                rep[name][form] = getattr(m, name)(form)
            except Exception:
                rep[name][form] = {"error": traceback.format_exc()[-1500:]}; failed = f"{name} ({form})"
    print("REPORT " + json.dumps(rep))


def run_child():
    env = {k: v for k, v in os.environ.items() if not k.startswith("PCO_GFX_")}
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("REPORT ")][-1][7:])


@pytest.fixture(scope="module")
def report():
    return run_child()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_matrix_is_the_recorded_one(report, golden):
    assert set(report) == set(golden) == set(CASES)
    assert all(set(report[c]) == set(golden[c]) == set(CASES[c]) for c in CASES)


@pytest.mark.parametrize("case,form", [(c, f) for c, forms in CASES.items() for f in forms])
def test_launch_sequence(report, golden, case, form):
    got, want = report[case][form], golden[case][form]
    assert "error" not in got, got["error"]
    assert set(got) == set(want)
    for call in want:
        assert got[call] == want[call], (case, form, call, [(i, a, b) for i, (a, b) in enumerate(zip(got[call], want[call])) if a != b][:4], len(got[call]), len(want[call]))


def test_the_recording_reaches_what_the_matrix_names(golden):
    """The calls were chosen for the branches they take; the recording must show them (else a case has quietly stopped covering its branch)."""
    def names(case, form="sync", call=None):
        calls = golden[case][form]
        return [n for c in calls if call in (None, c) for n in calls[c]]

    def has(case, stem, form="sync", call=None):
        return any(n.startswith(stem) for n in names(case, form, call))

    for form in BOTH:
        assert names("ranges_u64", form) == ["dec_walk_range_kernel<u64>", "dec_walk4_range_kernel<u64>", "dec_expand_range_kernel<u64>"] + (["pco_decode_prefix_kernel<u64>", "range_copy_kernel<u64>"] if form == "async" else [])
        assert [n for n in names("ranges_all_widths", form) if n.startswith("dec_walk_range")] == [f"dec_walk_range_kernel<{w}>" for w in ("u64", "u32", "u16", "u8")]
        for kind in ("range", "resume", "index"):
            assert has({"range": "ranges_k4", "resume": "reads_k4", "index": "index_k4"}[kind], f"dec_walk4_{kind}_kernel<u32>", form)
        # the walkers hand Lookback, Conv1 and Dict pages back: without the flag the prefix kernel, under it the general kernels in its place
        assert has("reads_handed_back_flags0", "pco_decode_prefix_kernel", form) and not has("reads_handed_back_flags0", "pco_decode_general", form)
        assert has("reads_handed_back_general", "pco_decode_general_resume_kernel", form) and not has("reads_handed_back_general", "pco_decode_prefix_kernel", form)
        assert "reads_shadow_kernel" in names("reads_handed_back_general", form) and "reads_finish_kernel" in names("reads_handed_back_flags0", form)
        assert has("index_handed_back_general", "pco_decode_general_index_kernel", form) and has("index_handed_back_flags0", "pco_decode_prefix_kernel", form)
        assert "index_finish_kernel" in names("index_handed_back_flags0", form) and "index_finish_kernel" in names("index_handed_back_general", form)
        assert not has("index_handed_back_flags0", "range_copy_kernel", form)
        # histories
        assert "reads_shadow_hist_kernel" in names("reads_hist_some", form) and has("reads_hist_some", "pco_decode_general_resume_kernel", form)
        assert has("index_hist_some", "pco_decode_general_index_hist_kernel", form) and has("index_hist_some", "index_history_snapshot_kernel", form)
        assert golden["index_hist_none"][form] == golden["index_ex_of_hist_none"][form], "a call of pco_gfx_index_pages_hist without a history is the _ex call"
        assert not has("index_hist_none", "index_history_snapshot_kernel", form)
        # directory forms
        assert "dir_resolve_kernel" in names("ranges_dir", form) and "dir_resolve_kernel" in names("ranges_dir_one_refused", form) and "dir_resolve_kernel" in names("index_dir", form)
        assert "dir_resolve_reads_kernel" in names("reads_dir", form) and "dir_resolve_reads_kernel" in names("reads_dir_one_refused", form)
        assert "dir_resolve_chunks_reads_kernel" in names("chunk_reads_dir", form) and "dir_resolve_chunks_kernel" in names("chunk_index_dir", form)
    # a synchronous read with a `from` reads the rows back; one without does not, and neither does the asynchronous form
    assert "reads_rows_kernel" in names("reads_u64", "sync", "second") and "reads_rows_kernel" not in names("reads_u64", "sync", "first")
    assert "reads_rows_kernel" not in names("reads_u64", "async")
    # the second round: the synchronous forms decode the page twice, the second time with the second history buffer; the asynchronous ones once
    for case, stem in (("second_round_reads", "pco_decode_prefix_kernel<u32>"), ("second_round_index", "pco_decode_prefix_kernel<u32>")):
        assert names(case, "sync").count(stem) == 2 and names(case, "async").count(stem) == 1, case
    assert names("reads_in_budget_passes").count("pco_decode_prefix_kernel<u32>") == 2 and names("reads_in_budget_passes").count("range_copy_kernel<u32>") == 2


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:   # the recorder
        rep = run_child()
        errors = {(c, f): v["error"] for c, forms in rep.items() for f, v in forms.items() if "error" in v}
        assert not errors, errors
        out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
        with open(out, "w") as f:
            json.dump(rep, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"recorded {len(rep)} cases into {out}")
