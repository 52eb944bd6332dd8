"""-m gpu: pco_gfx_decompress_page_reads_hist (include/pco_gfx.h section 4i) -- a Lookback page read in slices from a kind-4 cursor and a history ring.
Streams come from the library's wrapped writer and from the test-only generator (windows of 2 to 4096 rows, states of 1 to 256, random lookbacks up to
the full window and the reference's own search, a table beyond the general kernel's LDS); truth is the input array, the stepped tANS model of
tests/test_lookback_history_abi.py and the latents.  Every dst, cursor and history sits between canary bytes that are checked after every call; a
slot nobody wrote is canary bytes itself.  The helpers are the existing modules'; the library handle they take is wrapped so that their read calls
go through the new entry point with a history per task."""
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
import test_gpu_page_ranges as R  # noqa: E402  (Stream, write_pages, Pool, meta_info, numbers, profiled_ms)
import test_page_reads_abi as A  # noqa: E402  (the cursor's layout restated)
import test_gpu_page_reads as PR  # noqa: E402  (Cursors, Call, check_ok, the canaries, small_passes)
import test_gpu_general_cursors as GC  # noqa: E402  (Flagged: the _ex entry point as the yardstick)
import test_lookback_history_abi as HA  # noqa: E402  (kind 4 and the history restated, the stepped model with its delta variable)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec  # noqa: E402

pytestmark = pytest.mark.gpu
N_LONG, N_EVEN = PR.N_LONG, PR.N_EVEN
CANARY, GUARD, UNWRITTEN = PR.CANARY, PR.GUARD, PR.UNWRITTEN
LOOKBACK, POSITION = HA.LOOKBACK, A.POSITION


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


class Histories:
    """History buffers of the given sizes in one device tensor, each 8-byte aligned between guard bytes; everything starts as canary bytes."""

    def __init__(self, sizes):
        import torch
        self.sizes = list(sizes); self.offs = []; at = GUARD
        for s in self.sizes:
            self.offs.append(at); at += (s + 7) // 8 * 8 + GUARD
        self.dev = torch.full((at,), CANARY, dtype=torch.uint8, device="cuda")

    def ref(self, i, length=None):
        """(pointer, length) of buffer i for a task; (None, 0) for no history"""
        return (None, 0) if i is None else (self.dev.data_ptr() + self.offs[i], self.sizes[i] if length is None else length)

    def put(self, i, raw):
        import torch
        self.dev[self.offs[i]: self.offs[i] + len(raw)] = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        host = self.dev.cpu().numpy()
        mask = np.ones(host.size, bool)
        for o, s in zip(self.offs, self.sizes):
            mask[o: o + s] = False
        assert (host[mask] == CANARY).all(), "bytes around a history were written"
        return [host[o: o + s].tobytes() for o, s in zip(self.offs, self.sizes)]


class WithHistories:
    """The library with pco_gfx_decompress_page_reads routed through pco_gfx_decompress_page_reads_hist under `flags`, task i with the history refs[i]:
    what PR.Call calls."""

    def __init__(self, lib, refs, flags=0):
        self._lib, self._refs, self._flags = lib, refs, flags

    def pco_gfx_decompress_page_reads(self, n, tasks, res, d_res, stream):
        assert n == len(self._refs)
        self.tasks = (G.PageReadHistTask * n)(*[G.PageReadHistTask(*[getattr(tasks[i], f) for f, _ in G.PageReadTask._fields_], *self._refs[i]) for i in range(n)])
        return self._lib.pco_gfx_decompress_page_reads_hist(n, self.tasks, self._flags, res, d_res, stream)

    def __getattr__(self, name):
        return getattr(self._lib, name)


def run_hist(L, jobs, cur, hists, form="sync", flags=0):
    """jobs: [(Stream, page bytes or None, first, count, from slot, to slot, history slot or None or an explicit (slot, length))]"""
    refs = [hists.ref(*h) if isinstance(h, tuple) else hists.ref(h) for *_, h in jobs]
    return PR.Call(WithHistories(L, refs, flags), [j[:6] for j in jobs], cur, form).finish()


def dtype_of(s):
    return G.DTYPE_BYTE[s.nums.dtype.name]


def hist_bytes(L, s):
    return L.pco_gfx_lookback_history_bytes(s.wl, dtype_of(s))


# ---------------------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------------------
def seasonal(dt, n, seed, period=37):
    rng = np.random.default_rng(seed)
    hi = 100 if np.dtype(dt).itemsize == 1 else 5000
    return (np.tile(rng.integers(0, hi, period), n // period + 1)[:n] + rng.integers(0, 3, n)).astype(dt)


GENERATED = [  # (dtype, n, window_n_log, state_n_log, lookback_seed, mode, foreign table)
    (np.uint8, N_LONG, 1, 0, 3, "classic", False), (np.uint16, N_EVEN, 2, 1, 5, "classic", False), (np.uint32, N_LONG, 4, 4, 7, "classic", False),
    (np.uint64, N_EVEN, 8, 8, 9, "classic", False), (np.uint32, N_EVEN, 9, 0, 0, "classic", False), (np.uint64, N_LONG, 12, 1, 11, "classic", False),
    (np.uint16, N_LONG, 8, 0, 0, "classic", False), (np.uint8, N_EVEN, 9, 4, 21, "classic", False),
    (np.int64, N_LONG, 8, 4, 13, "int_mult", False), (np.int64, N_EVEN, 12, 8, 0, "int_mult", False), (np.int64, N_LONG, 2, 0, 17, "int_mult", False),
    (np.uint32, N_LONG, 9, 1, 15, "classic", True),
]


@pytest.fixture(scope="module")
def streams(L):
    """[Stream] with .mode, .wl, .sl (window_n_log, state_n_log) and .model (HA.model_lookback)"""
    out = []
    for s in R.write_pages(L, [("writer int64 periodic", R.numbers(np.int64, N_LONG, 8, period=365))], PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK)):
        s.mode = "classic"; out.append(s)
    fm = (np.tile(np.random.default_rng(4).integers(-2000, 2000, 91), N_EVEN // 91 + 1)[:N_EVEN] / 100.0).astype(np.float64)
    for s in R.write_pages(L, [("writer float64 float-mult", fm)], PR.per(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=G.DELTA_TRY_LOOKBACK)):
        s.mode = "float_mult"; out.append(s)
    for dt, n, wl, sl, seed, mode, foreign in GENERATED:
        kw = dict(tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=14, tbl_n_bins=300, tbl_seed=2) if foreign else {}
        if mode == "int_mult":
            rng = np.random.default_rng(seed + 40)
            x = (np.tile(rng.integers(0, 300, 37), n // 37 + 1)[:n] * 10 + rng.integers(0, 4, n)).astype(dt)
            kw.update(mode=O.MODE_TRY_INT_MULT, mode_u64=10)
        else:
            x = seasonal(dt, n, seed + 40); kw.update(mode=O.MODE_CLASSIC)
        s = PR.from_generator(f"{mode} {np.dtype(dt).name} n={n} window 2^{wl} state 2^{sl} seed {seed}{' asl 14' if foreign else ''}", x, delta=O.TE_DELTA_LOOKBACK,
                              window_n_log=wl, state_n_log=sl, lookback_seed=seed, **kw)
        s.mode = mode; out.append(s)
    for s in out:
        i = R.meta_info(L, s)
        assert i.delta_kind == 2 and i.secondary_uses_delta == 0, s.label
        s.wl, s.sl = int(i.window_n_log), int(i.state_n_log)
        s.model = HA.model_lookback(s.meta, s.page, s.n, s.nums.dtype.itemsize * 8)
        assert (s.model["window_n_log"], s.model["state_n_log"]) == (s.wl, s.sl)
    return out


def test_the_streams_are_what_they_are_called(L, streams):
    infos = [R.meta_info(L, s) for s in streams]
    assert [i.mode_kind for i in infos[:2]] == [0, 2] and all(i.mode_kind == {"classic": 0, "int_mult": 1}[s.mode] for i, s in list(zip(infos, streams))[2:])
    for (dt, n, wl, sl, seed, mode, foreign), s, i in zip(GENERATED, streams[2:], infos[2:]):
        assert (s.nums.dtype, s.n, s.wl, s.sl) == (np.dtype(dt), n, wl, sl)
        assert (i.ans_size_log[1] == 14) == foreign
        far = max(s.model["lookbacks"])
        assert far <= min(1 << wl, s.n - 1) and (not seed or far == 1 << wl or (1 << wl) > s.n - 256 and far > s.n // 2), (s.label, far)   # a seeded stream reaches the window's far end
    assert {s.wl for s in streams[2:]} == {1, 2, 4, 8, 9, 12} and {s.sl for s in streams[2:]} == {0, 1, 4, 8}
    assert {s.nums.dtype.name for s in streams} >= {"uint8", "uint16", "uint32", "uint64", "int64", "float64"} and {s.n for s in streams} == {N_LONG, N_EVEN}
    for s in streams:   # the model agrees with the input: F is the primary-latent history
        lat = [int(v) for v in TM.to_latent(s.nums)]
        if s.mode == "classic":
            assert s.model["F"] == lat, s.label
        elif s.mode == "int_mult":
            assert [p * 10 + q for p, q in zip(s.model["F"], s.model["secondary"])] == lat, s.label


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. chains
# ---------------------------------------------------------------------------------------------------------------------------------------
CHAINS = ["256", "512", "768", "one"]


def chain_sizes(n, chain):
    if chain == "one":
        return [n]
    k = int(chain)
    return [k] * (n // k) + ([n % k] if n % k else [])


def walk_chains(L, streams, form, flags=0):
    """Every stream through every chain, step t of all of them in call t; each lane owns two cursor slots and ONE history, updated in place.  Chain
    "256" reads and writes one slot (to == from).  Returns {(stream index, row): (the cursor's 256 bytes, the history's bytes)}: the same bytes
    whichever chain reached the row."""
    lanes = [(si, c) for si in range(len(streams)) for c in CHAINS]
    cur = PR.Cursors(2 * len(lanes))
    hists = Histories([hist_bytes(L, streams[si]) for si, _ in lanes])
    sizes = {ln: chain_sizes(streams[ln[0]].n, ln[1]) for ln in lanes}
    pos = {ln: 0 for ln in lanes}; parts = {ln: [] for ln in lanes}
    seen = {}
    for t in range(max(len(v) for v in sizes.values())):
        jobs = []; who = []
        for k, ln in enumerate(lanes):
            if t >= len(sizes[ln]):
                continue
            a, b = (2 * k, 2 * k) if ln[1] == "256" else (2 * k + (t + 1) % 2, 2 * k + t % 2)
            jobs.append((streams[ln[0]], None, pos[ln], sizes[ln][t], None if t == 0 else a, b, k)); who.append((ln, b, k))
        code, rec, got = run_hist(L, jobs, cur, hists, form, flags)
        assert code == G.PcoSuccess, L.pco_gfx_last_error()
        PR.check_ok([j[:6] for j in jobs], rec, got, (form, t))
        slots = cur.snapshot(); rings = hists.snapshot()
        for (ln, b, k), job, g in zip(who, jobs, got):
            s = streams[ln[0]]
            parts[ln].append(g); pos[ln] += job[3]
            row = min((pos[ln] + 255) // 256 * 256, s.n)
            c = A.unpack_cursor(PR.words_of(slots[b]))
            assert (c["version"], c["kind"], c["row"], c["page_n"], c["dtype"]) == (A.VERSION, LOOKBACK, row, s.n, dtype_of(s)), (s.label, ln[1], t, c)
            assert seen.setdefault((ln[0], row), (slots[b], rings[k])) == (slots[b], rings[k]), ("the pair of a row differs between two chains", s.label, ln[1], row)
    for ln in lanes:
        assert pos[ln] == streams[ln[0]].n and U.bits_equal(np.concatenate(parts[ln]), streams[ln[0]].nums), (streams[ln[0]].label, ln[1])
    return seen


@pytest.fixture(scope="module")
def walked(L, streams):
    return walk_chains(L, streams, "sync")


def expected_ring(s, row, F):
    """the history's bytes at `row`: the stamp, F[j] at j & (w - 1) for the rows the stamp promises, canary bytes in the slots no row has reached"""
    w = 1 << s.wl; width = s.nums.dtype.itemsize
    reach = min(row + (1 << s.sl), s.n)
    ring = np.full(w * width, CANARY, np.uint8).view(f"<u{width}").copy()
    for j in range(max(0, reach - w), reach):
        ring[j % w] = F[j]
    return np.array(HA.pack_header(row, s.n, dtype_of(s), s.wl), np.uint64).tobytes() + ring.tobytes()


def test_chains_reach_every_batch_boundary_with_kind_4_cursors_and_the_stepped_model_s_fields(streams, walked):
    for si, s in enumerate(streams):
        assert sorted(r for i, r in walked if i == si) == [min(r + 256, s.n) for r in range(0, s.n, 256)], s.label
        for row, bit, states in s.model["marks"]:
            assert PR.words_of(walked[(si, row)][0]) == HA.pack_lookback(row, bit, s.n, dtype_of(s), states), (s.label, row)   # words 10..31 are zero
        assert len(s.model["marks"]) in (11, 12)


def test_the_ring_holds_the_latents_of_the_rows_the_stamp_promises_and_canaries_elsewhere(streams, walked):
    n_unreached = 0
    for si, s in enumerate(streams):
        F = [int(v) for v in TM.to_latent(s.nums)] if s.mode == "classic" else s.model["F"]
        for row in sorted(r for i, r in walked if i == si):
            raw = walked[(si, row)][1]
            assert len(raw) == 64 + (s.nums.dtype.itemsize << s.wl)
            assert raw == expected_ring(s, row, F), (s.label, row)
            n_unreached += min(row + (1 << s.sl), s.n) < 1 << s.wl
    assert n_unreached >= 3 * 11   # the windows of 4096 rows are never filled


@pytest.mark.parametrize("form", ["async", "sync in passes"])
def test_the_other_forms_reach_the_same_pairs(L, streams, walked, form):
    if form == "sync in passes":
        with PR.small_passes():
            again = walk_chains(L, streams, "sync")
    else:
        again = walk_chains(L, streams, form)
    assert again.keys() == walked.keys() and all(again[k] == walked[k] for k in walked)


def test_the_flag_changes_nothing_on_a_lookback_page(L, streams, walked):
    again = walk_chains(L, streams[:4], "sync", G.CURSOR_GENERAL)
    assert all(again[k] == walked[k] for k in again) and len(again) > 40


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3., 4. without a history, and beside pages that take none
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def others(L):
    """pages that are not resumable Lookback: [two-kernel classic, Conv1, Dict under Lookback, Lookback with a delta'd secondary]"""
    import torch  # noqa: F401
    out = R.write_pages(L, [("classic uint32", R.numbers(np.uint32, N_LONG, 3))], PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))
    out.append(PR.from_generator("conv1 uint16", R.numbers(np.uint16, N_EVEN, 2), mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=4, bias=5, weights=[-16, 32]))
    rng = np.random.default_rng(7)
    d = rng.integers(0, 1 << 30, 30).astype(np.uint32)[np.tile(rng.integers(0, 30, 41), N_LONG // 41 + 1)[:N_LONG]]
    out.append(PR.from_generator("dict+lookback uint32", d, mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1, lookback_seed=5))
    x = (np.cumsum(np.random.default_rng(3).integers(-5, 7, N_LONG)) / 4.0).astype(np.float32)
    out.append(PR.from_generator("lookback+secondary float32", x, mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1,
                                 secondary_uses_delta=True, lookback_seed=5))
    infos = [R.meta_info(L, s) for s in out]
    assert [i.mode_kind for i in infos] == [0, 0, 4, 2] and [infos[k].delta_kind for k in (0, 1, 3)] == [1, 3, 2] and infos[3].secondary_uses_delta == 1
    assert GC.dict_delta(out[2])[0] == 2   # (the variant behind the dictionary: Lookback)
    for s in out:
        s.wl = 8
    return out


@pytest.mark.parametrize("flags", [0, G.CURSOR_GENERAL])
def test_without_a_history_every_task_is_the_ex_task(L, streams, others, flags):
    """results, dst and cursors against pco_gfx_decompress_page_reads_ex under the same flags: Lookback pages keep kind 2 and the prefix decode"""
    pages = streams[:6] + others
    rng = np.random.default_rng(3)
    cur_a, cur_b = PR.Cursors(2 * len(pages)), PR.Cursors(2 * len(pages))
    hists = Histories([])
    jobs = []
    for k, s in enumerate(pages):
        row = int(rng.integers(1, s.n // 256)) * 256
        first = min(row + int(rng.integers(0, 300)), s.n - 1)
        jobs.append((s, None, first, int(rng.integers(1, s.n - first + 1)), 2 * k if k % 2 else None, 2 * k + 1, None))   # half from a position, half from the start
        for c in (cur_a, cur_b):
            c.put(2 * k, A.pack_cursor(POSITION, row, 0, s.n, dtype_of(s)))
    jobs.append((pages[0], pages[0].page[:40], 0, 600, None, None, None))   # ... and a task that fails
    for form in ("sync", "async"):
        a = PR.run_reads(GC.Flagged(L, flags), [j[:6] for j in jobs], cur_a, form); b = run_hist(L, jobs, cur_b, hists, form, flags)
        assert a[0] == b[0] and (a[1] == b[1]).all(), (form, a[1], b[1])
        assert all((x is None and y is None) or U.bits_equal(x, y) for x, y in zip(a[2], b[2]))
        assert cur_a.snapshot() == cur_b.snapshot()
        ok = [j for j in range(len(jobs) - 1) if a[1]["status"][j] == 0]
        # (in both: under the flag a Conv1 page refuses the position-only `from`, and the asynchronous form has no second history for the delta'd secondary)
        assert set(range(len(jobs) - 1)) - set(ok) <= {7, 9} and (flags or form == "async" or len(ok) == len(jobs) - 1), (form, a[1]["status"])
        PR.check_ok([jobs[j][:6] for j in ok], a[1][ok], [a[2][j] for j in ok], form)


@pytest.mark.parametrize("form", ["sync", "async"])
def test_one_mixed_call_leaves_the_histories_of_the_other_pages_alone(L, streams, others, walked, form):
    """a two-kernel page, a Conv1 page, resumable Lookback pages, Dict under Lookback and a delta'd secondary: every task has a history, only the
    resumable ones use it"""
    lb = [(0, streams[0]), (8, streams[8])]
    pages = [others[0], others[1], lb[0][1], lb[1][1], others[2], others[3]]
    hists = Histories([64 + (s.nums.dtype.itemsize << s.wl) for s in pages])
    cur = PR.Cursors(2 * len(pages))
    jobs = [(s, None, 0, 1024, None, 2 * k + 1, k) for k, s in enumerate(pages)]
    code, rec, got = run_hist(L, jobs, cur, hists, form, G.CURSOR_GENERAL)
    want_ok = [0, 1, 2, 3, 4] + ([5] if form == "sync" else [])
    assert [int(x) for x in rec["status"]] == [0, 0, 0, 0, 0, 0 if form == "sync" else G.ST_UNSUPPORTED]
    PR.check_ok([jobs[j][:6] for j in want_ok], rec[want_ok], [got[j] for j in want_ok], form)
    slots = cur.snapshot(); rings = hists.snapshot()
    kinds = [A.unpack_cursor(PR.words_of(slots[2 * k + 1]))["kind"] for k in want_ok]
    assert kinds == [A.FULL, 3, LOOKBACK, LOOKBACK, POSITION] + ([POSITION] if form == "sync" else [])
    for k in (0, 1, 4, 5):
        assert rings[k] == bytes([CANARY]) * len(rings[k]), pages[k].label
    for k, (si, _) in zip((2, 3), lb):
        assert (slots[2 * k + 1], rings[k]) == walked[(si, 1024)]
    # ... and the resumable ones go on from their pairs beside the others, which go on from their cursors
    jobs = [(s, None, 1024, s.n - 1024, 2 * k + 1, 2 * k, k) for k, s in enumerate(pages) if k in want_ok]
    code, rec, got = run_hist(L, jobs, cur, hists, form, G.CURSOR_GENERAL)
    PR.check_ok([j[:6] for j in jobs], rec, got, form)
    slots = cur.snapshot(); rings = hists.snapshot()
    for k, (si, s) in zip((2, 3), lb):
        assert (slots[2 * k], rings[k]) == walked[(si, s.n)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_a_refused_pair_refuses_its_task_alone(L, streams, walked, form):
    si, s = 8, streams[8]   # int-mult: three variables, two passes
    info = R.meta_info(L, s)
    cur512, ring512 = walked[(si, 512)]
    base = A.unpack_cursor(PR.words_of(cur512))
    hb = hist_bytes(L, s)
    hdr = lambda **kw: np.array(HA.pack_header(**dict(dict(row=512, page_n=s.n, dtype=dtype_of(s), window_n_log=s.wl), **kw)), np.uint64).tobytes() + ring512[64:]   # noqa: E731

    def edit(**kw):
        d = dict(row=base["row"], bit=base["bit"], page_n=base["page_n"], dtype=base["dtype"], states=base["states"], version=base["version"], kind=base["kind"])
        d.update(kw)
        return HA.pack_lookback(**d)

    def state(v, j, x):
        st = [list(r) for r in base["states"]]; st[v][j] = x
        return edit(states=st)

    assert edit() == PR.words_of(cur512) and hdr() == ring512
    good_cur, good_ring = PR.words_of(cur512), ring512
    # (name, `from` words or None, the history's bytes, the history the task names: "own", None, or a length)
    rows = [("a short history", good_cur, good_ring, hb - 1), ("a short history on a page that starts", None, good_ring, hb - 1), ("the header alone", good_cur, good_ring, 64),
            ("header version", good_cur, hdr(version=2), "own"), ("header page_n", good_cur, hdr(page_n=s.n - 1), "own"), ("header dtype", good_cur, hdr(dtype=2), "own"),
            ("header window_n_log", good_cur, hdr(window_n_log=s.wl - 1), "own"), ("header row", good_cur, hdr(row=768), "own"), ("header row 0", good_cur, hdr(row=0), "own"),
            ("kind 2 with a history", A.pack_cursor(POSITION, 512, 0, s.n, dtype_of(s)), good_ring, "own"), ("kind 4 without a history", good_cur, good_ring, None),
            ("kind 3 with a history", edit(kind=3), good_ring, "own"),
            ("cursor version", edit(version=2), good_ring, "own"), ("cursor page_n", edit(page_n=s.n - 1), good_ring, "own"), ("at > first", edit(row=768), hdr(row=768), "own"),
            ("at unaligned", edit(row=300), hdr(row=300), "own"), ("bit before the body", edit(bit=s.model["body"] - 1), good_ring, "own"),
            ("bit beyond the page", edit(bit=8 * len(s.page) + 1), good_ring, "own"), ("delta state 2^asl", state(0, 1, 1 << info.ans_size_log[0]), good_ring, "own"),
            ("primary state 2^asl", state(1, 2, 1 << info.ans_size_log[1]), good_ring, "own"), ("secondary state 2^asl", state(2, 0, 1 << info.ans_size_log[2]), good_ring, "own")]
    assert s.model["body"] > 0
    hists = Histories([hb] * (len(rows) + 1))
    cur = PR.Cursors(2 * len(rows) + 2)
    jobs = []
    for k, (_, words, ring, names) in enumerate(rows):
        if words is not None:
            cur.put(2 * k, words)
        hists.put(k, ring)
        jobs.append((s, None, 600 if words is not None else 0, 300, 2 * k if words is not None else None, 2 * k + 1, k if names == "own" else (None if names is None else (k, names))))
    g = len(rows)
    cur.put(2 * g, good_cur); hists.put(g, good_ring)
    jobs.insert(5, (s, None, 600, 300, 2 * g, 2 * g + 1, g))   # a good task among them
    before_c, before_h = cur.snapshot(), hists.snapshot()
    code, rec, got = run_hist(L, jobs, cur, hists, form)
    if form == "sync":
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT
    after_c, after_h = cur.snapshot(), hists.snapshot()
    for at, job in enumerate(jobs):
        k = job[5] // 2
        if k == g:
            PR.check_ok([job[:6]], rec[at: at + 1], got[at: at + 1], form)
            assert (after_c[2 * g + 1], after_h[g]) == walked[(si, 1024)]
            continue
        assert (rec["status"][at], rec["n_out"][at], rec["consumed"][at], rec["aux"][at]) == (G.ST_INVALID_ARGUMENT, 0, 0, 0), rows[k][0]
        assert got[at] is None, ("dst was written", rows[k][0])
        assert after_c[2 * k] == before_c[2 * k] and after_c[2 * k + 1] == UNWRITTEN and after_h[k] == before_h[k], rows[k][0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. - 9. damage, a read that keeps its pair, aliasing
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_a_page_damaged_behind_the_read_and_inside_it(L, streams, walked, form):
    for si in (0, 5, 8):   # the writer's page, a window beyond the page, int-mult's two passes
        s = streams[si]
        bit = lambda row: A.unpack_cursor(PR.words_of(walked[(si, row)][0]))["bit"]   # noqa: E731
        page = s.page[: bit(1536) // 8 + 1]     # every batch in front of row 1536 is whole; what follows is gone
        cur = PR.Cursors(4); hists = Histories([hist_bytes(L, s)] * 2)
        for k in range(2):
            cur.put(2 * k, PR.words_of(walked[(si, 512)][0])); hists.put(k, walked[(si, 512)][1])
        jobs = [(s, page, 600, 900, 0, 1, 0), (s, page, 600, 1200, 2, 3, 1)]   # rows [600, 1500) end in front of the damage; [600, 1800) run into it
        code, rec, got = run_hist(L, jobs, cur, hists, form)
        assert list(rec["status"]) == [G.ST_OK, G.ST_INSUFFICIENT_DATA] and list(rec["n_out"]) == [900, 0], (s.label, form, rec)
        assert U.bits_equal(got[0], s.nums[600:1500]) and got[1] is None
        slots = cur.snapshot(); rings = hists.snapshot()
        assert (slots[1], rings[0]) == walked[(si, 1536)] and slots[3] == UNWRITTEN and rings[1] == walked[(si, 512)][1], (s.label, form)


def test_a_read_without_to_keeps_the_pair_and_to_may_be_from(L, streams, walked):
    picks = [0, 1, 3, 8, 11]
    cur = PR.Cursors(2 * len(picks)); hists = Histories([hist_bytes(L, streams[si]) for si in picks])
    for k, si in enumerate(picks):
        cur.put(2 * k, PR.words_of(walked[(si, 768)][0])); hists.put(k, walked[(si, 768)][1])
    # to == NULL: rows inside the next batches, twice, then a read that crosses three boundaries without moving either
    for first, count in ((800, 100), (768, 256), (900, 700)):
        jobs = [(streams[si], None, first, count, 2 * k, None, k) for k, si in enumerate(picks)]
        code, rec, got = run_hist(L, jobs, cur, hists)
        assert code == G.PcoSuccess, L.pco_gfx_last_error()
        PR.check_ok([j[:6] for j in jobs], rec, got)
        slots = cur.snapshot(); rings = hists.snapshot()
        for k, si in enumerate(picks):
            assert (slots[2 * k], rings[k]) == walked[(si, 768)] and slots[2 * k + 1] == UNWRITTEN, streams[si].label
    # to == from, the history in place: the pair moves to row 1536, and on to the page's end
    for first, count, row in ((768, 768, 1536), (1536, None, None)):
        jobs = [(streams[si], None, first, count or streams[si].n - first, 2 * k, 2 * k, k) for k, si in enumerate(picks)]
        code, rec, got = run_hist(L, jobs, cur, hists)
        assert code == G.PcoSuccess, L.pco_gfx_last_error()
        PR.check_ok([j[:6] for j in jobs], rec, got)
        slots = cur.snapshot(); rings = hists.snapshot()
        for k, si in enumerate(picks):
            assert (slots[2 * k], rings[k]) == walked[(si, row or streams[si].n)], streams[si].label


def test_a_pair_of_another_page_of_the_same_chunk_stays_inside_every_buffer(L):
    """Same tables and window, another page's bit position, states and ring: wrong numbers or an error status, every canary intact."""
    x = seasonal(np.uint32, 2 * N_LONG, 9)
    pairs = []
    for wl, sl, seed in ((8, 1, 5), (4, 4, 0), (12, 8, 7)):
        meta, pages = O.test_encode(x, pages=[N_LONG, N_LONG], mode=O.MODE_CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=wl, state_n_log=sl, lookback_seed=seed)
        ab = [R.Stream(f"page {p} window 2^{wl}", x[p * N_LONG: (p + 1) * N_LONG], meta, pages[p]) for p in range(2)]
        for s in ab:
            s.wl = wl
        pairs.append(ab)
    flat = [s for ab in pairs for s in ab]
    cur = PR.Cursors(2 * len(flat)); hists = Histories([hist_bytes(L, s) for s in flat])
    jobs = [(s, None, 0, 1024, None, 2 * k, k) for k, s in enumerate(flat)]
    code, rec, got = run_hist(L, jobs, cur, hists)
    assert code == G.PcoSuccess
    PR.check_ok([j[:6] for j in jobs], rec, got)
    slots = cur.snapshot()
    for k, s in enumerate(flat):   # page k reads on from its sibling's pair, k ^ 1: the bit position kept inside this page
        c = A.unpack_cursor(PR.words_of(slots[2 * (k ^ 1)]))
        cur.put(2 * k + 1, HA.pack_lookback(1024, min(c["bit"], 8 * len(s.page)), s.n, c["dtype"], c["states"]))
    jobs = [(s, None, 1024, s.n - 1024, 2 * k + 1, 2 * k + 1, k ^ 1) for k, s in enumerate(flat)]
    code, rec, got = run_hist(L, jobs, cur, hists)   # (finish() checks the canaries around every dst)
    cur.snapshot(); hists.snapshot()
    assert all(st in (G.ST_OK, G.ST_INSUFFICIENT_DATA, G.ST_CORRUPTION) for st in rec["status"]), rec["status"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 11. the reader
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_chunk_reader_with_histories_returns_the_rows_of_the_default_reader(L):
    import torch
    lb = R.numbers(np.int64, 9000, 8, period=365)
    fm = (np.tile(np.random.default_rng(4).integers(-2000, 2000, 91), 60)[:5000] / 100.0).astype(np.float64)
    cd = R.numbers(np.int64, 5000, 9)
    cases = [(lb, "int64", ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_lookback()), [5000, 4000]),
             (fm, "float64", ChunkConfig(mode_spec=ModeSpec.try_float_mult(0.01), delta_spec=DeltaSpec.try_lookback()), [5000]),
             (cd, "int64", ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(1)), [3000, 2000])]
    for a, name, cfg, sizes in cases:
        cc = paged.compress_chunks([torch.from_numpy(a).cuda()], cfg, page_sizes=[sizes])
        dr = cc.directory
        for steps in ([256, 1024, 512], [2048, 256], [a.size]):
            plain = paged.ChunkReader(cc.blob, dr, [name], 0); hist = paged.ChunkReader(cc.blob, dr, [name], 0, history=True)
            assert (hist.histories is not None) == (name != "int64" or a is lb)
            L.pco_gfx_profile_begin()
            got = [hist.read(n).cpu().numpy() for n in steps if n <= a.size]
            got.append(hist.read(a.size - hist.pos).cpu().numpy())
            names = U.profile_names(L)
            want = [plain.read(n).cpu().numpy() for n in steps if n <= a.size]
            want.append(plain.read(a.size - plain.pos).cpu().numpy())
            assert all(U.bits_equal(g, w) for g, w in zip(got, want)) and U.bits_equal(np.concatenate(got), a), (name, steps)
            if hist.histories is not None:
                assert any(n.startswith("pco_decode_general_resume_kernel") for n in names) and not any(n.startswith("pco_decode_prefix_kernel") for n in names), names


# ---------------------------------------------------------------------------------------------------------------------------------------
# 12. the work follows the slice
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_work_of_a_lookback_read_follows_its_slice(L):
    """One i64 Lookback page of 2^18 numbers (2^20 when the whole page decodes in under 2 ms).  Kernel time from pco_gfx_profile_*: (a) rows
    [15 n / 16, n) from a saved pair against the same rows through pco_gfx_decompress_page_ranges: 1/16 of the batches by construction, at most 1/4;
    (b) the page as sixteen chained reads against sixteen pco_gfx_decompress_page_reads_ex reads of the same slices, each of which decodes its prefix:
    16 against 136 slice-units of batches by construction (0.12), at most 1/2."""
    import torch

    def setup(n):
        s = R.write_pages(L, [(f"lookback int64 2^{n.bit_length() - 1}", R.numbers(np.int64, n, 8, period=365))],
                          G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK, max_page_n=n))[0]
        i = R.meta_info(L, s)
        assert i.delta_kind == 2
        s.wl = int(i.window_n_log)
        return s

    def measure(s):
        n = s.n; seg = n // 16; w = 8; dt = G.DTYPE_BYTE["int64"]
        pool = R.Pool([s.meta, s.page])
        hb = L.pco_gfx_lookback_history_bytes(s.wl, dt)
        whole = torch.zeros(n * w + 64, dtype=torch.uint8, device="cuda")
        part = torch.zeros(seg * w + 64, dtype=torch.uint8, device="cuda")
        curs = torch.zeros((3, 256), dtype=torch.uint8, device="cuda")                     # the chain's cursor, the saved one, the _ex chain's
        rings = torch.zeros((2, (hb + 7) // 8 * 8), dtype=torch.uint8, device="cuda")       # the chain's history, the saved one
        cptr = lambda k: curs.data_ptr() + 256 * k   # noqa: E731
        hptr = lambda k: rings.data_ptr() + k * rings.shape[1]   # noqa: E731

        def hist_read(dst, first, count, fr, to, h):
            t = (G.PageReadHistTask * 1)(G.PageReadHistTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), dst, n, first, count, dt, 4, fr, to, hptr(h), hb)); res = (G.TaskResult * 1)()
            G.check(L.pco_gfx_decompress_page_reads_hist(1, t, 0, res, None, None))

        def ex_read(dst, first, count, fr, to):
            t = (G.PageReadTask * 1)(G.PageReadTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), dst, n, first, count, dt, 4, fr, to)); res = (G.TaskResult * 1)()
            G.check(L.pco_gfx_decompress_page_reads_ex(1, t, 0, res, None, None))

        def chain():
            for k in range(16):
                hist_read(whole.data_ptr() + w * k * seg, k * seg, seg, cptr(0) if k else None, cptr(0), 0)
                if k == 14:   # the pair in front of the last slice, saved
                    curs[1].copy_(curs[0]); rings[1].copy_(rings[0])

        def ex_chain():
            for k in range(16):
                ex_read(whole.data_ptr() + w * k * seg, k * seg, seg, cptr(2) if k else None, cptr(2))

        def last_as_range():
            t = (G.PageRangeTask * 1)(G.PageRangeTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), part.data_ptr(), n, 15 * seg, seg, dt, 4)); res = (G.TaskResult * 1)()
            G.check(L.pco_gfx_decompress_page_ranges(1, t, res, None, None))

        ms_ex = R.profiled_ms(L, ex_chain)
        assert U.bits_equal(whole[: n * w].cpu().numpy().view(np.int64), s.nums)
        whole.zero_()
        L.pco_gfx_profile_begin()
        chain()
        names = U.profile_names(L)
        assert any(k.startswith("pco_decode_general_resume_kernel") for k in names) and not any(k.startswith("pco_decode_prefix_kernel") for k in names), names
        ms_chain = R.profiled_ms(L, chain)
        assert U.bits_equal(whole[: n * w].cpu().numpy().view(np.int64), s.nums)
        ms_range = R.profiled_ms(L, last_as_range)
        part.zero_()
        ms_read = R.profiled_ms(L, lambda: hist_read(part.data_ptr(), 15 * seg, seg, cptr(1), None, 1))
        assert U.bits_equal(part[: seg * w].cpu().numpy().view(np.int64), s.nums[15 * seg:])
        return ms_range, ms_read, ms_ex, ms_chain

    s = setup(1 << 18)
    ms = measure(s)
    if ms[0] < 2.0:
        s = setup(1 << 20); ms = measure(s)
    ms_range, ms_read, ms_ex, ms_chain = ms
    print(f"{s.label}: rows [15 n / 16, n): as a range {ms_range:.3f} ms, from a saved pair {ms_read:.3f} ms; the page in sixteen chained reads: position-only cursors "
          f"{ms_ex:.3f} ms, kind-4 cursors and a history {ms_chain:.3f} ms")
    assert ms_read <= ms_range / 4, (ms_read, ms_range)
    assert ms_chain <= ms_ex / 2, (ms_chain, ms_ex)
