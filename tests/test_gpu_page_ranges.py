"""-m gpu: pco_gfx_decompress_page_ranges (include/pco_gfx.h section 4d) -- rows [first, first + count) of a wrapped page without decoding the
rest.  Streams come from the library's own wrapped writer (pco_gfx_compress_wrapped_chunks_ex, whose bytes other tests pin to the oracle) and,
for lookback with a delta'd secondary variable, from the test-only generator; truth is the input array.  Every dst sits between canary bytes
that are checked after every call."""
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
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec, PagingSpec  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


class Stream:
    def __init__(self, label, nums, meta, page):
        self.label, self.nums, self.meta, self.page, self.n = label, np.ascontiguousarray(nums), bytes(meta), bytes(page), int(nums.size)


def write_pages(L, labelled, cfg):
    """One wrapped chunk of ONE page per array through pco_gfx_compress_wrapped_chunks_ex: [Stream]."""
    import torch
    arrays = [np.ascontiguousarray(a) for _, a in labelled]
    k = len(arrays)
    srcs = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in arrays]
    caps = [L.pco_gfx_wrapped_chunk_cap(a.size, G.DTYPE_BYTE[a.dtype.name], C.addressof(cfg)) for a in arrays]
    dsts = [torch.zeros(c + 64, dtype=torch.uint8, device="cuda") for c in caps]
    tasks = (G.WrappedTask * k)(*[G.WrappedTask(s.data_ptr(), a.size, d.data_ptr(), c, G.DTYPE_BYTE[a.dtype.name], 0, None) for a, s, d, c in zip(arrays, srcs, dsts, caps)])
    infos = (G.PageInfo * (2 * k))()
    G.check(L.pco_gfx_compress_wrapped_chunks_ex(k, tasks, C.addressof(cfg), infos, None, None))
    out = []
    for i, (label, a) in enumerate(labelled):
        host = dsts[i].cpu().numpy()
        m, e = infos[2 * i], infos[2 * i + 1]
        assert m.status == 0 and e.status == 0 and e.n == a.size, (label, m.status, e.status)
        out.append(Stream(label, a, host[: m.len], host[e.offset: e.offset + e.len]))
    return out


class Pool:
    """Byte strings side by side in one device tensor, each 16-byte aligned with 16 readable zero bytes behind it."""

    def __init__(self, blobs):
        import torch
        self.offs = []; at = 0
        for b in blobs:
            self.offs.append(at); at += (len(b) + 16 + 15) // 16 * 16
        host = np.zeros(at + 16, np.uint8)
        for o, b in zip(self.offs, blobs):
            host[o: o + len(b)] = np.frombuffer(b, np.uint8)
        self.dev = torch.from_numpy(host).cuda()

    def ptr(self, i):
        return self.dev.data_ptr() + self.offs[i]


def run_ranges(L, jobs, form="sync"):
    """jobs: [(Stream, page bytes or None for the stream's own, first, count)].  One call; returns (code, results as a numpy record array,
    [decoded range per job]) after checking every canary."""
    import torch
    blobs = []; index = {}
    for s, page, _, _ in jobs:
        for key, b in ((("m", id(s)), s.meta), (("p", id(s), id(page)), s.page if page is None else page)):
            if key not in index:
                index[key] = len(blobs); blobs.append(b)
    pool = Pool(blobs)
    spans = []; at = 0
    for s, _, _, count in jobs:
        w = s.nums.dtype.itemsize
        at += GUARD; spans.append(at); at += (count * w + 15) // 16 * 16
    total = at + GUARD
    out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    tasks = (G.PageRangeTask * len(jobs))()
    for j, (s, page, first, count) in enumerate(jobs):
        pg = s.page if page is None else page
        tasks[j] = G.PageRangeTask(pool.ptr(index[("m", id(s))]), len(s.meta), pool.ptr(index[("p", id(s), id(page))]), len(pg),
                                   (out.data_ptr() + spans[j]) if count else None, s.n, first, count, G.DTYPE_BYTE[s.nums.dtype.name], 4)
    if form == "sync":
        res = (G.TaskResult * len(jobs))()
        code = L.pco_gfx_decompress_page_ranges(len(jobs), tasks, res, None, None)
        rec = np.frombuffer(bytes(res), U.RES_DT).copy()
    else:   # d_results on a non-blocking stream
        st = torch.cuda.Stream()
        d_res = torch.zeros(len(jobs) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        code = L.pco_gfx_decompress_page_ranges(len(jobs), tasks, None, d_res.data_ptr(), C.c_void_p(st.cuda_stream))
        st.synchronize()
        rec = d_res.cpu().numpy().view(U.RES_DT).copy()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    mask = np.ones(total, bool); got = []
    for j, (s, _, first, count) in enumerate(jobs):
        w = s.nums.dtype.itemsize
        mask[spans[j]: spans[j] + count * w] = False
        got.append(host[spans[j]: spans[j] + count * w].view(s.nums.dtype))
    assert (host[mask] == CANARY).all(), "bytes outside dst[0 .. count * width) were written"
    return code, rec, got


def check_ok(jobs, rec, got, what=""):
    for j, (s, page, first, count) in enumerate(jobs):
        tag = (what, s.label, first, count)
        assert rec["status"][j] == G.ST_OK, (tag, int(rec["status"][j]))
        assert rec["n_out"][j] == count and rec["aux"][j] == 0, tag
        last = count > 0 and (first + count + 255) // 256 >= (s.n + 255) // 256
        assert rec["consumed"][j] == (len(s.page if page is None else page) if last else 0), (tag, int(rec["consumed"][j]))
        assert U.bits_equal(got[j], s.nums[first: first + count]), tag


# ---------------------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------------------
TYPES = [np.uint8, np.int16, np.float16, np.uint32, np.float32, np.int64, np.float64]
SIZES = [1, 255, 256, 257, 3000, 70000]


def numbers(dt, n, seed, period=0):
    dt = np.dtype(dt); rng = np.random.default_rng(seed)
    if period:   # seasonal: what a lookback delta finds
        base = rng.integers(-100, 100, period)
        y = base[np.arange(n) % period] * 3 + rng.integers(-1, 2, n)
    else:
        y = np.cumsum(rng.integers(-5, 7, n))
    if dt.kind == "f":
        return (y / 4.0).astype(dt)
    if dt.kind == "u":
        y = y - y.min()
    return (y % (1 << (8 * dt.itemsize - 1))).astype(dt) if dt.itemsize < 8 else y.astype(dt)


def ranges_of(n):
    want = [(0, 0), (0, 1), (255, 2), (256, 256), (n - 1, 1), (0, n), (n - 5, 5)]
    if n % 256 and n > 256:
        want.append((n - n % 256 + (n % 256) // 3, max(1, (n % 256) // 3)))   # inside the ragged last batch
    if n == 70000:
        want += [(40000, 1000), (65530, 12)]
    return sorted({(f, c) for f, c in want if f >= 0 and f + c <= n})


@pytest.fixture(scope="module")
def grid(L):
    """Every stream of the grid, written once."""
    out = []

    def add(kind, cfg, items):
        out.extend(write_pages(L, [(f"{kind} {a.dtype.name} n={a.size}", a) for a in items], cfg))

    per = lambda **kw: G.make_config(enable_8_bit=True, max_page_n=1 << 20, **kw)   # noqa: E731
    every = [numbers(dt, n, 11 * i + n) for i, dt in enumerate(TYPES) for n in SIZES]
    add("classic", per(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), every)
    add("consecutive1", per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), every)
    add("consecutive2", per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=2), every)
    add("consecutive7", per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7), [numbers(dt, 3000, 5) for dt in TYPES])
    add("lookback", per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK), [numbers(dt, n, 7 * i + n, period=365) for i, dt in enumerate(TYPES) for n in SIZES])
    add("conv1", per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=8, conv1=True),
        [numbers(dt, n, 3) for dt in TYPES if np.dtype(dt).itemsize <= 4 for n in (257, 3000, 70000)])
    add("int_mult+delta", per(mode=G.MODE_TRY_INT_MULT, mode_u64=10, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1),
        [(numbers(dt, n, 9) // 10 * 10 + 3).astype(dt) for dt in (np.uint32, np.int64) for n in (257, 3000, 70000)])
    add("float_mult+delta", per(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1),
        [(np.cumsum(np.random.default_rng(n).integers(-5, 7, n)) / 100.0).astype(dt) for dt in (np.float32, np.float64) for n in (257, 3000, 70000)])
    add("float_quant", per(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=8, delta=G.DELTA_NOOP),
        [np.random.default_rng(n).normal(size=n).astype(dt) for dt in (np.float32, np.float64) for n in (257, 3000, 70000)])
    add("dict50", per(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True),
        [np.random.default_rng(1).integers(0, 1 << 15, 50).astype(dt)[np.random.default_rng(n).integers(0, 50, n)] for dt in (np.int16, np.uint32, np.float32, np.int64, np.float64)
         for n in (257, 3000, 70000)])
    # level 12 asks for 4096 unoptimised bins at this size (wrapped/chunk_compressor.rs:362-371); 1000 equally likely values 65 apart stay a bin each:
    # merging two of them would cost six offset bits on 140 numbers to save one bin's ~35 bits of metadata
    sparse = (np.arange(1000, dtype=np.uint16) * 65 + 7)[np.random.default_rng(12).integers(0, 1000, 70000)]
    big = write_pages(L, [("level12 uint16 n=70000", sparse)], per(level=12, mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP))
    info = meta_info(L, big[0])
    assert info.n_bins[1] > 256, info.n_bins[1]   # beyond the walkers' tables: handed back
    out.extend(big)
    return out


class MetaInfo(C.Structure):
    _fields_ = [("mode_kind", C.c_uint32), ("mode_k", C.c_uint32), ("mode_base_latent", C.c_uint64), ("delta_kind", C.c_uint32), ("delta_order", C.c_uint32),
                ("window_n_log", C.c_uint32), ("state_n_log", C.c_uint32), ("secondary_uses_delta", C.c_uint32), ("n_vars_parsed", C.c_uint32),
                ("present", C.c_uint32 * 3), ("ans_size_log", C.c_uint32 * 3), ("n_bins", C.c_uint32 * 3), ("meta_bytes", C.c_uint64)]


def meta_info(L, s):
    info = MetaInfo()
    buf = (C.c_uint8 * len(s.meta)).from_buffer_copy(s.meta)
    assert L.pco_gfx_chunk_meta_info(buf, C.c_size_t(len(s.meta)), C.c_ubyte(G.DTYPE_BYTE[s.nums.dtype.name]), C.c_uint8(4), C.byref(info)) == 0
    return info


def test_the_grid_streams_are_what_they_are_called(L, grid):
    """The configs are explicit, and the writer may still refuse one (a delta that does not pay): the kinds the routes differ by must be there."""
    kinds = {}
    for s in grid:
        i = meta_info(L, s)
        kinds.setdefault(s.label.split()[0], set()).add((i.mode_kind, i.delta_kind, i.delta_order if i.delta_kind == 1 else 0))
    assert kinds["classic"] == {(0, 0, 0)} and (0, 1, 1) in kinds["consecutive1"] and (0, 1, 2) in kinds["consecutive2"] and (0, 1, 7) in kinds["consecutive7"]
    assert any(k[1] == 2 for k in kinds["lookback"]) and any(k[1] == 3 for k in kinds["conv1"]) and any(k[0] == 4 for k in kinds["dict50"])
    assert any(k[0] == 1 for k in kinds["int_mult+delta"]) and any(k[0] == 2 for k in kinds["float_mult+delta"]) and any(k[0] == 3 for k in kinds["float_quant"])


@pytest.mark.parametrize("form", ["sync", "async"])
def test_every_range_of_the_grid_is_the_input_slice(L, grid, form):
    jobs = [(s, None, f, c) for s in grid for (f, c) in ranges_of(s.n)]
    code, rec, got = run_ranges(L, jobs, form)
    assert code == G.PcoSuccess, L.pco_gfx_last_error()
    check_ok(jobs, rec, got, form)


def test_lookback_with_a_delta_d_secondary_variable(L):
    """No encoder writes it; the format allows it.  Synchronous: decoded (a second history buffer, taken when asked for); asynchronous: UNSUPPORTED,
    the one exception pco_gfx_decompress_pages has too."""
    x = (np.cumsum(np.random.default_rng(3).integers(-5, 7, 3000)) / 4.0).astype(np.float32)
    meta, pages = O.test_encode(x, pages=[x.size], mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25, delta=O.TE_DELTA_LOOKBACK, window_n_log=8, state_n_log=1,
                                secondary_uses_delta=True, lookback_seed=5)
    s = Stream("lookback+secondary float32", x, meta, pages[0])
    info = meta_info(L, s)
    assert info.delta_kind == 2 and info.secondary_uses_delta == 1 and info.present[2] == 1
    jobs = [(s, None, f, c) for f, c in ranges_of(s.n)]
    code, rec, got = run_ranges(L, jobs, "sync")
    assert code == G.PcoSuccess
    check_ok(jobs, rec, got)
    code, rec, got = run_ranges(L, jobs, "async")
    for j, (_, _, f, c) in enumerate(jobs):
        assert rec["status"][j] == (G.ST_UNSUPPORTED if c else G.ST_OK) and rec["n_out"][j] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# laziness, deterministically
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_page_damaged_behind_the_range_decodes_and_one_damaged_inside_does_not(L):
    rng = np.random.default_rng(21)
    cases = [(U.synth("c2", 70000), dict(mode=1, delta=2, delta_order=1)),
             ((rng.integers(1000, 10000, 40000) / 100.0), dict(mode=2, mode_f64=0.01, delta=1)),
             (rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32), dict(mode=1, delta=1))]
    for nums, kw in cases:
        s = write_pages(L, [(str(kw), nums)], G.make_config(max_page_n=1 << 20, **kw))[0]
        n = s.n; n_b = (n + 255) // 256
        good = []; bad = []
        for cut in sorted({3, 9, len(s.page) // 7, len(s.page) // 3, len(s.page) // 2, (len(s.page) * 9) // 10, len(s.page) - 1}):
            page = s.page[:cut]
            ok_nums, err, in_meta = O.wrapped_page_prefix(s.meta, page, nums.dtype, n)
            w = 0 if in_meta else ok_nums.size
            assert err == G.ST_INSUFFICIENT_DATA and w % 256 == 0 and w < n
            if w >= 256:   # ranges whose last batch ends inside the intact prefix
                good += [(s, page, 0, 1), (s, page, w - 256, 256), (s, page, max(0, w - 700), min(w, 700)), (s, page, w - 1, 1)]
            wb = w // 256   # the first batch that cannot be finished
            bad += [(s, page, w, 1), (s, page, 0, min(n, w + 1)), (s, page, min(n - 1, w + 300), 1), (s, page, n - 1, 1)]
            assert all((f + c + 255) // 256 > wb for _, _, f, c in bad[-4:]) and wb < n_b
        assert len(good) >= 8
        code, rec, got = run_ranges(L, good, "sync")
        assert code == G.PcoSuccess, (kw, rec["status"])
        for j, (_, page, f, c) in enumerate(good):
            assert rec["status"][j] == 0 and rec["n_out"][j] == c and rec["consumed"][j] == 0 and U.bits_equal(got[j], nums[f: f + c]), (kw, f, c)
        code, rec, got = run_ranges(L, bad, "sync")   # (run_ranges checks the canaries around every dst)
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INSUFFICIENT_DATA
        assert (rec["status"] == G.ST_INSUFFICIENT_DATA).all() and (rec["n_out"] == 0).all(), (kw, rec["status"])
        code, rec, got = run_ranges(L, good + bad, "async")
        assert (rec["status"][: len(good)] == 0).all() and (rec["status"][len(good):] == G.ST_INSUFFICIENT_DATA).all() and (rec["n_out"][len(good):] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# one big mixed call
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_big_mixed_call_reports_its_bad_task_alone(L):
    rng = np.random.default_rng(77)
    per = lambda **kw: G.make_config(enable_8_bit=True, **kw)   # noqa: E731
    kinds = [(per(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP), 0), (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1), 0),
             (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=2), 0), (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=7), 0),
             (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK), 365), (per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONV1, delta_order=8, conv1=True), 0),
             (per(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True), -50)]
    streams = []
    for k, (cfg, period) in enumerate(kinds):
        items = []
        for i, dt in enumerate(TYPES):
            if k == 5 and np.dtype(dt).itemsize > 4 or k == 6 and np.dtype(dt).itemsize == 1:
                continue
            n = int(rng.integers(300, 5001))
            a = numbers(dt, n, 100 * k + i, period=max(period, 0))
            if period < 0:
                a = a[:50][rng.integers(0, 50, n)]
            items.append((f"kind{k} {np.dtype(dt).name} n={n}", a))
        streams += write_pages(L, items, cfg)
    fm = [(np.cumsum(rng.integers(-5, 7, n)) / 100.0).astype(dt) for dt, n in ((np.float32, 4100), (np.float64, 999))]
    streams += write_pages(L, [(f"float_mult {a.dtype.name}", a) for a in fm], per(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))
    streams += write_pages(L, [(f"float_quant {a.dtype.name}", (a * 7).astype(a.dtype)) for a in fm], per(mode=G.MODE_TRY_FLOAT_QUANT, mode_u64=8, delta=G.DELTA_NOOP))
    streams += write_pages(L, [("int_mult int64", (numbers(np.int64, 2500, 4) * 10 + 3))], per(mode=G.MODE_TRY_INT_MULT, mode_u64=10, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))
    assert {s.nums.dtype.itemsize for s in streams} == {1, 2, 4, 8}
    jobs = []
    for j in range(1100):   # (above the 1024 chunks from which a whole-page call takes the publishing walker; several tasks per page)
        s = streams[j % len(streams)]
        f = int(rng.integers(0, s.n)); c = int(rng.integers(0, min(s.n - f, 600) + 1))
        jobs.append((s, None, f, c))
    victim = next(s for s in streams if s.label.startswith("kind1 uint32"))
    bad_at = 550
    jobs[bad_at] = (victim, victim.page[: len(victim.page) // 3], victim.n - 10, 10)
    for form, env in (("sync", None), ("async", None), ("sync", "0.0001")):   # 100 KB of scratch per pass: the scratch route runs in passes
        if env is not None:
            os.environ["PCO_GFX_WORKSPACE_GB"] = env
        try:
            code, rec, got = run_ranges(L, jobs, form)
        finally:
            os.environ.pop("PCO_GFX_WORKSPACE_GB", None)
        if form == "sync":
            assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INSUFFICIENT_DATA
        assert rec["status"][bad_at] == G.ST_INSUFFICIENT_DATA and rec["n_out"][bad_at] == 0
        keep = [j for j in range(len(jobs)) if j != bad_at]
        check_ok([jobs[j] for j in keep], rec[keep], [got[j] for j in keep], (form, env))


# ---------------------------------------------------------------------------------------------------------------------------------------
# work follows the prefix
# ---------------------------------------------------------------------------------------------------------------------------------------
def profiled_ms(L, fn):
    import torch
    fn()   # untimed
    torch.cuda.synchronize()
    L.pco_gfx_profile_begin()
    fn()
    torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 16); ms = (C.c_float * 4096)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 4096)
    return float(sum(ms[:nk]))


def test_the_work_of_a_range_follows_its_prefix(L):
    """One u64 delta-1 page of 2^20 numbers: rows [0, 1024) are 1/1024 of the tANS chain.  DESIGN section 8 puts a one-page chain at 20-37 ns per
    latent, so the whole page is at least 20 ms and the prefix tens of microseconds plus launch floors: 1/8 leaves about two orders of magnitude
    for a busy device.  The yardstick is the unchanged whole-page entry point."""
    import torch
    n = 1 << 20
    s = write_pages(L, [("c2 2^20", U.synth("c2", n))], G.make_config(mode=1, delta=2, delta_order=1, max_page_n=n))[0]
    pool = Pool([s.meta, s.page])
    whole = torch.zeros(n * 8 + 64, dtype=torch.uint8, device="cuda")
    part = torch.zeros(1024 * 8 + 64, dtype=torch.uint8, device="cuda")

    def pages(k):
        t = (G.PageTask * k)(*[G.PageTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), whole.data_ptr(), n, 2, 4)] * k)
        res = (G.TaskResult * k)()
        G.check(L.pco_gfx_decompress_pages(k, t, res, None, None))

    def ranges(k):
        t = (G.PageRangeTask * k)(*[G.PageRangeTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), part.data_ptr(), n, 0, 1024, 2, 4)] * k)
        res = (G.TaskResult * k)()
        G.check(L.pco_gfx_decompress_page_ranges(k, t, res, None, None))
        assert all(r.n_out == 1024 and r.consumed == 0 for r in res)

    ms_whole = profiled_ms(L, lambda: pages(1))
    ms_range = profiled_ms(L, lambda: ranges(1))
    assert U.bits_equal(part[: 1024 * 8].cpu().numpy().view(np.uint64), s.nums[:1024]) and U.bits_equal(whole[: n * 8].cpu().numpy().view(np.uint64), s.nums)
    print(f"whole page {ms_whole:.3f} ms, rows [0, 1024) {ms_range:.3f} ms")
    # the scratch of 2048 prefixes against that of 2048 whole decodes of the same pages (every task writes the same numbers to the same place)
    torch.cuda.synchronize(); L.pco_gfx_release_workspace()
    ranges(2048); ws_range = L.pco_gfx_workspace_bytes()
    torch.cuda.synchronize(); L.pco_gfx_release_workspace()
    pages(2048); ws_whole = L.pco_gfx_workspace_bytes()
    torch.cuda.synchronize(); L.pco_gfx_release_workspace()
    print(f"workspace: 2048 prefixes {ws_range} B, 2048 whole pages {ws_whole} B")
    assert ms_range <= ms_whole / 8, (ms_range, ms_whole)
    assert 0 < ws_range < ws_whole, (ws_range, ws_whole)


# ---------------------------------------------------------------------------------------------------------------------------------------
# paged.decompress_rows
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_decompress_rows(L):
    import torch
    a = (np.cumsum(np.random.default_rng(1).integers(-5, 7, 4500)) / 4.0).astype(np.float32)
    b = U.synth("c4", 10000)
    cfg = ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(1), paging_spec=PagingSpec.equal_pages_up_to(4096))
    cc = paged.compress_chunks([torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()], cfg, page_sizes=[[1000, 3000, 500], None])
    d = cc.directory
    assert [p.n for p in d if p.chunk == 0 and p.piece] == [1000, 3000, 500] and len([p for p in d if p.chunk == 1 and p.piece]) == 3
    names = ["float32", "int64"]
    for rows in ([(10, 20), (0, 10000)], [(990, 1010), (3333, 3334)], [(999, 4001), None], [(1000, 1001), (6666, 6667)], [(0, 4500), (5, 5)], [None, (3000, 7000)],
                 [(77, 77), None], [None, None]):
        got = paged.decompress_rows(cc.blob, d, names, rows)
        want = [x[r[0]: r[1]] for x, r in zip((a, b), rows) if r is not None]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert U.bits_equal(g.cpu().numpy(), w), rows
    with pytest.raises(ValueError):
        paged.decompress_rows(cc.blob, d, names, [(5, 4), None])
    with pytest.raises(ValueError):
        paged.decompress_rows(cc.blob, d, names, [None, (0, 10001)])
    # an interval inside one page of the float32 chunk: kernels of ONE number width, and the int64 chunk's pages produce nothing
    L.pco_gfx_profile_begin()
    got = paged.decompress_rows(cc.blob, d, names, [(1500, 1600), None])
    kernels = U.profile_names(L)
    assert kernels and all(k.endswith("<u32>") for k in kernels), kernels
    assert paged.map_rows_to_pages([1000, 3000, 500], 1500, 1600) == [(1, 500, 100, 0)]
    assert U.bits_equal(got[0].cpu().numpy(), a[1500:1600])
