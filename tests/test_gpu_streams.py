"""-m gpu: the stream, thread and workspace contracts of the batched ABI (include/pco_gfx.h section 3 and its thread-safety paragraph).

Every other GPU test makes one call at a time from one host thread with stream == NULL, where all ordering is trivial.  Here every batched entry
point runs on a non-blocking caller stream (torch.cuda.Stream()), in its synchronous and its asynchronous form, behind pending work on that stream,
next to pending work on another stream of the same thread (one workspace: pco_host.h WorkspaceUse), and from four host threads at once.  Nothing is
compared with another output of the library: encodes with the oracle's bytes, decodes with the input array, compactions with numpy.

Sensitivity is by construction, never by removing an ordering: a buffer that is read too early holds OTHER VALID numbers (or another valid chunk),
so a wrongly ordered kernel produces clean but wrong bytes; snapshots are copies queued on the stream with no host synchronisation in between, so a
join that is missing lets the copy overtake the last kernel; host task arrays are overwritten with valid decoy tasks as soon as a call returns.

Batches cycle through a few distinct arrays (gpu_util.tile), so the oracle's bytes are computed once per distinct array and still compared for
100 % of the chunks; every chunk is also round-tripped against its input.

What the asynchronous forms do on the host (test_input_side_stream_order reads stream.query() right after each call returns, behind ~30 ms of
queued device work; information for callers, not an assertion):
  pco_gfx_compress_chunks(results = NULL)     returned BEFORE the stream drained
  pco_gfx_decompress_chunks(results = NULL)   returned BEFORE the stream drained
  pco_gfx_decompress_pages(results = NULL)    returned BEFORE the stream drained
  pco_gfx_compact_chunks(total = NULL)        returned BEFORE the stream drained
(MI355X, ROCm 7, explicit specs, pinned task arrays: the uploads of the library's own pageable staging vectors did not wait for the stream.  An Auto
spec resolves modes and deltas on the host and synchronises inside the call; pco_gfx_compress_wrapped_chunks has a synchronous form only.)
"""
import ctypes as C
import gc
import os
import sys
import threading
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import gpu_util as U  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402

pytestmark = pytest.mark.gpu

N14 = 1 << 14
C2 = dict(mode=1, delta=2, delta_order=1)
LOOKBACK = dict(mode=1, delta=3)


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    lib.pco_gfx_compact_chunks.argtypes = U.COMPACT_ARGTYPES
    return lib


def gen(kind, n, seed):
    rng = np.random.default_rng(1000 + seed)
    if kind == "f32": return rng.standard_normal(n).astype(np.float32)
    if kind == "lomax": return (rng.pareto(0.5, n) * 10).clip(0, 2e9).astype(np.int32)
    return U.synth(kind, n, seed=1000 + seed)   # c1 u32 incompressible, c2 u64 ramp, c3 f64 decimals, c4 i64 periodic


def distinct(kinds, n, per_kind, seed0=0):
    return [gen(k, n, seed0 + s) for s in range(per_kind) for k in kinds]


def handle(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def oracle_chunks(arrays_distinct, kw):
    ocfg = O.make_config(**kw)
    return [U.oracle_chunk(a, ocfg) for a in arrays_distinct]


def encode(L, st, cfg, stream, sync=True, tasks=None):
    """pco_gfx_compress_chunks on `stream`; d_results is always passed.  Returns the host results (synchronous form) or None."""
    t = tasks if tasks is not None else st.enc_tasks()
    res = np.zeros(st.k, U.RES_DT) if sync else None
    code = L.pco_gfx_compress_chunks(st.k, U.ptr(t), C.byref(cfg), U.ptr(res) if sync else None, st.d_res.data_ptr(), handle(stream))
    G.check(code)
    return res


def decode(L, st, sizes, stream, sync=True, tasks=None, out=None, slots=None, d_dres=None):
    t = tasks if tasks is not None else st.dec_tasks(sizes, slots=slots, out=out)
    res = np.zeros(st.k, U.RES_DT) if sync else None
    code = L.pco_gfx_decompress_chunks(st.k, U.ptr(t), U.ptr(res) if sync else None, (d_dres if d_dres is not None else st.d_dres).data_ptr(), handle(stream))
    G.check(code)
    return res


def assert_chunks(got, want_distinct, what):
    bad = [i for i, g in enumerate(got) if g != want_distinct[i % len(want_distinct)]]
    assert not bad, f"{what}: {len(bad)} of {len(got)} chunks differ from the oracle's bytes, first {bad[:5]}"


def assert_ok(res, what):
    assert (res["status"] == 0).all(), f"{what}: statuses {np.unique(res['status'])}, first bad task {int(np.flatnonzero(res['status'])[0])}"


def compact_reference(chunks, dst_offset, dst_len, canary):
    body = b"".join(chunks)
    want = np.full(dst_len, canary, np.uint8)
    want[dst_offset: dst_offset + len(body)] = np.frombuffer(body, np.uint8)
    offs = dst_offset + np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    return want, offs


# ---------------------------------------------------------------------------------------------------------------------------------------
# A.1  every batched entry point on a non-NULL stream, synchronous form
# ---------------------------------------------------------------------------------------------------------------------------------------
def _conv1_reference(a, ch):
    p = G.chunk_meta_conv1(ch[4:], G.DTYPE_BYTE[a.dtype.name])
    assert p is not None, "the smooth series must fit a Conv1 config"
    f = O.test_encode(a, mode=G.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=p[0], bias=p[1], weights=p[2], level=8)
    return U.chunk_of_file(f, len(ch))


def _dict_reference(a, ch):
    import test_gpu_dict_encode as TD
    d = TD.dict_of_chunk(ch, a.dtype)
    assert d is not None, "a pool of 200 values must encode as a Dict chunk"
    np.testing.assert_array_equal(d, TD.model_dict(a))
    return TD.patched_oracle_chunk(a, d, ch, delta=O.TE_DELTA_CONSECUTIVE, order=1, level=8)


def _spec_inputs(spec):
    """(product config, oracle config keywords or None, distinct arrays, reference(a, chunk) for the specs the oracle only encodes given the product's parameters)"""
    if spec == "consecutive": return G.make_config(**C2), C2, distinct(("c2", "f32", "lomax", "c3"), N14, 4), None
    if spec == "auto": return G.make_config(), dict(), distinct(("c2", "f32", "lomax", "c3"), N14, 2), None
    if spec == "lookback": return G.make_config(**LOOKBACK), LOOKBACK, distinct(("c4", "c2", "f32", "lomax"), N14, 2), None
    if spec == "conv1":
        import test_gpu_conv1_encode as TC
        return TC.cfg(3), None, [TC.smooth(N14, dt, seed=s) for s in range(2) for dt in ("int32", "float32", "uint32")], _conv1_reference
    rng = np.random.default_rng(77)
    arrays = []
    for dt in ("uint64", "float32", "uint64", "float32"):
        pool = rng.integers(0, 1 << 30, 200).astype(dt)
        arrays.append(pool[rng.integers(0, 200, N14)])
    return G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1, dict=True), None, arrays, _dict_reference


@pytest.mark.parametrize("spec", ["consecutive", "auto", "lookback", "conv1", "dict"])
def test_chunk_entry_points_on_a_caller_stream(L, spec):
    """pco_gfx_compress_chunks, pco_gfx_compact_chunks and pco_gfx_decompress_chunks, synchronous form, on a non-blocking stream: 256 chunks of 2^14
    numbers of mixed types per spec.  Bytes == the oracle's for every chunk, compacted stream == numpy's concatenation, arrays == the inputs."""
    import torch
    cfg, okw, dist, ref = _spec_inputs(spec)
    st = U.Staged(L, U.tile(dist, 256))
    s = torch.cuda.Stream()
    res = encode(L, st, cfg, s)
    assert_ok(res, spec)
    got = st.slot_bytes(res["n_out"])
    want = oracle_chunks(dist, okw) if ref is None else [ref(a, got[i]) for i, a in enumerate(dist)]
    assert_chunks(got, want, f"compress_chunks[{spec}] on a stream")
    d_res = st.results()
    assert np.array_equal(d_res["n_out"], res["n_out"]) and (d_res["status"] == 0).all()   # (d_results is filled in synchronous calls too)
    # compaction on the same stream, at an odd offset
    cap = int(res["n_out"].sum()) + 4099
    dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda"); d_offs = torch.zeros(st.k + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = C.c_uint64(0); tasks = st.enc_tasks()
    G.check(L.pco_gfx_compact_chunks(st.k, U.ptr(tasks), st.d_res.data_ptr(), dst.data_ptr(), cap, 4099, d_offs.data_ptr(), C.byref(total), handle(s)))
    want_dst, want_offs = compact_reference([want[i % len(want)] for i in range(st.k)], 4099, cap + 64, 0xA5)
    assert total.value == cap and np.array_equal(d_offs.cpu().numpy().view(np.uint64), want_offs)
    assert np.array_equal(dst.cpu().numpy(), want_dst), f"compact_chunks[{spec}] on a stream"
    dres = decode(L, st, res["n_out"], s)
    assert_ok(dres, spec)
    assert np.array_equal(dres["n_out"], st.n) and np.array_equal(dres["consumed"], res["n_out"])
    assert st.outputs_equal() == []


@pytest.mark.parametrize("spec", ["consecutive", "auto", "lookback"])
def test_wrapped_entry_points_on_a_caller_stream(L, spec):
    """pco_gfx_compress_wrapped_chunks and pco_gfx_decompress_pages, synchronous form, on a non-blocking stream: 96 chunks of 2^14 numbers in pages of
    3000.  Every ChunkMeta and page == the oracle's wrapped::ChunkCompressor's, every page decodes to its part of the input."""
    import torch
    kw = {"consecutive": C2, "auto": dict(), "lookback": LOOKBACK}[spec]
    dist = distinct(("c2", "f32", "lomax", "c3") if spec != "lookback" else ("c4", "c2", "f32", "lomax"), N14, 2)
    cfg = G.make_config(max_page_n=3000, **kw)
    st = U.Staged(L, U.tile(dist, 96))
    s = torch.cuda.Stream()
    wcaps = np.array([L.pco_gfx_wrapped_chunk_cap(a.size, int(d), C.addressof(cfg)) for a, d in zip(st.arrays, st.dtb)], np.int64)
    woff = np.concatenate([[0], np.cumsum(wcaps)]).astype(np.int64)
    wdst = torch.zeros(int(woff[-1]) + 64, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
    assert wdst.data_ptr() % 16 == 0 and (wcaps % 16 == 0).all()
    tasks = st.enc_tasks(); tasks["dst"] = wdst.data_ptr() + woff[:-1].astype(np.uint64); tasks["dst_cap"] = wcaps
    n_pages = [L.pco_gfx_wrapped_n_pages(a.size, 3000) for a in st.arrays]
    infos = (G.PageInfo * (sum(n_pages) + st.k))()
    G.check(L.pco_gfx_compress_wrapped_chunks(st.k, U.ptr(tasks), C.addressof(cfg), infos, handle(s)))
    host = wdst.cpu().numpy()
    want = [O.wrapped_compress(a, O.make_config(max_page_n=3000, **kw)) for a in dist]
    ptasks = []; at = 0
    for i, a in enumerate(st.arrays):
        m = infos[at]; assert m.status == 0 and m.offset == 0
        base = int(woff[i]); meta = host[base: base + m.len].tobytes(); pages = []; start = 0
        for p in range(n_pages[i]):
            e = infos[at + 1 + p]; assert e.status == 0
            pages.append(host[base + e.offset: base + e.offset + e.len].tobytes())
            ptasks.append((wdst.data_ptr() + base, m.len, wdst.data_ptr() + base + e.offset, e.len, st.out.data_ptr() + int(st.in_off[i]) + start * a.dtype.itemsize, e.n, int(st.dtb[i]), 4))
            start += e.n
        w = want[i % len(want)]
        assert (meta, pages) == (w[0], w[1]), f"wrapped chunk {i} [{spec}] differs from the oracle's"
        at += 1 + n_pages[i]
    pt = np.array(ptasks, U.PAGE_DT); pres = np.zeros(len(pt), U.RES_DT)
    G.check(L.pco_gfx_decompress_pages(len(pt), U.ptr(pt), U.ptr(pres), None, handle(s)))
    assert_ok(pres, spec)
    assert np.array_equal(pres["n_out"], pt["page_n"]) and np.array_equal(pres["consumed"], pt["page_len"])
    assert st.outputs_equal() == []


@pytest.mark.parametrize("widths", ["one", "two"])
def test_trail_decode_on_a_caller_stream(L, widths):
    """>= 1024 chunks of one width in one decode call on a caller stream: the publishing walker, the ordinary walker on the second side stream and the
    expanders under them on the first (launch_decode's fork / join events), once for a single width and once with 1024 chunks each of two widths
    (PCO_GFX_DEC_TRAIL=2 is read when the library is loaded, which other test modules of the same process have done long before)."""
    import torch
    dist = distinct(("c2",) if widths == "one" else ("c2", "f32"), N14, 4)
    st = U.Staged(L, U.tile(dist, 1024 if widths == "one" else 2048))
    s = torch.cuda.Stream()
    res = encode(L, st, G.make_config(**C2), s)
    assert_ok(res, widths)
    assert_chunks(st.slot_bytes(res["n_out"]), oracle_chunks(dist, C2), "compress_chunks before the trail decode")
    marked0 = L.pco_gfx_trail_marked()
    for form in ("sync", "async"):
        st.out.zero_(); torch.cuda.synchronize()
        dres = decode(L, st, res["n_out"], s, sync=form == "sync")
        s.synchronize()
        dres = st.results(st.d_dres)
        assert_ok(dres, f"{widths}/{form}")
        assert np.array_equal(dres["n_out"], st.n) and st.outputs_equal() == [], f"{widths}/{form}"
    marked, gave = L.pco_gfx_trail_marked() - marked0, L.pco_gfx_trail_givebacks()
    assert marked > 0, "no chunk went to the expanders under the walk"
    assert gave <= L.pco_gfx_trail_marked()


# ---------------------------------------------------------------------------------------------------------------------------------------
# A.2  stream order on the input side
# ---------------------------------------------------------------------------------------------------------------------------------------
ASYNC_SEEN = {}   # entry point -> stream.query() right after the asynchronous call returned (True: the stream had already drained)


def _note(name, drained):
    ASYNC_SEEN.setdefault(name, []).append(bool(drained))
    print(f"[async form] {name}: returned {'AFTER the stream drained (the call blocked on the host)' if drained else 'BEFORE the stream drained'}")


@pytest.mark.parametrize("form", ["sync", "async"])
def test_input_side_stream_order_encode(L, form):
    """~30 ms of copies on the stream, then (still on it) the real numbers copied over a source buffer that held OTHER valid numbers, then
    pco_gfx_compress_chunks / pco_gfx_compress_wrapped_chunks on that stream with pinned task arrays.  A kernel ordered anywhere but behind the
    stream encodes the stale numbers: clean bytes, not the oracle's."""
    import torch
    dist = distinct(("c2", "f32", "lomax", "c3"), N14, 2)
    stale = distinct(("c2", "f32", "lomax", "c3"), N14, 2, seed0=50)
    st = U.Staged(L, U.tile(dist, 256)); old = U.Staged(L, U.tile(stale, 256))
    assert np.array_equal(st.in_off, old.in_off)
    want = oracle_chunks(dist, C2)
    s = torch.cuda.Stream()
    work = old.src.clone(); torch.cuda.synchronize()
    tasks = U.pinned(st.enc_tasks(src=work))
    U.device_delay(s)
    with torch.cuda.stream(s):
        work.copy_(st.src, non_blocking=True)
    res = encode(L, st, G.make_config(**C2), s, sync=form == "sync", tasks=tasks)
    if form == "async":
        _note("pco_gfx_compress_chunks", s.query())
    s.synchronize()
    res = st.results()
    assert_ok(res, form)
    assert_chunks(st.slot_bytes(res["n_out"]), want, f"compress_chunks ({form}) behind a pending copy of its input")
    if form == "sync":   # the wrapped encoder has a synchronous form only
        cfg = G.make_config(max_page_n=5000, **C2)
        work.copy_(old.src); torch.cuda.synchronize()
        wcaps = np.array([L.pco_gfx_wrapped_chunk_cap(a.size, int(d), C.addressof(cfg)) for a, d in zip(st.arrays, st.dtb)], np.int64)
        woff = np.concatenate([[0], np.cumsum(wcaps)]).astype(np.int64)
        wdst = torch.zeros(int(woff[-1]) + 64, dtype=torch.uint8, device="cuda"); torch.cuda.synchronize()
        t = st.enc_tasks(src=work); t["dst"] = wdst.data_ptr() + woff[:-1].astype(np.uint64); t["dst_cap"] = wcaps
        t = U.pinned(t)
        n_pages = [L.pco_gfx_wrapped_n_pages(a.size, 5000) for a in st.arrays]
        infos = (G.PageInfo * (sum(n_pages) + st.k))()
        U.device_delay(s)
        with torch.cuda.stream(s):
            work.copy_(st.src, non_blocking=True)
        G.check(L.pco_gfx_compress_wrapped_chunks(st.k, U.ptr(t), C.addressof(cfg), infos, handle(s)))
        host = wdst.cpu().numpy(); wwant = [O.wrapped_compress(a, O.make_config(max_page_n=5000, **C2)) for a in dist]; at = 0
        for i in range(st.k):
            base = int(woff[i]); meta = host[base: base + infos[at].len].tobytes()
            pages = [host[base + infos[at + 1 + p].offset: base + infos[at + 1 + p].offset + infos[at + 1 + p].len].tobytes() for p in range(n_pages[i])]
            assert (meta, pages) == wwant[i % len(wwant)][:2], f"wrapped chunk {i} behind a pending copy of its input"
            at += 1 + n_pages[i]


@pytest.mark.parametrize("form", ["sync", "async"])
def test_input_side_stream_order_decode(L, form):
    """The same for the decoders: the slots hold valid OLDER chunks (the oracle's bytes of other arrays); the real chunks (the oracle's too) are
    copied in on the stream behind the delay; pco_gfx_decompress_chunks and pco_gfx_decompress_pages then run on that stream."""
    import torch
    dist = distinct(("c2", "f32", "lomax", "c3"), N14, 2)
    stale = distinct(("c2", "f32", "lomax", "c3"), N14, 2, seed0=50)
    st = U.Staged(L, U.tile(dist, 256))
    new = oracle_chunks(dist, C2); old = oracle_chunks(stale, C2)
    real = st.put_chunks([new[i % len(new)] for i in range(st.k)])
    older = st.put_chunks([old[i % len(old)] for i in range(st.k)])
    sizes = np.array([len(new[i % len(new)]) for i in range(st.k)], np.uint64)
    s = torch.cuda.Stream()
    st.slots.copy_(older); torch.cuda.synchronize()
    tasks = U.pinned(st.dec_tasks(sizes))
    U.device_delay(s)
    with torch.cuda.stream(s):
        st.slots.copy_(real, non_blocking=True)
    decode(L, st, sizes, s, sync=form == "sync", tasks=tasks)
    if form == "async":
        _note("pco_gfx_decompress_chunks", s.query())
    s.synchronize()
    dres = st.results(st.d_dres)
    assert_ok(dres, form)
    assert st.outputs_equal() == [], f"decompress_chunks ({form}) behind a pending copy of its input"
    # pages: the wrapped pieces of the same arrays, each chunk's ChunkMeta and single page side by side in its slot
    wnew = [O.wrapped_compress(a, O.make_config(**C2)) for a in dist]; wold = [O.wrapped_compress(a, O.make_config(**C2)) for a in stale]
    assert all(len(w[1]) == 1 for w in wnew + wold)
    M = (max(len(w[0]) for w in wnew + wold) + 31) // 16 * 16   # every slot: the ChunkMeta at 0, the page at M
    lay = lambda w: w[0] + bytes(M - len(w[0])) + w[1][0]   # noqa: E731
    real = st.put_chunks([lay(wnew[i % len(wnew)]) for i in range(st.k)])
    older = st.put_chunks([lay(wold[i % len(wold)]) for i in range(st.k)])
    pt = np.zeros(st.k, U.PAGE_DT)
    pt["meta"] = st.slots.data_ptr() + st.slot_off[:-1].astype(np.uint64); pt["meta_len"] = [len(wnew[i % len(wnew)][0]) for i in range(st.k)]
    pt["page"] = pt["meta"] + np.uint64(M)
    pt["page_len"] = [len(wnew[i % len(wnew)][1][0]) for i in range(st.k)]
    pt["dst"] = st.out.data_ptr() + st.in_off[:-1].astype(np.uint64); pt["page_n"] = st.n; pt["dtype"] = st.dtb; pt["format_major"] = 4
    pt = U.pinned(pt)
    st.slots.copy_(older); st.out.zero_(); st.d_dres.zero_(); torch.cuda.synchronize()
    pres = np.zeros(st.k, U.RES_DT)
    U.device_delay(s)
    with torch.cuda.stream(s):
        st.slots.copy_(real, non_blocking=True)
    G.check(L.pco_gfx_decompress_pages(st.k, U.ptr(pt), U.ptr(pres) if form == "sync" else None, st.d_dres.data_ptr(), handle(s)))
    if form == "async":
        _note("pco_gfx_decompress_pages", s.query())
    s.synchronize()
    assert_ok(st.results(st.d_dres), form)
    assert st.outputs_equal() == [], f"decompress_pages ({form}) behind a pending copy of its input"


@pytest.mark.parametrize("form", ["sync", "async"])
def test_input_side_stream_order_compact(L, form):
    """pco_gfx_compact_chunks behind a pending copy of BOTH its inputs: the slots (older valid chunks first) and d_results (their sizes first)."""
    import torch
    dist = distinct(("c2", "f32", "lomax", "c3"), N14, 2)
    stale = distinct(("c2", "f32", "lomax", "c3"), N14, 2, seed0=50)
    st = U.Staged(L, U.tile(dist, 256))
    new = oracle_chunks(dist, C2); old = oracle_chunks(stale, C2)
    chunks = [new[i % len(new)] for i in range(st.k)]
    real = st.put_chunks(chunks); older = st.put_chunks([old[i % len(old)] for i in range(st.k)])

    def results_of(cs):
        r = np.zeros(st.k, U.RES_DT); r["n_out"] = [len(cs[i % len(cs)]) for i in range(st.k)]
        return torch.from_numpy(r.view(np.uint8).copy()).cuda()
    real_res, old_res = results_of(new), results_of(old)
    cap = sum(len(c) for c in chunks) + 7
    dst = torch.full((cap + 64,), 0x5A, dtype=torch.uint8, device="cuda"); d_offs = torch.zeros(st.k + 1, dtype=torch.int64, device="cuda")
    st.slots.copy_(older); st.d_res.copy_(old_res); torch.cuda.synchronize()
    tasks = U.pinned(st.enc_tasks())
    s = torch.cuda.Stream()
    U.device_delay(s)
    with torch.cuda.stream(s):
        st.slots.copy_(real, non_blocking=True); st.d_res.copy_(real_res, non_blocking=True)
    total = C.c_uint64(0)
    G.check(L.pco_gfx_compact_chunks(st.k, U.ptr(tasks), st.d_res.data_ptr(), dst.data_ptr(), cap, 7, d_offs.data_ptr(), C.byref(total) if form == "sync" else None, handle(s)))
    if form == "async":
        _note("pco_gfx_compact_chunks", s.query())
    s.synchronize()
    want_dst, want_offs = compact_reference(chunks, 7, cap + 64, 0x5A)
    assert np.array_equal(d_offs.cpu().numpy().view(np.uint64), want_offs) and (form == "async" or total.value == cap)
    assert np.array_equal(dst.cpu().numpy(), want_dst), f"compact_chunks ({form}) behind a pending copy of its inputs"


# ---------------------------------------------------------------------------------------------------------------------------------------
# A.3  stream order on the output side: encode -> compact -> snapshot -> decode -> snapshot with no host synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------------
def pipeline(L, st, decoy, cfg, sizes, s, dst_offset=0, slack=0):
    """The asynchronous pipeline on stream `s`; every host task array is overwritten with the decoy's (valid buffers, other numbers) as soon as its
    call has returned, then dropped.  Returns the device tensors to look at after ONE synchronisation."""
    import torch
    cap = int(sizes.sum()) + dst_offset + slack
    payload = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    d_offs = torch.zeros(st.k + 1, dtype=torch.int64, device="cuda")
    snap_payload = torch.zeros_like(payload); snap_offs = torch.zeros_like(d_offs); snap_out = torch.zeros_like(st.out); snap_res = torch.zeros_like(st.d_res)
    st.slots.zero_(); st.out.zero_(); st.d_res.fill_(0xFF); st.d_dres.fill_(0xFF)
    torch.cuda.synchronize()
    t = st.enc_tasks()
    encode(L, st, cfg, s, sync=False, tasks=t)
    t[:] = decoy.enc_tasks(); del t
    t = st.enc_tasks()
    G.check(L.pco_gfx_compact_chunks(st.k, U.ptr(t), st.d_res.data_ptr(), payload.data_ptr(), cap, dst_offset, d_offs.data_ptr(), None, handle(s)))
    t[:] = decoy.enc_tasks(); del t
    with torch.cuda.stream(s):
        snap_payload.copy_(payload, non_blocking=True); snap_offs.copy_(d_offs, non_blocking=True); snap_res.copy_(st.d_res, non_blocking=True)
    t = st.dec_tasks(sizes)
    decode(L, st, sizes, s, sync=False, tasks=t)
    t[:] = decoy.dec_tasks(decoy.sizes); del t
    gc.collect()
    with torch.cuda.stream(s):
        snap_out.copy_(st.out, non_blocking=True)
    s.synchronize()
    return snap_payload, snap_offs, snap_res, snap_out, cap


@pytest.mark.parametrize("spec", ["consecutive", "lookback"])
def test_output_side_stream_order_pipeline(L, spec):
    """encode(results = NULL) -> compact(total = NULL) -> device copies of the stream and the offsets -> decode(results = NULL) of the slots ->
    device copy of the outputs, all queued on one stream without a host synchronisation, the task arrays overwritten after each call.  The chunk
    sizes the decode tasks need come from the oracle (the same bytes a previous synchronous encode writes).  The SNAPSHOTS must hold the oracle's
    chunks back to back and the inputs: a last kernel that is not joined into the caller's stream is overtaken by the copy behind it."""
    import torch
    kw = {"consecutive": C2, "lookback": LOOKBACK}[spec]
    dist = distinct(("c2", "f32", "lomax", "c3") if spec == "consecutive" else ("c4", "c2", "lomax"), N14, 2)
    st = U.Staged(L, U.tile(dist, 512)); decoy = U.Staged(L, U.tile(distinct(("c2", "f32", "lomax", "c3") if spec == "consecutive" else ("c4", "c2", "lomax"), N14, 2, seed0=50), 512))
    cfg = G.make_config(**kw)
    want = oracle_chunks(dist, kw); chunks = [want[i % len(want)] for i in range(st.k)]
    sizes = np.array([len(c) for c in chunks], np.uint64)
    dres = encode(L, decoy, cfg, None); assert_ok(dres, "decoy"); decoy.sizes = dres["n_out"].copy()   # valid chunks in the decoy's slots
    s = torch.cuda.Stream()
    snap_payload, snap_offs, snap_res, snap_out, cap = pipeline(L, st, decoy, cfg, sizes, s)
    res = snap_res.cpu().numpy().view(U.RES_DT)[: st.k]
    assert_ok(res, "encode statuses in the snapshot")
    assert np.array_equal(res["n_out"], sizes)
    want_dst, want_offs = compact_reference(chunks, 0, cap + 64, 0xC3)
    assert np.array_equal(snap_offs.cpu().numpy().view(np.uint64), want_offs)
    assert np.array_equal(snap_payload.cpu().numpy(), want_dst), "the snapshot of the compacted stream is not the oracle's chunks back to back"
    assert_ok(st.results(st.d_dres), "decode statuses")
    assert st.outputs_equal(snap_out) == [], "the snapshot of the outputs is not the input"


# ---------------------------------------------------------------------------------------------------------------------------------------
# A.4  two streams, one thread, one workspace
# ---------------------------------------------------------------------------------------------------------------------------------------
def _host_calls_exact(L):
    """The host-buffer entry points (stream 0, plain hipMemcpy) right behind asynchronous calls of this thread on other streams."""
    a = gen("c2", 50000, 9); kw = C2
    f = O.simple_compress(a, O.make_config(**kw))
    assert U.bits_equal(U.gpu_simple_decompress(f, a.dtype, a.size), a), "pco_standalone_simple_decompress_into behind pending asynchronous calls"
    assert U.gpu_simple_compress(a, G.make_config(**kw)) == f, "pco_gfx_simple_compress_into_ex behind pending asynchronous calls"


def _encoded(L, dist, k, kw):
    """k chunks staged, encoded on the NULL stream and checked against the oracle: the input of an asynchronous decode"""
    st = U.Staged(L, U.tile(dist, k))
    res = encode(L, st, G.make_config(**kw), None)
    assert_ok(res, "staging")
    assert_chunks(st.slot_bytes(res["n_out"]), oracle_chunks(dist, kw), "staging encode")
    st.sizes = res["n_out"].copy()
    return st


def test_two_streams_decode_then_encode(L):
    """Stream A: an asynchronous decode of 1024 u64 chunks (the trail path: both side streams).  Stream B, at once: an asynchronous encode of 1200
    f32 chunks (another width, more tasks: the workspace must grow while A runs).  Then the host-buffer entry points on stream 0."""
    import torch
    a = _encoded(L, distinct(("c2",), N14, 4), 1024, C2)
    distb = distinct(("f32", "lomax"), N14, 2); b = U.Staged(L, U.tile(distb, 1200)); wantb = oracle_chunks(distb, C2)
    L.pco_gfx_release_workspace()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    decode(L, a, a.sizes, sa, sync=False)
    w1 = L.pco_gfx_workspace_bytes()
    encode(L, b, G.make_config(**C2), sb, sync=False)
    w2 = L.pco_gfx_workspace_bytes()
    _host_calls_exact(L)
    torch.cuda.synchronize()
    assert w2 > w1 > 0, (w1, w2)
    assert_ok(a.results(a.d_dres), "A"); assert a.outputs_equal() == []
    rb = b.results(); assert_ok(rb, "B")
    assert_chunks(b.slot_bytes(rb["n_out"]), wantb, "asynchronous encode on stream B behind a decode on stream A")


def test_two_streams_encode_then_decode(L):
    """Stream A: an asynchronous lookback encode of 384 i64 chunks.  Stream B, at once: an asynchronous decode of 1536 f32 / i32 chunks."""
    import torch
    dista = distinct(("c4",), N14, 4); a = U.Staged(L, U.tile(dista, 384)); wanta = oracle_chunks(dista, LOOKBACK)
    b = _encoded(L, distinct(("f32", "lomax"), N14, 2), 1536, C2)
    L.pco_gfx_release_workspace()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    encode(L, a, G.make_config(**LOOKBACK), sa, sync=False)
    w1 = L.pco_gfx_workspace_bytes()
    decode(L, b, b.sizes, sb, sync=False)
    w2 = L.pco_gfx_workspace_bytes()
    _host_calls_exact(L)
    torch.cuda.synchronize()
    assert w2 > w1 > 0, (w1, w2)
    ra = a.results(); assert_ok(ra, "A")
    assert_chunks(a.slot_bytes(ra["n_out"]), wanta, "asynchronous lookback encode on stream A with a decode queued on stream B")
    assert_ok(b.results(b.d_dres), "B"); assert b.outputs_equal() == []


def test_two_streams_a_b_a(L):
    """A -> B -> A: 1024 u64 chunks decoded on A, 2048 smaller f32 chunks on B (the same scratch buffers, which must grow), 1024 u64 chunks on A
    again into a second output area.  The stream differs from the previous call's every time, and the third call must wait for B's work too."""
    import torch
    a = _encoded(L, distinct(("c2",), N14, 4), 1024, C2)
    b = _encoded(L, distinct(("f32",), 1 << 12, 4), 2048, C2)
    L.pco_gfx_release_workspace()
    out2 = torch.zeros_like(a.out); d2 = torch.zeros_like(a.d_dres); torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    decode(L, a, a.sizes, sa, sync=False)
    w1 = L.pco_gfx_workspace_bytes()
    decode(L, b, b.sizes, sb, sync=False)
    w2 = L.pco_gfx_workspace_bytes()
    decode(L, a, a.sizes, sa, sync=False, out=out2, d_dres=d2)
    _host_calls_exact(L)
    torch.cuda.synchronize()
    assert w2 > w1 > 0, (w1, w2)
    assert_ok(a.results(a.d_dres), "A"); assert a.outputs_equal() == []
    assert_ok(b.results(b.d_dres), "B"); assert b.outputs_equal() == []
    assert_ok(a.results(d2), "A again"); assert a.outputs_equal(out2) == []


# ---------------------------------------------------------------------------------------------------------------------------------------
# A.5  release and counters while work is pending
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_release_and_counters_while_work_is_pending(L):
    import torch
    a = _encoded(L, distinct(("c2",), N14, 4), 1024, C2)
    diste = distinct(("c2", "f32", "lomax"), N14, 2); e = U.Staged(L, U.tile(diste, 192)); wante = oracle_chunks(diste, C2)
    s = torch.cuda.Stream()
    marked0, strict0 = L.pco_gfx_trail_marked(), L.pco_gfx_strict_histogram_fallbacks()
    decode(L, a, a.sizes, s, sync=False)
    held = L.pco_gfx_workspace_bytes()
    marked, gave = L.pco_gfx_trail_marked(), L.pco_gfx_trail_givebacks()   # (wait for the thread's last call)
    assert held > 0 and marked > marked0 and gave <= marked, (held, marked0, marked, gave)
    encode(L, e, G.make_config(strict_histogram=True, **C2), s, sync=False)
    strict = L.pco_gfx_strict_histogram_fallbacks()
    decode(L, a, a.sizes, s, sync=False)
    L.pco_gfx_release_workspace()   # right behind an asynchronous call: it must wait for that call before it frees what the kernels use
    assert L.pco_gfx_workspace_bytes() == 0
    s.synchronize()
    assert strict >= strict0
    assert L.pco_gfx_trail_marked() >= marked and L.pco_gfx_trail_givebacks() <= L.pco_gfx_trail_marked()   # (the totals survive the release)
    assert_ok(a.results(a.d_dres), "decode"); assert a.outputs_equal() == []
    re = e.results(); assert_ok(re, "strict encode")
    assert_chunks(e.slot_bytes(re["n_out"]), wante, "asynchronous strict-histogram encode")
    a.out.zero_(); torch.cuda.synchronize()
    dres = decode(L, a, a.sizes, s)   # the next call starts from an empty workspace
    assert_ok(dres, "after the release"); assert a.outputs_equal() == [] and L.pco_gfx_workspace_bytes() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# B.  host threads
# ---------------------------------------------------------------------------------------------------------------------------------------
def _run_threads(targets):
    """Start one thread per target behind a barrier; re-raise the first failure in the caller."""
    errors = []; barrier = threading.Barrier(len(targets))

    def wrap(fn):
        def run():
            try:
                barrier.wait(timeout=120)
                fn()
            except BaseException as e:   # noqa: BLE001
                errors.append(e); barrier.abort()
        return run
    ts = [threading.Thread(target=wrap(fn)) for fn in targets]
    for t in ts: t.start()
    for t in ts: t.join(timeout=600)
    assert not any(t.is_alive() for t in ts), "a worker thread did not finish"
    if errors:
        raise errors[0]


def test_four_threads_with_a_stream_and_a_workload_each(L):
    """u64 consecutive and f64 float-mult under the default ChunkConfig (both through the shared host pool of the Auto resolution, and through the
    wrapped batched calls as well), u32 incompressible (Classic, the select histogram) and i64 lookback, each on its own thread and stream, three
    batches of different sizes each so that the workspaces grow while the other threads run."""
    import torch
    plans = [("c2", dict(), True), ("c3", dict(), True), ("c1", dict(mode=1, delta=1), False), ("c4", LOOKBACK, False)]
    sizes = (40, 130, 70)
    work = []
    for kind, kw, wrapped in plans:   # the oracle's bytes on the main thread, before anything runs
        dist = distinct((kind,), N14, 4)
        work.append((kind, kw, wrapped, dist, oracle_chunks(dist, kw), [O.wrapped_compress(a, O.make_config(max_page_n=6000, **kw)) for a in dist] if wrapped else None))
    main_before = L.pco_gfx_workspace_bytes()
    fresh = {}; counters = {}

    def worker(kind, kw, wrapped, dist, want, wwant):
        def run():
            fresh[kind] = L.pco_gfx_workspace_bytes()
            s = torch.cuda.Stream(); cfg = G.make_config(**kw)
            for it, k in enumerate(sizes):
                st = U.Staged(L, U.tile(dist, k))
                res = encode(L, st, cfg, s)
                assert_ok(res, (kind, it))
                assert_chunks(st.slot_bytes(res["n_out"]), want, f"thread {kind}, batch {it}")
                dres = decode(L, st, res["n_out"], s)
                assert_ok(dres, (kind, it)); assert st.outputs_equal() == [], (kind, it)
                if wrapped:
                    wcfg = G.make_config(max_page_n=6000, **kw)
                    wcaps = np.array([L.pco_gfx_wrapped_chunk_cap(a.size, int(d), C.addressof(wcfg)) for a, d in zip(st.arrays, st.dtb)], np.int64)
                    woff = np.concatenate([[0], np.cumsum(wcaps)]).astype(np.int64)
                    wdst = torch.zeros(int(woff[-1]) + 64, dtype=torch.uint8, device="cuda"); st.out.zero_(); torch.cuda.synchronize()
                    t = st.enc_tasks(); t["dst"] = wdst.data_ptr() + woff[:-1].astype(np.uint64); t["dst_cap"] = wcaps
                    npg = L.pco_gfx_wrapped_n_pages(N14, 6000); infos = (G.PageInfo * (st.k * (1 + npg)))()
                    G.check(L.pco_gfx_compress_wrapped_chunks(st.k, U.ptr(t), C.addressof(wcfg), infos, handle(s)))
                    host = wdst.cpu().numpy(); pts = []
                    for i in range(st.k):
                        at = i * (1 + npg); base = int(woff[i]); m = infos[at]; start = 0
                        meta = host[base: base + m.len].tobytes(); pages = []
                        for p in range(npg):
                            e = infos[at + 1 + p]; pages.append(host[base + e.offset: base + e.offset + e.len].tobytes())
                            pts.append((wdst.data_ptr() + base, m.len, wdst.data_ptr() + base + e.offset, e.len, st.out.data_ptr() + int(st.in_off[i]) + start * 8, e.n, int(st.dtb[i]), 4))
                            start += e.n
                        assert (meta, pages) == wwant[i % len(wwant)][:2], f"thread {kind}, batch {it}, wrapped chunk {i}"
                    pt = np.array(pts, U.PAGE_DT); pres = np.zeros(len(pt), U.RES_DT)
                    G.check(L.pco_gfx_decompress_pages(len(pt), U.ptr(pt), U.ptr(pres), None, handle(s)))
                    assert_ok(pres, (kind, it, "pages")); assert st.outputs_equal() == [], (kind, it, "pages")
            counters[kind] = (L.pco_gfx_trail_marked(), L.pco_gfx_trail_givebacks(), L.pco_gfx_workspace_bytes())
            assert L.pco_gfx_last_status() == G.ST_OK
        return run
    _run_threads([worker(*w) for w in work])
    assert all(v == 0 for v in fresh.values()) and len(fresh) == 4, f"a fresh thread must report an empty workspace: {fresh}"
    assert L.pco_gfx_workspace_bytes() == main_before, f"the main thread's workspace changed; per thread (marked, givebacks, workspace bytes): {counters}"
    assert all(c[2] > 0 and c[1] <= c[0] for c in counters.values()), f"per thread (marked, givebacks, workspace bytes): {counters}"


def test_error_state_is_thread_local(L):
    """Thread X fails twice before the device (an invalid number type; TryDict without PCO_GFX_CFG_DICT) while thread Y has just succeeded: Y still
    reads OK and an empty message, X reads its own failure."""
    st = U.Staged(L, [gen("c2", 3000, 1)])
    y_done, x_done = threading.Event(), threading.Event()
    seen = {}

    def thread_y():
        res = encode(L, st, G.make_config(**C2), None); assert_ok(res, "Y")
        y_done.set()
        assert x_done.wait(120)
        seen["y"] = (L.pco_gfx_last_status(), L.pco_gfx_last_error())

    def thread_x():
        assert y_done.wait(120)
        a = st.arrays[0]; dst = np.zeros(1 << 16, np.uint8); n = C.c_size_t(0); cfg = G.make_config(**C2)
        code = L.pco_gfx_simple_compress_into_ex(a.ctypes.data_as(C.c_void_p), a.size, 99, C.byref(cfg), 0, dst.ctypes.data_as(C.c_void_p), dst.size, C.byref(n))
        seen["x1"] = (code, L.pco_gfx_last_status(), L.pco_gfx_last_error())
        cfg = G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP)
        res = np.zeros(1, U.RES_DT); tasks = st.enc_tasks()
        code = L.pco_gfx_compress_chunks(1, U.ptr(tasks), C.byref(cfg), U.ptr(res), None, None)
        seen["x2"] = (code, L.pco_gfx_last_status(), L.pco_gfx_last_error())
        x_done.set()
    _run_threads([thread_y, thread_x])
    assert seen["y"] == (G.ST_OK, b""), seen
    assert seen["x1"][:2] == (G.PcoInvalidType, G.ST_INVALID_ARGUMENT) and b"dtype" in seen["x1"][2], seen
    assert seen["x2"][:2] == (G.PcoCompressionError, G.ST_UNSUPPORTED) and b"Dict" in seen["x2"][2], seen


def test_workspaces_of_threads_that_exit_are_given_back(L):
    """Eight short-lived threads one after another, each growing a workspace of W bytes (several hundred MB: 192 lookback chunks of 2^16 i64) with
    one call.  After the last has gone the device's free memory may be lower than before the first by LESS THAN ONE W: eight leaked workspaces
    would be 8 W, one W covers allocator and runtime noise.  Every buffer is allocated before the first reading; the threads allocate nothing
    through torch."""
    import torch
    dist = distinct(("c4",), 1 << 16, 2); want = oracle_chunks(dist, LOOKBACK)
    st = U.Staged(L, U.tile(dist, 192)); cfg = G.make_config(**LOOKBACK)
    streams = [torch.cuda.Stream() for _ in range(8)]
    torch.cuda.synchronize()
    seen = []

    def one(s):
        def run():
            w0 = L.pco_gfx_workspace_bytes()
            res = encode(L, st, cfg, s)
            seen.append((w0, L.pco_gfx_workspace_bytes(), res, threading.get_native_id()))
        return run
    free0 = torch.cuda.mem_get_info()[0]
    for s in streams:
        t = threading.Thread(target=one(s)); t.start(); t.join(timeout=300)
        assert not t.is_alive() and len(seen) == streams.index(s) + 1
        # (join returns when the Python part of the thread is over; the thread-exit destructor that gives the workspace back runs a moment later,
        #  as the native thread goes: wait for that, two seconds at the most)
        for _ in range(200):
            if not os.path.exists(f"/proc/self/task/{seen[-1][3]}"): break
            time.sleep(0.01)
    free1 = torch.cuda.mem_get_info()[0]
    W = min(x[1] for x in seen)
    assert all(x[0] == 0 for x in seen) and W > (256 << 20), [(x[0], x[1]) for x in seen]
    for x in seen:
        assert_ok(x[2], "thread")
    assert_chunks(st.slot_bytes(seen[-1][2]["n_out"]), want, "the last thread's encode")
    assert free0 - free1 < W, f"free memory fell by {free0 - free1} bytes over eight exited threads; one workspace is {W} bytes"
