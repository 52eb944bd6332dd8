"""-m gpu: pco_gfx_compact_chunks (include/pco_gfx.h section 3; stream_kernels.hip) against numpy.

The reference is b"".join(slot_i[:n_out_i] for the chunks whose status is OK) placed at dst_offset, d_offsets = the exclusive running sum from
dst_offset.  The destination is filled with a canary byte first and compared WHOLE, the 64 bytes beyond dst_cap included, so a byte written outside
[dst_offset, end) shows as well as a byte missing inside.  The slots come from real pco_gfx_compress_chunks calls (spot-checked against the oracle);
chunk counts walk the scan's 1024-entry rounds and their carry, chunk sizes the copy's byte-wise head and tail, its 16-byte quads and its 64 KiB
slices, destinations every alignment."""
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

pytestmark = pytest.mark.gpu

CANARY = 0xA5
NOOP = dict(mode=1, delta=1)
C2 = dict(mode=1, delta=2, delta_order=1)
OFFSETS = (0, 1, 7, 15, 16, 4099)
ALL_ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    lib.pco_gfx_compact_chunks.argtypes = U.COMPACT_ARGTYPES
    return lib


def handle(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


class Encoded:
    """A batch encoded by one synchronous pco_gfx_compress_chunks call: the slots and d_results stay on the device, the host keeps each chunk's
    bytes and status.  `small_caps`: indices of tasks that declare a dst_cap of 48 bytes, too small for the encoder (their slots keep their size)."""

    def __init__(self, L, arrays, kw, small_caps=()):
        self.L = L
        self.st = st = U.Staged(L, arrays)
        caps = st.caps.copy()
        if len(small_caps):
            caps[np.asarray(list(small_caps), np.int64)] = 48
        self.tasks = st.enc_tasks(caps=caps)
        cfg = G.make_config(**kw)
        self.res = res = np.zeros(st.k, U.RES_DT)
        code = L.pco_gfx_compress_chunks(st.k, U.ptr(self.tasks), C.byref(cfg), U.ptr(res), st.d_res.data_ptr(), None) if st.k else G.PcoSuccess
        self.failed = sorted(int(i) for i in small_caps)
        if self.failed:   # the call reports its first failed task; every other task is encoded
            assert code == G.PcoCompressionError and L.pco_gfx_last_status() != G.ST_OK
        else:
            G.check(code)
        ok = np.ones(st.k, bool); ok[self.failed] = False
        assert (res["status"][ok] == 0).all() and (res["status"][~ok] != 0).all(), np.unique(res["status"])
        sizes = np.where(ok, res["n_out"], 0)
        self.chunks = st.slot_bytes(sizes)   # b"" for a failed chunk
        self.body = sum(len(c) for c in self.chunks)

    def spot_check(self, kw, idx):
        for i in idx:
            assert self.chunks[i] == U.oracle_chunk(self.st.arrays[i], O.make_config(**kw)), f"chunk {i} is not the oracle's"

    def compact(self, dst_offset, dst_cap=None, misalign=0, sync=True, stream=None, d_results="own", d_offsets="own", d_dst="own"):
        """One pco_gfx_compact_chunks call into a fresh canary-filled destination of dst_cap bytes (+ 64 beyond).  Returns (code, total or None,
        host copy of the whole destination, host d_offsets)."""
        import torch
        k = self.st.k
        cap = self.body + dst_offset if dst_cap is None else dst_cap
        raw = torch.full((cap + 64 + 16,), CANARY, dtype=torch.uint8, device="cuda")
        assert raw.data_ptr() % 16 == 0
        dst = raw[misalign: misalign + cap + 64]
        offs = torch.full((k + 1,), 0x1111111111111111, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        total = C.c_uint64(0xDEAD)
        code = self.L.pco_gfx_compact_chunks(k, U.ptr(self.tasks), self.st.d_res.data_ptr() if d_results == "own" else d_results,
                                             dst.data_ptr() if d_dst == "own" else d_dst, cap, dst_offset, offs.data_ptr() if d_offsets == "own" else d_offsets,
                                             C.byref(total) if sync else None, handle(stream))
        torch.cuda.synchronize()
        return code, (total.value if sync else None), dst.cpu().numpy(), offs.cpu().numpy().view(np.uint64)

    def reference(self, dst_offset, dst_cap=None):
        cap = self.body + dst_offset if dst_cap is None else dst_cap
        want = np.full(cap + 64, CANARY, np.uint8)
        want[dst_offset: dst_offset + self.body] = np.frombuffer(b"".join(self.chunks), np.uint8)
        offs = np.uint64(dst_offset) + np.concatenate([[0], np.cumsum([len(c) for c in self.chunks])]).astype(np.uint64)
        return want, offs

    def check(self, dst_offset, misalign=0, sync=True, stream=None, slack=0):
        cap = self.body + dst_offset + slack
        code, total, dst, offs = self.compact(dst_offset, cap, misalign, sync, stream)
        want, want_offs = self.reference(dst_offset, cap)
        what = f"n = {self.st.k}, dst_offset = {dst_offset}, d_dst at +{misalign}, {'sync' if sync else 'async'}"
        assert code == G.PcoSuccess, what
        assert np.array_equal(offs, want_offs), what
        assert total is None or total == self.body + dst_offset, what
        if not np.array_equal(dst, want):
            bad = np.flatnonzero(dst != want)
            raise AssertionError(f"{what}: {bad.size} bytes differ, first at {int(bad[0])} (stream is [{dst_offset}, {dst_offset + self.body}), dst_cap = {cap})")


def pool_u32(n_total, seed=1):
    return np.random.default_rng(seed).integers(0, 1 << 32, n_total, dtype=np.uint64).astype(np.uint32)


def cut(pool, sizes):
    at = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert at[-1] <= pool.size
    return [pool[at[i]: at[i + 1]] for i in range(len(sizes))]


def layout(kind, n):
    """n arrays: 'tiny' = 1..3 numbers (u32 / u64 / i16 alternating, a few bytes of payload each), '5k' = incompressible u32 chunks of 1150..1350 numbers"""
    if kind == "tiny":
        rng = np.random.default_rng(5)
        return [rng.integers(0, 1 << 15, 1 + i % 3).astype((np.uint32, np.uint64, np.int16)[(i // 3) % 3]) for i in range(n)]
    sizes = [1150 + (i * 37) % 201 for i in range(n)]
    return cut(pool_u32(sum(sizes) if n else 1), sizes)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. shapes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tiny", "5k"])
@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2500])
def test_chunk_counts_across_the_scan_rounds(L, n, kind):
    """The scan takes 1024 chunks per round and carries the running sum into the next: counts on both sides of one round and 2.4 rounds, with chunks
    of a few bytes and of about 5 KB, at every destination offset and with an unaligned d_dst, in both forms."""
    e = Encoded(L, layout(kind, n), NOOP)
    e.spot_check(NOOP, range(0, n, max(n // 8, 1)))   # (oracle bytes for 9 chunks at most, i.e. every chunk up to n = 9 and 9 / n of them beyond: the slots are the encoder's, tested elsewhere; the compaction is compared in full)
    if kind == "tiny" and n:
        print(f"[tiny] chunk sizes {sorted(set(len(c) for c in e.chunks))}")
        assert min(len(c) for c in e.chunks) < 32   # (a standalone chunk of one small number: a few bytes behind its ChunkMeta)
    for j, off in enumerate(OFFSETS):
        e.check(off, misalign=0, sync=True)
        e.check(off, misalign=3, sync=j % 2 == 0, slack=j)


def test_chunks_at_and_beyond_the_64_kib_slices(L):
    """Incompressible u32 (and u8) chunks whose encoded sizes straddle 65 536 and 131 072 bytes -- the element counts are FOUND by encoding a range of
    counts -- so that a chunk ends exactly at (u8), just before and just after a slice boundary of the copy kernel."""
    pool = pool_u32(40000, seed=3)
    bytes8 = np.random.default_rng(4).integers(0, 256, 140000).astype(np.uint8)   # (u32 sizes move in steps of 4 and miss the boundary itself; u8 sizes hit it)
    kw = dict(enable_8_bit=True, **NOOP)
    picked = []
    for target in (65536, 131072):
        for src, step in ((pool, 4), (bytes8, 1)):
            cand = list(range(target // step - 160 // step, target // step + 24 // step))
            probe = Encoded(L, [src[:c] for c in cand], kw)
            sizes = np.array([len(c) for c in probe.chunks])
            assert sizes.min() <= target < sizes.max(), (target, sizes.min(), sizes.max())
            at = int(np.flatnonzero(sizes <= target)[-1])
            picked += [src[:c] for c in cand[at - 1: at + 3]]
            print(f"[slices] target {target}, {src.dtype}: counts {cand[at - 1: at + 3]} encode to {sizes[at - 1:at + 3].tolist()} bytes")
            assert sizes[at] <= target < sizes[at + 1] and (step != 1 or sizes[at] == target)
    arrays = picked + layout("5k", 5) + picked[::-1]
    e = Encoded(L, arrays, kw)
    e.spot_check(NOOP, range(len(arrays)))
    for off in OFFSETS:
        for mis in (0, 3):
            e.check(off, misalign=mis, sync=(off + mis) % 2 == 0)


def test_one_long_chunk_among_small_ones(L):
    """One incompressible 2^18-number u64 chunk (2 MB, 32 slices) among 300 small chunks: max_cap sets the slices of EVERY chunk, so most blocks of the
    small ones return early, and the long chunk is spread over many blocks whose heads and tails meet inside it."""
    big = np.random.default_rng(9).integers(0, 1 << 63, 1 << 18, dtype=np.uint64)
    small = layout("tiny", 150) + layout("5k", 150)
    arrays = small[:200] + [big] + small[200:]
    e = Encoded(L, arrays, NOOP)
    assert len(e.chunks[200]) > 31 << 16   # (more than 31 slices of the copy kernel)
    e.spot_check(NOOP, [0, 199, 200, 201, 300])
    for off in OFFSETS:
        for mis in (0, 3):
            e.check(off, misalign=mis, sync=(off + mis) % 2 == 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 10. failed chunks contribute nothing
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last", "round"])
def test_failed_chunks_contribute_nothing(L, where):
    """Tasks whose dst_cap is too small for the encoder fail honestly (status INVALID_ARGUMENT in d_results); the compaction skips them: the later
    chunks close the gap, d_offsets[i] == d_offsets[i + 1] for a failed chunk, the stream is the join of the chunks that are OK."""
    n = 2200 if where == "round" else 40
    failed = {"first": [0], "middle": [17, 18, 30], "last": [n - 1], "round": list(range(1024, 2048)) + [5, 2199]}[where]
    e = Encoded(L, layout("5k", n), NOOP, small_caps=failed)
    assert all(e.chunks[i] == b"" for i in failed) and e.body == sum(len(c) for i, c in enumerate(e.chunks) if i not in failed) > 0
    for off in (0, 7, 4099):
        for sync in (True, False):
            code, total, dst, offs = e.compact(off, sync=sync, misalign=3 if sync else 0)
            want, want_offs = e.reference(off)
            assert code == G.PcoSuccess and np.array_equal(offs, want_offs) and (total is None or total == off + e.body)
            assert all(offs[i] == offs[i + 1] for i in failed)
            assert np.array_equal(dst, want), (where, off, sync)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 11. overflow
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_offset", [0, 4099])
def test_overflow_in_both_forms(L, dst_offset):
    """The comparison is on the END offset (dst_offset + the chunks' bytes) against dst_cap: end == dst_cap succeeds, dst_cap one byte less fails, in the
    synchronous form with PCO_GFX_INVALID_ARGUMENT and *total = d_offsets[n_tasks] = ~0 (the header's wording: the value stored is d_offsets[n_tasks],
    which reads ~0 when the destination is too small), in the asynchronous form with d_offsets[n_tasks] == ~0 alone.  Nothing is copied either way."""
    e = Encoded(L, layout("5k", 1030), NOOP)
    end = dst_offset + e.body
    e.check(dst_offset, sync=True); e.check(dst_offset, sync=False)   # end == dst_cap exactly
    for cap in (end - 1, dst_offset, max(dst_offset - 1, 0), e.body - 1 if dst_offset else end // 2):
        for sync in (True, False):
            code, total, dst, offs = e.compact(dst_offset, dst_cap=cap, sync=sync)
            assert int(offs[-1]) == ALL_ONES, (cap, sync)
            assert (dst == CANARY).all(), f"dst_cap = {cap} < end = {end}: bytes were copied"
            if sync:
                assert code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT and total == ALL_ONES
            else:
                assert code == G.PcoSuccess
    if dst_offset:   # the body alone would fit dst_cap; the END offset does not: an overflow
        code, total, dst, offs = e.compact(dst_offset, dst_cap=e.body + 1, sync=True)
        assert code == G.PcoCompressionError and total == ALL_ONES and (dst == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 12. on a caller stream, asynchronously, behind an asynchronous encode
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dst_offset,slack", [(1025, 0, 0), (700, 15, 0), (1500, 4099, 9)])
def test_asynchronous_compaction_behind_an_asynchronous_encode(L, n, dst_offset, slack):
    """test_gpu_streams' pipeline with the compaction's own parameters varied: encode(results = NULL), compact(total = NULL) and device copies of the
    stream and the offsets on one non-blocking stream, one synchronisation at the end, against the oracle's chunks back to back."""
    import torch
    import test_gpu_streams as S
    dist = S.distinct(("c2", "f32", "lomax"), 3000, 3)
    st = U.Staged(L, U.tile(dist, n)); decoy = U.Staged(L, U.tile(S.distinct(("c2", "f32", "lomax"), 3000, 3, seed0=50), n))
    cfg = G.make_config(**C2)
    want = S.oracle_chunks(dist, C2); chunks = [want[i % len(want)] for i in range(n)]
    sizes = np.array([len(c) for c in chunks], np.uint64)
    dres = S.encode(L, decoy, cfg, None); S.assert_ok(dres, "decoy"); decoy.sizes = dres["n_out"].copy()
    s = torch.cuda.Stream()
    snap_payload, snap_offs, snap_res, snap_out, cap = S.pipeline(L, st, decoy, cfg, sizes, s, dst_offset=dst_offset, slack=slack)
    res = snap_res.cpu().numpy().view(U.RES_DT)[:n]
    S.assert_ok(res, "encode"); assert np.array_equal(res["n_out"], sizes)
    want_dst, want_offs = S.compact_reference(chunks, dst_offset, cap + 64, 0xC3)
    assert np.array_equal(snap_offs.cpu().numpy().view(np.uint64), want_offs)
    assert np.array_equal(snap_payload.cpu().numpy(), want_dst)
    assert st.outputs_equal(snap_out) == []


def test_argument_errors(L):
    import torch
    e = Encoded(L, layout("5k", 3), NOOP)
    for kw in (dict(d_results=None), dict(d_offsets=None), dict(d_dst=None)):
        for sync in (True, False):
            code, total, dst, offs = e.compact(0, sync=sync, stream=torch.cuda.Stream(), **kw)
            assert code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT, kw
            assert (dst == CANARY).all() and (offs == 0x1111111111111111).all(), kw
    code, total, dst, offs = e.compact(0, dst_cap=0, d_dst=None)   # (a NULL destination of capacity 0 is only too small)
    assert code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT and int(offs[-1]) == ALL_ONES


def test_framed_stream_is_the_oracles_multi_chunk_file(L):
    """Chunks compacted on a caller stream behind the header's room, framed with pco_gfx_write_standalone_header / _footer: the oracle's file of the same
    chunks (PagingSpec::Exact cuts one chunk per entry), and pco_standalone_simple_decompress_into reads it back."""
    import torch
    sizes = [5000, 1, 70000, 257, 30000, 4096]
    nums = U.synth("c2", sum(sizes), seed=31)
    want = O.simple_compress_exact(nums, O.make_config(**C2), sizes)
    e = Encoded(L, cut(nums, sizes), C2)
    hdr = np.zeros(32, np.uint8)
    h = L.pco_gfx_write_standalone_header(hdr.ctypes.data_as(C.c_void_p), 32, nums.size, 0)
    assert h == U.standalone_header_len(nums.size)
    s = torch.cuda.Stream()
    code, total, dst, offs = e.compact(h, dst_cap=h + e.body + 1, sync=True, stream=s)
    assert code == G.PcoSuccess and total == h + e.body
    assert (dst[:h] == CANARY).all() and dst[total] == CANARY
    file = dst[: total + 1].copy(); file[:h] = hdr[:h]
    assert L.pco_gfx_write_standalone_footer(file[total:].ctypes.data_as(C.c_void_p), 1) == 1
    assert file.tobytes() == want
    assert U.bits_equal(U.gpu_simple_decompress(file.tobytes(), nums.dtype, nums.size), nums)
