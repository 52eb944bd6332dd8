"""-m gpu: the batched wrapped WRITER (include/pco_gfx.h section 4c): pco_gfx_compress_wrapped_chunks_ex (PagingSpec::Exact per chunk, host and
device piece directory, synchronous and asynchronous form, pass-cutting) and pco_gfx_compact_wrapped_chunks (stream_wrapped.hip).

References: the oracle's wrapped::ChunkCompressor bytes (oracle_lib.wrapped_compress(..., exact_pages=...)); for the two specs the oracle does
not encode on its own (Conv1, Dict) the product's one-chunk host-buffer path pco_chunk_compressor_new_exact; numpy for the compacted image
(built from the HOST infos and the slots' bytes); the inputs for every round trip.  Figures the module prints: see its last test.

Measured on an MI355X: the module adds about 10 s to the -m gpu suite (39 tests in 9.4 s)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import gpu_util as U  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from test_gpu_wrapped_batched import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE, CANARY = 64, 0xEE, 0xA5
ALL_ONES = (1 << 64) - 1
INFO_DT = np.dtype([("offset", "<u8"), ("len", "<u8"), ("n", "<u8"), ("status", "<u4"), ("aux", "<u4")])
C2 = dict(mode=1, delta=2, delta_order=1)


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def handle(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def equal_pages(n, max_page_n):
    """chunk_config.rs:145-161"""
    k = -(-n // max_page_n)
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


class Call:
    """`arrays` staged for one pco_gfx_compress_wrapped_chunks_ex call: page_lists[i] is None (EqualPagesUpTo) or the chunk's exact page sizes.
    Every dst slot is followed by GUARD bytes of GUARD_BYTE; slots start zeroed."""

    def __init__(self, L, arrays, cfg, page_lists=None, src=None):
        import torch
        self.L, self.cfg = L, cfg
        self.arrays = [np.ascontiguousarray(a) for a in arrays]
        self.k = k = len(self.arrays)
        self.page_lists = page_lists = list(page_lists) if page_lists is not None else [None] * k
        self.dtb = [G.DTYPE_BYTE[a.dtype.name] for a in self.arrays]
        self.keep = [(C.c_uint64 * len(p))(*p) if p is not None else None for p in page_lists]
        self.caps = [L.pco_gfx_wrapped_chunk_cap_exact(kp, len(p), d, C.addressof(cfg)) if p is not None else L.pco_gfx_wrapped_chunk_cap(a.size, d, C.addressof(cfg))
                     for a, d, p, kp in zip(self.arrays, self.dtb, page_lists, self.keep)]
        assert all(c > 0 and c % 16 == 0 for c in self.caps)
        self.pages = [list(p) if p is not None else equal_pages(a.size, int(cfg.max_page_n) or 1 << 18) for a, p in zip(self.arrays, page_lists)]
        self.n_pieces = sum(1 + len(p) for p in self.pages)
        self.piece_first = np.concatenate([[0], np.cumsum([1 + len(p) for p in self.pages])]).astype(np.int64)
        nb = [(a.nbytes + 15) // 16 * 16 for a in self.arrays]
        self.in_off = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        self.host_in = np.zeros(int(self.in_off[-1]) + 64, np.uint8)
        for a, o in zip(self.arrays, self.in_off):
            self.host_in[o: o + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.slot_off = np.concatenate([[0], np.cumsum([c + GUARD for c in self.caps])]).astype(np.int64)
        host_slots = np.zeros(int(self.slot_off[-1]) + 64, np.uint8)
        for o, c in zip(self.slot_off[:-1], self.caps):
            host_slots[o + c: o + c + GUARD] = GUARD_BYTE
        self.src = src if src is not None else torch.from_numpy(self.host_in).cuda()
        self.slots = torch.from_numpy(host_slots).cuda()
        self.out = torch.zeros(self.host_in.size, dtype=torch.uint8, device="cuda")
        self.d_infos = torch.zeros(max(self.n_pieces, 1) * INFO_DT.itemsize, dtype=torch.uint8, device="cuda")
        assert self.slots.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        self.infos = np.zeros(self.n_pieces, INFO_DT)
        self.tasks = self.make_tasks()

    def make_tasks(self, override=None):
        t = (G.WrappedTask * max(self.k, 1))()
        for i in range(self.k):
            p = self.page_lists[i]
            t[i] = G.WrappedTask(self.src.data_ptr() + int(self.in_off[i]), self.arrays[i].size, self.slots.data_ptr() + int(self.slot_off[i]), self.caps[i], self.dtb[i],
                                 len(p) if p is not None else 0, C.cast(self.keep[i], C.c_void_p) if p is not None else None)
        for i, kw in (override or {}).items():
            for f, v in kw.items():
                setattr(t[i], f, v)
        return t

    def encode(self, sync=True, stream=None, d_infos=True, tasks=None):
        return self.L.pco_gfx_compress_wrapped_chunks_ex(self.k, tasks if tasks is not None else self.tasks, C.addressof(self.cfg), U.ptr(self.infos) if sync else None,
                                                         self.d_infos.data_ptr() if d_infos else None, handle(stream))

    def device_infos(self):
        return self.d_infos.cpu().numpy()[: self.n_pieces * INFO_DT.itemsize].view(INFO_DT).copy()

    def pieces(self, infos=None):
        """[(meta bytes, [page bytes], [page n])] per chunk, read from the slots through `infos`; also checks the guards and the entries' shape"""
        infos = self.infos if infos is None else infos
        host = self.slots.cpu().numpy(); out = []
        for i in range(self.k):
            base = int(self.slot_off[i]); e = infos[self.piece_first[i]: self.piece_first[i + 1]]
            assert (e["status"] == 0).all(), (i, e["status"])
            assert e["offset"][0] == 0 and e["n"][0] == 0 and (e["offset"] % 16 == 0).all() and (e["offset"] + e["len"] <= self.caps[i]).all()
            assert (host[base + self.caps[i]: base + self.caps[i] + GUARD] == GUARD_BYTE).all(), f"guard bytes behind dst {i} were written"
            b = [host[base + int(o): base + int(o) + int(n)].tobytes() for o, n in zip(e["offset"], e["len"])]
            out.append((b[0], b[1:], [int(x) for x in e["n"][1:]]))
        return out

    def untouched(self):
        host = self.slots.cpu().numpy()
        return all((host[o: o + c] == 0).all() and (host[o + c: o + c + GUARD] == GUARD_BYTE).all() for o, c in zip(self.slot_off[:-1], self.caps))

    def page_tasks(self, infos=None, base_of=None):
        """PcoGfxPageTask records decoding every page from the slots (or from wherever base_of(piece index) says its bytes start) into self.out"""
        infos = self.infos if infos is None else infos
        t = []
        for i, a in enumerate(self.arrays):
            k0 = int(self.piece_first[i]); m = infos[k0]; start = 0
            where = (lambda k: self.slots.data_ptr() + int(self.slot_off[i]) + int(infos[k]["offset"])) if base_of is None else base_of
            for p in range(len(self.pages[i])):
                e = infos[k0 + 1 + p]
                t.append((where(k0), int(m["len"]), where(k0 + 1 + p), int(e["len"]), self.out.data_ptr() + int(self.in_off[i]) + start * a.dtype.itemsize, int(e["n"]), self.dtb[i], 4))
                start += int(e["n"])
        return np.array(t, U.PAGE_DT)

    def decode_and_compare(self, infos=None, base_of=None, stream=None):
        import torch
        self.out.zero_(); torch.cuda.synchronize()
        pt = self.page_tasks(infos, base_of); res = np.zeros(len(pt), U.RES_DT)
        G.check(self.L.pco_gfx_decompress_pages(len(pt), U.ptr(pt), U.ptr(res), None, handle(stream)))
        assert (res["status"] == 0).all() and np.array_equal(res["n_out"], pt["page_n"]) and np.array_equal(res["consumed"], pt["page_len"])
        host = self.out.cpu().numpy()
        assert np.array_equal(host[: self.in_off[-1]], self.host_in[: self.in_off[-1]]), "decoded pages differ from the input"


def corner_lists(n, rng):
    """Exact page lists for a chunk of n >= 2000 numbers that hit the corners"""
    cut = np.sort(rng.choice(np.arange(1, n), size=9, replace=False))
    return [[n], [1, n - 1], [n - 1, 1], [255, 256, 257, n - 768], [2, 1, n - 3], [13] * (n // 13) + ([n % 13] if n % 13 else []),
            np.diff(np.concatenate([[0], cut, [n]])).tolist()]


def oracle_pieces(a, okw, pages, max_page_n=0):
    return O.wrapped_compress(a, O.make_config(max_page_n=max_page_n, **okw), max_pages=len(pages) + 1 if pages is not None else 4096, exact_pages=pages)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. parity under PagingSpec::Exact
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_pages_match_the_oracle_and_round_trip(L, case):
    """One call per spec: chunks of 4001 numbers (300 pages of 13 among them), one of 40 in pages of one number, under page lists that hit the
    corners, beside two EqualPagesUpTo chunks.  ChunkMeta and every page == the oracle's, d_infos == infos, guards intact, pages decode."""
    kw, gen = CASES[case]
    rng = np.random.default_rng(11)
    n = 4001
    lists = corner_lists(n, rng) + [[1] * 40] + [None, None]
    arrays = [gen(n, 200 + i) for i in range(len(lists) - 3)] + [gen(40, 300), gen(5000, 301), gen(1, 302)]
    cfg = G.make_config(max_page_n=700, enable_8_bit=True, **kw)
    c = Call(L, arrays, cfg, lists)
    G.check(c.encode())
    got = c.pieces()
    for a, pl, g in zip(c.arrays, lists, got):
        want = oracle_pieces(a, kw, pl, 700)
        assert g[2] == want[2] == (pl if pl is not None else equal_pages(a.size, 700))
        assert g[0] == want[0], f"{case}: ChunkMeta differs from the oracle's (pages {str(pl)[:40]})"
        assert g[1] == want[1], f"{case}: page bytes differ from the oracle's (pages {str(pl)[:40]})"
    d = c.device_infos()
    for f in INFO_DT.names:
        assert np.array_equal(d[f], c.infos[f]), f"d_infos.{f} differs from infos.{f}"
    c.decode_and_compare()


def host_handle_pieces(a, config_kw, pages):
    """the product's one-chunk host-buffer path (pco_chunk_compressor_new_exact), the second opinion"""
    import pcodec_amd as P
    cc = P.wrapped.FileCompressor().chunk_compressor(a, P.ChunkConfig(paging_spec=P.PagingSpec.exact_page_sizes(pages), **config_kw))
    return cc.write_meta(), [cc.write_page(i) for i in range(len(pages))], cc.n_per_page()


@pytest.mark.parametrize("spec", ["conv1", "dict"])
def test_exact_pages_under_conv1_and_dict(L, spec):
    """The two opt-in specs: every page list against the host-buffer handle's bytes (the oracle encodes neither on its own), and the round trip."""
    import pcodec_amd as P
    rng = np.random.default_rng(5)
    n = 4001
    if spec == "conv1":
        import test_gpu_conv1_encode as TC
        arrays = [TC.smooth(n, dt, seed=s) for s, dt in enumerate(("int32", "float32", "uint32", "int32", "float32", "uint32", "int32"))]
        cfg = G.make_config(mode=1, delta=G.DELTA_TRY_CONV1, delta_order=3, conv1=True)
        pk = dict(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_conv1(3), enable_conv1=True)
        lists = [pl for pl in corner_lists(n, rng) if min(pl) >= 3]   # (a page shorter than the order is an error: test_argument_errors)
    else:
        arrays = []
        for dt in ("uint64", "float32", "uint64", "float32", "int16", "uint64", "float32"):
            pool = rng.integers(0, 1 << 14, 200).astype(dt); arrays.append(pool[rng.integers(0, 200, n)])
        cfg = G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1, dict=True)
        pk = dict(mode_spec=P.ModeSpec.try_dict(), delta_spec=P.DeltaSpec.try_consecutive(1), enable_dict=True)
        lists = corner_lists(n, rng)
    arrays = arrays[: len(lists)]
    c = Call(L, arrays, cfg, lists)
    G.check(c.encode())
    for a, pl, g in zip(c.arrays, lists, c.pieces()):
        want = host_handle_pieces(a, pk, pl)
        assert g[2] == list(want[2]) == pl and g[0] == want[0] and g[1] == want[1], f"{spec}: differs from the host-buffer handle's bytes (pages {str(pl)[:40]})"
    meta = c.pieces()[0][0]
    assert (G.chunk_meta_conv1(meta, c.dtb[0]) if spec == "conv1" else G.chunk_meta_dict(meta, c.dtb[0])) is not None, "the spec was not taken"
    assert np.array_equal(c.device_infos(), c.infos)
    c.decode_and_compare()


def test_a_page_shorter_than_the_consecutive_order(L):
    """[2, 1, n - 3] under TryConsecutive(3): whatever the oracle does with it is right, and the host-buffer handle agrees."""
    import pcodec_amd as P
    kw = dict(mode=1, delta=2, delta_order=3)
    a = U.synth("c2", 3000, seed=9); pl = [2, 1, 2997]
    want = oracle_pieces(a, kw, pl)
    c = Call(L, [a], G.make_config(**kw), [pl])
    G.check(c.encode())
    g = c.pieces()[0]
    assert (g[0], g[1], g[2]) == (want[0], want[1], want[2])
    hh = host_handle_pieces(a, dict(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_consecutive(3)), pl)
    assert (g[0], g[1]) == (hh[0], hh[1])
    c.decode_and_compare()


def test_one_call_mixes_exact_and_equal_pages_of_several_dtypes(L):
    rng = np.random.default_rng(3)
    arrays = [U.synth("c2", 20001, seed=1), np.cumsum(rng.integers(-5, 6, 9000)).astype(np.int32), rng.normal(size=7000).astype(np.float32),
              np.cumsum(rng.integers(-5, 6, 3000)).astype(np.int16), U.synth("c2", 1, seed=2), rng.integers(0, 255, 2500).astype(np.uint8),
              U.synth("c4", 6000, seed=3)]
    lists = [None, [4000, 5000], None, [1] * 10 + [2990], [1], None, [17] * 352 + [16]]
    cfg = G.make_config(max_page_n=4096, enable_8_bit=True, **C2)
    c = Call(L, arrays, cfg, lists)
    G.check(c.encode())
    for a, pl, g in zip(c.arrays, lists, c.pieces()):
        assert g == oracle_pieces(a, C2, pl, 4096), (a.dtype, str(pl)[:40])
    assert np.array_equal(c.device_infos(), c.infos)
    c.decode_and_compare()


@pytest.mark.parametrize("case", ["c2", "auto_f32", "c4"])
def test_equal_pages_through_the_new_entry_point_equal_the_old_one(L, case):
    import test_gpu_wrapped_batched as WB
    kw, gen = CASES[case]
    arrays = [gen(n, 100 + i) for i, n in enumerate([1, 255, 256, 257, 5000, 4096 * 3, 20001])]
    cfg = G.make_config(max_page_n=700, enable_8_bit=True, **kw)
    old, (dsts, infos, n_pages) = WB.wrapped_batch(L, arrays, cfg)
    c = Call(L, arrays, cfg)
    G.check(c.encode())
    assert c.pieces() == old
    for k in range(c.n_pieces):
        assert tuple(c.infos[k]) == (infos[k].offset, infos[k].len, infos[k].n, infos[k].status, infos[k].aux)
    c.decode_and_compare()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. argument errors: PCO_GFX_INVALID_ARGUMENT, and nothing is written
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(L):
    a = U.synth("c2", 3000); b = U.synth("c2", 2000, seed=5)
    cfg = G.make_config(max_page_n=1000, **C2)
    c = Call(L, [b, a], cfg, [None, [1000, 1500, 500]])

    def refused(tasks=None, cfg=None, **kw):
        if cfg is not None:
            c.cfg, keep = cfg, c.cfg
        code = c.encode(tasks=tasks, **kw)
        if cfg is not None:
            c.cfg = keep
        import torch
        torch.cuda.synchronize()
        return code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT and c.untouched() and not c.d_infos.any().item()

    zero = (C.c_uint64 * 3)(1000, 0, 2000); short = (C.c_uint64 * 3)(1000, 1500, 499); long_ = (C.c_uint64 * 3)(1000, 1500, 501)
    assert refused(c.make_tasks({1: dict(page_sizes=C.cast(zero, C.c_void_p))})), "a page of 0 numbers"
    assert b"0 numbers" in L.pco_gfx_last_error()
    assert refused(c.make_tasks({1: dict(page_sizes=C.cast(short, C.c_void_p))})), "sizes summing to n - 1"
    assert b"paging spec suggests 2999 numbers but 3000 were given" in L.pco_gfx_last_error()
    assert refused(c.make_tasks({1: dict(page_sizes=C.cast(long_, C.c_void_p))})), "sizes summing to n + 1"
    assert refused(c.make_tasks({1: dict(page_sizes=None)})), "page_sizes == NULL with n_pages != 0"
    assert refused(c.make_tasks({0: dict(page_sizes=C.cast(zero, C.c_void_p))})), "page_sizes != NULL with n_pages == 0"
    assert refused(c.make_tasks({1: dict(dst=c.tasks[1].dst + 8)})), "a misaligned dst"
    assert refused(c.make_tasks({1: dict(dst_cap=c.caps[1] - 1)})), "dst_cap one below the exact cap"
    assert refused(c.make_tasks({0: dict(dst_cap=c.caps[0] - 1)})), "dst_cap one below the cap"
    assert refused(sync=False, d_infos=False), "both info arrays NULL"
    bad = G.make_config(max_page_n=1000, **C2); bad.flags = 1 << 9
    assert refused(cfg=bad), "unknown flag bits"
    assert refused(cfg=bad, sync=False), "unknown flag bits, asynchronous form"
    G.check(c.encode())   # the same buffers, unchanged, encode once the arguments are right
    assert c.pieces()[1] == oracle_pieces(a, C2, [1000, 1500, 500])


def test_a_conv1_page_shorter_than_the_order_is_refused(L):
    """Found on the device (the fit decides whether the chunk is Conv1 at all): the chunk's pieces carry INVALID_ARGUMENT, the call fails with it,
    as on the host-buffer path; the healthy chunk beside it is encoded."""
    import pcodec_amd as P
    import test_gpu_conv1_encode as TC
    a = TC.smooth(3000, "int32", seed=1); b = TC.smooth(3000, "int32", seed=2)
    cfg = G.make_config(mode=1, delta=G.DELTA_TRY_CONV1, delta_order=4, conv1=True)
    c = Call(L, [a, b], cfg, [[3, 2997], [4, 2996]])
    assert c.encode() == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT
    print(f"[conv1 short page] piece statuses {c.infos['status'].tolist()}")
    assert (c.infos["status"][:3] == G.ST_INVALID_ARGUMENT).any() and (c.infos["status"][3:] == 0).all()
    assert np.array_equal(c.device_infos()["status"], c.infos["status"])
    with pytest.raises(G.PcoGfxError) as ei:
        host_handle_pieces(a, dict(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_conv1(4), enable_conv1=True), [3, 2997])
    assert ei.value.status == G.ST_INVALID_ARGUMENT
    host = c.slots.cpu().numpy()
    assert (host[c.slot_off[0] + c.caps[0]: c.slot_off[0] + c.caps[0] + GUARD] == GUARD_BYTE).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. compaction
# ---------------------------------------------------------------------------------------------------------------------------------------
def compact(c, gap, dst_offset, dst_cap=None, misalign=0, sync=True, stream=None, d_infos=None, slack=0):
    """One pco_gfx_compact_wrapped_chunks call into a fresh canary-filled destination (+ 64 bytes beyond): (code, total, destination, offsets)"""
    import torch
    body = int((c.infos["len"] + gap).sum())
    cap = body + dst_offset + slack if dst_cap is None else dst_cap
    raw = torch.full((cap + 64 + 16,), CANARY, dtype=torch.uint8, device="cuda")
    dst = raw[misalign: misalign + cap + 64]
    offs = torch.full((c.n_pieces + 1,), 0x1111111111111111, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = C.c_uint64(0xDEAD)
    code = c.L.pco_gfx_compact_wrapped_chunks(c.k, c.tasks, C.addressof(c.cfg), (d_infos if d_infos is not None else c.d_infos).data_ptr(), gap, dst.data_ptr(), cap,
                                              dst_offset, offs.data_ptr(), C.byref(total) if sync else None, handle(stream))
    torch.cuda.synchronize()
    return code, (total.value if sync else None), dst.cpu().numpy(), offs.cpu().numpy().view(np.uint64), cap


def compact_reference(c, infos, gap, dst_offset, cap):
    """numpy: the kept chunks' pieces, each behind `gap` canary bytes, from dst_offset; a chunk with a failed piece is dropped whole"""
    host = c.slots.cpu().numpy()
    want = np.full(cap + 64, CANARY, np.uint8); offs = np.zeros(c.n_pieces + 1, np.uint64); at = dst_offset
    for i in range(c.k):
        k0, k1 = int(c.piece_first[i]), int(c.piece_first[i + 1])
        keep = (infos["status"][k0:k1] == 0).all()
        for k in range(k0, k1):
            offs[k] = at
            if keep:
                src = int(c.slot_off[i]) + int(infos["offset"][k]); n = int(infos["len"][k])
                want[at + gap: at + gap + n] = host[src: src + n]; at += gap + n
    offs[c.n_pieces] = at
    return want, offs


def check_compact(c, gap, dst_offset, misalign=0, sync=True, stream=None, slack=0, infos=None, d_infos=None):
    infos = c.infos if infos is None else infos
    code, total, dst, offs, cap = compact(c, gap, dst_offset, None, misalign, sync, stream, d_infos, slack)
    want, want_offs = compact_reference(c, infos, gap, dst_offset, cap)
    what = f"{c.n_pieces} pieces, gap {gap}, dst_offset {dst_offset}, d_dst at +{misalign}, {'sync' if sync else 'async'}"
    assert code == G.PcoSuccess, what
    assert np.array_equal(offs, want_offs), what
    assert total is None or total == int(want_offs[-1]), what
    if not np.array_equal(dst, want):
        bad = np.flatnonzero(dst != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {int(bad[0])}")


@pytest.fixture(scope="module")
def mixed(L):
    """30 chunks: incompressible u32 chunks whose pages straddle the 16 KiB work slice, one 2 MB page, tiny chunks, compressible ones"""
    rng = np.random.default_rng(21)
    noise = lambda n: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)   # noqa: E731
    arrays, lists = [], []
    for i in range(8):
        arrays.append(noise(20000 + 37 * i)); lists.append([4090 + i, 4096, 4100, 20000 + 37 * i - 12286 - i])   # pages of ~16 380 .. 16 400 bytes and one of ~31 KB
    arrays.append(rng.integers(0, 1 << 63, 1 << 18, dtype=np.uint64)); lists.append(None)   # one page of 2 MiB
    for i in range(12):
        arrays.append(U.synth("c2", 1 + i, seed=i)); lists.append([1] * (1 + i) if i % 2 else None)
    for i in range(9):
        arrays.append(U.synth("c2", 30000 + i, seed=40 + i)); lists.append(None)
    c = Call(L, arrays, G.make_config(mode=1, delta=1, max_page_n=1 << 18), lists)
    G.check(c.encode())
    c.pieces()
    assert c.infos["len"].max() > 2000000 and c.infos["len"].min() < 32
    return c


@pytest.mark.parametrize("gap", [0, 4, 7])
def test_compaction_at_every_destination_alignment(L, mixed, gap):
    for off in range(17):
        check_compact(mixed, gap, off, misalign=0, sync=off % 2 == 0)
    check_compact(mixed, gap, 4099, misalign=3, sync=True, slack=9)
    check_compact(mixed, gap, 5, misalign=11, sync=False)


@pytest.mark.parametrize("n_chunks", [1, 2047, 2048, 2049, 50001])
def test_piece_counts_across_the_scan_rounds(L, n_chunks):
    """Chunks of one number in one page: two pieces each, so 2 .. 100 002 pieces -- both sides of the scan's 4096-piece round and far beyond it."""
    rng = np.random.default_rng(8)
    arrays = [rng.integers(0, 1 << 15, 1).astype((np.uint32, np.uint64, np.int16)[i % 3]) for i in range(min(n_chunks, 3))]
    c = Call(L, U.tile(arrays, n_chunks), G.make_config(mode=1, delta=1))
    G.check(c.encode())
    if n_chunks > 10 ** 5 // 2:
        assert c.n_pieces > 10 ** 5
    want = [oracle_pieces(a, dict(mode=1, delta=1), None) for a in arrays]
    got = c.pieces()
    assert all(got[i] == want[i % 3] for i in range(0, n_chunks, max(n_chunks // 50, 1)))
    assert np.array_equal(c.device_infos(), c.infos)
    for gap, off, sync in ((0, 0, True), (4, 3, False), (7, 16, True)):
        check_compact(c, gap, off, sync=sync)


@pytest.mark.parametrize("where", ["meta", "first page", "last page", "several"])
def test_a_chunk_with_a_failed_piece_drops_whole(L, mixed, where):
    """The failure is a hand-edited COPY of d_infos with one status set (no kernel is made to fail): the chunk contributes neither gaps nor bytes,
    all its d_offsets entries are equal, the later chunks close up."""
    import torch
    infos = mixed.infos.copy()
    pf = mixed.piece_first
    hit = {"meta": [int(pf[0])], "first page": [int(pf[3]) + 1], "last page": [int(pf[mixed.k]) - 1], "several": [int(pf[8]) + 1, int(pf[10]), int(pf[11]) - 1, int(pf[20]) + 1]}[where]
    infos["status"][hit] = G.ST_INVALID_ARGUMENT
    d = torch.from_numpy(infos.view(np.uint8).copy()).cuda()
    for gap, off, sync in ((0, 0, True), (4, 7, False), (7, 4099, True)):
        check_compact(mixed, gap, off, sync=sync, infos=infos, d_infos=d)
    code, total, dst, offs, cap = compact(mixed, 4, 0, d_infos=d)
    for k in hit:
        i = int(np.searchsorted(pf, k, side="right")) - 1
        assert len(set(offs[int(pf[i]): int(pf[i + 1]) + 1].tolist())) == 1


@pytest.mark.parametrize("gap,dst_offset", [(0, 0), (4, 4099)])
def test_overflow_in_both_forms(L, mixed, gap, dst_offset):
    end = dst_offset + int((mixed.infos["len"] + gap).sum())
    check_compact(mixed, gap, dst_offset, sync=True); check_compact(mixed, gap, dst_offset, sync=False)   # end == dst_cap exactly
    for cap in (end - 1, dst_offset, end // 2):
        for sync in (True, False):
            code, total, dst, offs, _ = compact(mixed, gap, dst_offset, dst_cap=cap, sync=sync)
            assert int(offs[-1]) == ALL_ONES, (cap, sync)
            assert (dst == CANARY).all(), f"dst_cap = {cap} < end = {end}: bytes were copied"
            if sync:
                assert code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT and total == ALL_ONES
            else:
                assert code == G.PcoSuccess


def test_compaction_argument_errors(L, mixed):
    c = mixed
    for kw in (dict(d_infos=None), dict(d_offsets=None), dict(d_dst=None)):
        args = dict(d_infos=c.d_infos.data_ptr(), d_offsets=c.d_infos.data_ptr(), d_dst=c.d_infos.data_ptr()); args.update(kw)
        code = L.pco_gfx_compact_wrapped_chunks(c.k, c.tasks, C.addressof(c.cfg), args["d_infos"], 0, args["d_dst"], 1 << 30, 0, args["d_offsets"], None, None)
        assert code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT, kw
    assert np.array_equal(c.device_infos(), c.infos)


def test_gap_4_builds_the_pcopage_file(L):
    """The reference's `pcopage` bench codec (pco_cli/src/bench/codecs/pcopage.rs:33-75) writes: u64 n | u32 chunk count | the wrapped header | per
    chunk: u32 page count, the ChunkMeta, then per page: u32 page_n, the page -- all little-endian.  Compaction with gap = 4 behind 14 bytes of room
    leaves exactly the words to fill in; the file must equal that layout built in Python from the ORACLE's pieces."""
    import struct
    n, chunk_n, page_n = 100000, 30000, 7000
    nums = U.synth("c2", n, seed=77)
    chunk_ns = equal_pages(n, chunk_n); at = np.concatenate([[0], np.cumsum(chunk_ns)])
    chunks = [nums[at[i]: at[i + 1]] for i in range(len(chunk_ns))]
    okw = dict()   # pcopage: ChunkConfig::default() (Auto mode, Auto delta) with its level and page size
    hdr = np.zeros(8, np.uint8); assert L.pco_wrapped_write_header(hdr.ctypes.data_as(C.c_void_p), 8) == 2
    want = struct.pack("<QI", n, len(chunks)) + hdr[:2].tobytes()
    for ch in chunks:
        meta, pages, ns = oracle_pieces(ch, okw, None, page_n)
        want += struct.pack("<I", len(pages)) + meta
        for p, pn in zip(pages, ns):
            want += struct.pack("<I", pn) + p
    c = Call(L, chunks, G.make_config(max_page_n=page_n))
    G.check(c.encode())
    code, total, dst, offs, cap = compact(c, 4, 14, slack=5)
    assert code == G.PcoSuccess and total == len(want)
    assert (dst[:14] == CANARY).all() and all((dst[int(offs[k]): int(offs[k]) + 4] == CANARY).all() for k in range(c.n_pieces)) and (dst[total:] == CANARY).all()
    file = dst[:total].copy()
    file[:14] = np.frombuffer(struct.pack("<QI", n, len(chunks)) + hdr[:2].tobytes(), np.uint8)
    for i in range(c.k):
        k0 = int(c.piece_first[i])
        file[int(offs[k0]): int(offs[k0]) + 4] = np.frombuffer(struct.pack("<I", len(c.pages[i])), np.uint8)
        for p, pn in enumerate(c.pages[i]):
            o = int(offs[k0 + 1 + p]); file[o: o + 4] = np.frombuffer(struct.pack("<I", pn), np.uint8)
    assert file.tobytes() == want


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. streams
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pipeline_inputs():
    rng = np.random.default_rng(13)
    dist = [U.synth("c2", 16384, seed=1), rng.normal(size=16384).astype(np.float32), U.synth("c2", 9000, seed=2), np.cumsum(rng.integers(-5, 6, 12000)).astype(np.int32)]
    lists = [None, [5000, 11384], [1, 8999], None]
    return dist, lists


@pytest.mark.parametrize("n_chunks", [96, 300])
def test_asynchronous_encode_and_compaction_on_a_caller_stream(L, n_chunks):
    """On a non-blocking stream: a bounded device delay, then the real numbers copied over a source that held OTHER valid numbers, then
    pco_gfx_compress_wrapped_chunks_ex(infos = NULL) and pco_gfx_compact_wrapped_chunks(total = NULL) with no host synchronisation in between; one
    synchronisation; then the directory (d_infos, d_offsets) and the decode out of the compacted stream.  A kernel ordered anywhere but behind the
    stream encodes the stale numbers: clean bytes, not the oracle's.  (Whether the calls returned before the stream drained is reported, not asserted.)"""
    import torch
    dist, lists = _pipeline_inputs()
    stale = [np.roll(a, 7) for a in dist]
    cfg = G.make_config(max_page_n=6000, **C2)
    c = Call(L, U.tile(dist, n_chunks), cfg, U.tile(lists, n_chunks))
    old = Call(L, U.tile(stale, n_chunks), cfg, U.tile(lists, n_chunks))
    want = [oracle_pieces(a, C2, pl, 6000) for a, pl in zip(dist, lists)]
    work = old.src.clone()
    c.src = work; c.tasks = c.make_tasks()
    gap, off = 4, 14
    cap = int(sum(c.caps)) + gap * c.n_pieces + off
    dst = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda"); d_offs = torch.zeros(c.n_pieces + 1, dtype=torch.int64, device="cuda")
    fresh = torch.from_numpy(c.host_in).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    U.device_delay(s)
    with torch.cuda.stream(s):
        work.copy_(fresh, non_blocking=True)
    G.check(c.encode(sync=False, stream=s))
    print(f"[async form] pco_gfx_compress_wrapped_chunks_ex: returned {'AFTER' if s.query() else 'BEFORE'} the stream drained")
    G.check(L.pco_gfx_compact_wrapped_chunks(c.k, c.tasks, C.addressof(cfg), c.d_infos.data_ptr(), gap, dst.data_ptr(), cap, off, d_offs.data_ptr(), None, handle(s)))
    print(f"[async form] pco_gfx_compact_wrapped_chunks: returned {'AFTER' if s.query() else 'BEFORE'} the stream drained")
    s.synchronize()
    c.infos = c.device_infos()
    got = c.pieces()
    for i in range(c.k):
        assert got[i] == want[i % len(want)], f"chunk {i} behind a pending copy of its input is not the oracle's"
    want_dst, want_offs = compact_reference(c, c.infos, gap, off, cap)
    offs = d_offs.cpu().numpy().view(np.uint64)
    assert np.array_equal(offs, want_offs) and np.array_equal(dst.cpu().numpy(), want_dst)
    c.decode_and_compare(base_of=lambda k: dst.data_ptr() + int(offs[k]) + gap, stream=s)


def test_two_streams_share_one_workspace(L):
    """Asynchronous encode + compaction of batch A on stream 1, of batch B on stream 2 right behind it, of A again on stream 1: one thread, one
    workspace -- every call is ordered behind the previous one's kernels, so all three results are the oracle's."""
    import torch
    dist, lists = _pipeline_inputs()
    cfg = G.make_config(max_page_n=6000, **C2)
    want = [oracle_pieces(a, C2, pl, 6000) for a, pl in zip(dist, lists)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    runs = []
    for s, shift in ((s1, 0), (s2, 1), (s1, 2)):
        order = [(j + shift) % 4 for j in range(4)]
        c = Call(L, U.tile([dist[j] for j in order], 128), cfg, U.tile([lists[j] for j in order], 128))
        cap = int(sum(c.caps)); dst = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda"); d_offs = torch.zeros(c.n_pieces + 1, dtype=torch.int64, device="cuda")
        runs.append((c, order, dst, d_offs, cap, s))
    torch.cuda.synchronize()
    U.device_delay(s1, ms=10)
    for c, order, dst, d_offs, cap, s in runs:
        G.check(c.encode(sync=False, stream=s))
        G.check(L.pco_gfx_compact_wrapped_chunks(c.k, c.tasks, C.addressof(cfg), c.d_infos.data_ptr(), 0, dst.data_ptr(), cap, 0, d_offs.data_ptr(), None, handle(s)))
    torch.cuda.synchronize()
    for c, order, dst, d_offs, cap, s in runs:
        c.infos = c.device_infos()
        got = c.pieces()
        assert all(got[i] == want[order[i % 4]] for i in range(c.k))
        want_dst, want_offs = compact_reference(c, c.infos, 0, 0, cap)
        assert np.array_equal(d_offs.cpu().numpy().view(np.uint64), want_offs) and np.array_equal(dst.cpu().numpy(), want_dst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. pass-cutting (child processes: PCO_GFX_WORKSPACE_GB is read once, when the library is loaded)
# ---------------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], ".."))
import numpy as np
import gpu_util as U
import test_gpu_wrapped_writer as T
from pcodec_amd import _lib as G
L = G.lib()
rng = np.random.default_rng(4)
dist = [U.synth("c2", 20000, seed=1), np.cumsum(rng.integers(-5, 6, 20000)).astype(np.int32), U.synth("c2", 15000, seed=2)]
lists = [None, [1, 9999, 10000], [7000, 8000]]
cfg = G.make_config(max_page_n=6000, **T.C2)
c = T.Call(L, U.tile(dist, 200), cfg, U.tile(lists, 200))
est = L.pco_gfx_wrapped_scratch_estimate(c.k, c.tasks, C.addressof(cfg))
L.pco_gfx_profile_begin()
G.check(c.encode())
names = C.create_string_buffer(1 << 18); ms = (C.c_float * 16384)()
nk = L.pco_gfx_profile_end(names, len(names), ms, 16384)
kernels = names.raw.split(b"\0")[:nk]
c.pieces()
print("RESULT " + json.dumps(dict(estimate=est, splits=sum(k.startswith(b"enc_split_kernel") for k in kernels), inits=kernels.count(b"enc_init_kernel"),
      slots=hashlib.sha256(c.slots.cpu().numpy().tobytes()).hexdigest(), infos=hashlib.sha256(c.infos.tobytes()).hexdigest(),
      d_infos=hashlib.sha256(c.device_infos().tobytes()).hexdigest(), workspace=L.pco_gfx_workspace_bytes())))
"""


def _child(env_gb):
    env = dict(os.environ); env.pop("PCO_GFX_WORKSPACE_GB", None)
    if env_gb is not None:
        env["PCO_GFX_WORKSPACE_GB"] = env_gb
    r = subprocess.run([sys.executable, "-c", CHILD, HERE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_a_synchronous_call_beyond_the_budget_runs_in_passes():
    """200 chunks under a budget of 0.55 x the library's own worst-case estimate for them (pco_gfx_wrapped_scratch_estimate: the figure the pass-cutting
    divides the budget by), so 110 chunks fit a pass -- above the floor of 64 -- and the call takes two balanced passes of 100: the same bytes, infos and d_infos as the uncut call, and
    the split and init kernels launched once per pass."""
    whole = _child(None)
    assert whole["inits"] == 1 and whole["estimate"] > 0
    gb = whole["estimate"] * 0.55 / 1e9
    cut = _child(repr(gb))
    print(f"[passes] estimate {whole['estimate']} B for 200 chunks; budget {gb:.6f} GB: enc_init_kernel x {cut['inits']}, split kernels {cut['splits']} (uncut: {whole['splits']}); "
          f"workspace {cut['workspace']} B vs {whole['workspace']} B uncut")
    assert cut["inits"] == 2 and cut["splits"] > whole["splits"] >= 1
    assert (cut["slots"], cut["infos"], cut["d_infos"]) == (whole["slots"], whole["infos"], whole["d_infos"])
    assert cut["workspace"] <= whole["workspace"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the Python layer
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_paged_python_round_trip_and_blob(L):
    import torch
    import pcodec_amd as P
    from pcodec_amd import paged
    dist, lists = _pipeline_inputs()
    config = P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_consecutive(1), paging_spec=P.PagingSpec.equal_pages_up_to(6000))
    tensors = [torch.from_numpy(a.view(np.uint8).copy()).cuda().view(getattr(torch, a.dtype.name)) for a in dist]
    s = torch.cuda.Stream()
    out = paged.compress_chunks(tensors, config, page_sizes=lists, gap=4, stream=s)
    d = out.directory
    # the C-level compaction of the same call, and the oracle's pieces
    c = Call(L, dist, config.to_c(), lists)
    G.check(c.encode())
    code, total, dst, offs, cap = compact(c, 4, 0)
    assert code == G.PcoSuccess and out.total == total
    blob = out.blob[:total].cpu().numpy()
    for e in d:
        want = oracle_pieces(dist[e.chunk], C2, lists[e.chunk], 6000)
        piece = want[0] if e.piece == 0 else want[1][e.piece - 1]
        assert blob[e.offset: e.offset + e.length].tobytes() == piece and e.n == (0 if e.piece == 0 else want[2][e.piece - 1])
        assert np.array_equal(blob[e.offset: e.offset + e.length], dst[e.offset: e.offset + e.length])
    assert [e.offset - 4 for e in d] == offs[:-1].tolist()
    back = paged.decompress_chunks(out.blob, d, [a.dtype.name for a in dist], stream=s)
    for a, b in zip(dist, back):
        assert U.bits_equal(a, b.cpu().numpy().view(a.dtype))
    one = paged.compress_chunks([tensors[0]], P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_consecutive(1),
                                                          paging_spec=P.PagingSpec.exact_page_sizes([16000, 384])))
    assert [e.n for e in one.directory] == [0, 16000, 384]
    with pytest.raises(ValueError):
        paged.compress_chunks(tensors, P.ChunkConfig(paging_spec=P.PagingSpec.exact_page_sizes([16384])))
