"""-m gpu: the device codec at the ends of the ranges the format and the C ABI allow.

(a) SIZE: chunks and pages of 2^24 numbers (`kMaxEntries`), the largest the format's 24-bit count field holds.  A chunk of 2^24 numbers has
    exactly 2^16 batches, so a batch, tile or segment index kept in 16 bits overflows there and only there; the rows below are one chunk per
    call through the batched entry points, each named after what it strikes.  One test per row; each prints the kernels that took the chunk, the
    device time of the encode and of the decode, and the workspace the call took.
(b) MODE PARAMETERS: the grid of tests/format_limits_util.py (int-mult bases up to 2^w - 1, float-quant k up to the mantissa width, float-mult
    bases that are subnormal, negative, or have an infinite or subnormal inverse; data with the types' extremes, +-0, subnormals, infinities
    and NaN payloads) at n = 1, 255, 257 and 3000 -- tests/test_format_limits.py pins the oracle on the same grid first.
(c) Two other ends that cost little: consecutive delta orders 1..7 on chunks and pages of 1..8 numbers (a delta state longer than the page),
    and level 12 at n = 2^20 on 16-bit types (4096 unoptimised bins asked of at most 65 536 distinct values, and of far fewer).

Every check compares bytes with the oracle and numbers bit for bit with the input; device outputs sit in guard-filled buffers.  Nothing is
skipped: a row the device refuses fails."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import format_limits_util as F
import gpu_util as U
import oracle_lib as O
from pcodec_amd import _lib as G
from test_gpu_width_paths import GUARD, decode_call, encode_call
from test_gpu_wrapped_writer import INFO_DT, Call

pytestmark = pytest.mark.gpu

MAX_N = 1 << 24   # pco_dev.h kMaxEntries, constants.rs MAX_ENTRIES


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def header_len(f):
    """Length of a standalone file's header, read from its varint n_hint."""
    bits = int.from_bytes(f[6:16], "little")
    return 6 + (6 + 1 + (bits & 63) + 7) // 8 + 2


def chunk_of(f):
    """The one chunk of a one-chunk standalone file."""
    return f[header_len(f):-1]


def profile_ms(L):
    """{kernel or span name: milliseconds} since pco_gfx_profile_begin()."""
    import torch
    torch.cuda.synchronize()
    names = C.create_string_buffer(1 << 16); ms = (C.c_float * 4096)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 4096)
    raw = names.raw; out = {}; pos = 0
    for i in range(nk):
        e = raw.index(b"\0", pos); name = raw[pos:e].decode(); pos = e + 1
        out[name] = out.get(name, 0.0) + float(ms[i])
    return out


def walkers(names):
    return sorted(n for n in names if "walk" in n and "hist" not in n)


# =============================================================================================================== (a) size limits
def _walk_u8(n):
    w = np.cumsum(np.random.default_rng(1).integers(-2, 3, n, dtype=np.int8), dtype=np.int64) % 510
    return np.where(w > 255, 510 - w, w).astype(np.uint8)          # a random walk reflected at 0 and 255


def _ramp_u64(n):
    return np.uint64(1 << 40) + np.uint64(1000) * np.arange(n, dtype=np.uint64) + np.random.default_rng(2).integers(0, 512, n).astype(np.uint64)


def _noise_u64(n):
    return np.frombuffer(np.random.default_rng(3).bytes(n * 8), np.uint64)


def _periodic_i64(n):
    base = np.random.default_rng(40).integers(-(1 << 40), 1 << 40, 365)
    return (base[np.arange(n) % 365] + np.random.default_rng(4).integers(-3, 4, n)).astype(np.int64)


def _decimals_f32(n):
    return (np.random.default_rng(5).integers(1000, 10000, n) / 100.0).astype(np.float32)


SIZE_ROWS = {
    "u8-walk-delta1": (_walk_u8, MAX_N, dict(mode=1, delta=2, delta_order=1)),             # narrow fused walk, 2^16 full batches
    "u64-ramp-order7": (_ramp_u64, MAX_N - 1, dict(mode=1, delta=2, delta_order=7)),       # last batch of 255, longest halo
    "u64-incompressible": (_noise_u64, MAX_N, dict(mode=1, delta=1)),                      # fallback chunk at the largest body: 2^30 bits
    "i64-periodic-lookback": (_periodic_i64, MAX_N, dict(mode=1, delta=3)),                # hash pre-pass and pipeline positions
    "f32-decimals-fmult": (_decimals_f32, MAX_N - 256, dict(mode=2, mode_f64=0.01, delta=1)),   # two variables, 65 535 batches exactly
}


@functools.lru_cache(maxsize=None)
def size_row(name):
    """(array, config keywords, the oracle's chunk), computed once per row (the u8 row serves four tests)."""
    make, n, kw = SIZE_ROWS[name]
    a = np.ascontiguousarray(make(n))
    t0 = time.time()
    want = chunk_of(O.simple_compress(a, O.make_config(max_page_n=n, enable_8_bit=True, **kw)))
    print(f"{name}: n = {n}, oracle encode {time.time() - t0:.2f} s, {len(want)} bytes")
    assert int.from_bytes(want[1:4], "little") == n - 1     # the 24-bit count field (0xFFFFFF at n = 2^24)
    return a, kw, want


def encode_one(L, a, cfg):
    """One chunk through pco_gfx_compress_chunks into a guard-filled buffer: (chunk bytes, {kernel: ms})."""
    import torch
    dt = G.DTYPE_BYTE[a.dtype.name]
    src = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
    cap = (L.pco_gfx_guarantee_chunk_size(a.size, dt) + 64 + 15) // 16 * 16
    dst = torch.full((cap + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    task = (G.EncodeTask * 1)(G.EncodeTask(src.data_ptr(), a.size, dst.data_ptr(), cap, dt, 0))
    res = (G.TaskResult * 1)()
    L.pco_gfx_profile_begin()
    G.check(L.pco_gfx_compress_chunks(1, task, C.byref(cfg), res, None, None))
    ms = profile_ms(L)
    assert res[0].status == 0 and 0 < res[0].n_out <= cap, (res[0].status, res[0].n_out)
    host = dst.cpu().numpy()
    assert (host[cap:] == GUARD).all(), "written behind the destination's capacity"
    return host[: res[0].n_out].tobytes(), ms


@pytest.mark.parametrize("name", list(SIZE_ROWS))
def test_one_chunk_at_the_size_limit(L, name):
    """One chunk of 2^24 numbers (or just below, where the row says so) through pco_gfx_compress_chunks and pco_gfx_decompress_chunks: the
    bytes are the oracle's, the oracle's bytes decode to the input, nothing is written behind the numbers, a walker kernel took the chunk in
    each direction, and the library's scratch stays within 64 bytes per number (up to three full-width latent variables,
    two sort buffers, six 16-bit lookback proposals, 16-bit latents, symbols, tANS fields and the dissect words come to 61) plus 256 MiB."""
    import torch
    a, kw, want = size_row(name)
    L.pco_gfx_release_workspace()
    t0 = time.time()
    got, enc = encode_one(L, a, G.make_config(enable_8_bit=True, **kw))
    t_enc = time.time() - t0
    ws1 = L.pco_gfx_workspace_bytes()
    t0 = time.time()
    L.pco_gfx_profile_begin()
    decode_call([want], [a])
    dec = profile_ms(L)
    t_dec = time.time() - t0
    ws2 = L.pco_gfx_workspace_bytes()
    top = lambda ms: [(k, round(v, 2)) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])[:8]]
    print(f"{name}: encode {sum(enc.values()):.1f} ms on the device, walkers {walkers(enc)}, top {top(enc)}")
    print(f"{name}: decode {sum(dec.values()):.1f} ms on the device, walkers {walkers(dec)}, top {top(dec)}")
    print(f"{name}: wall encode {t_enc:.2f} s, decode {t_dec:.2f} s; workspace after encode / decode {ws1 / 2**20:.0f} / {ws2 / 2**20:.0f} MiB "
          f"for {a.nbytes / 2**20:.0f} MiB of input")
    assert len(got) == len(want) and got == want, (name, len(got), len(want))
    assert walkers(enc), (name, sorted(enc))
    assert walkers(dec), (name, sorted(dec))
    assert max(ws1, ws2) <= 64 * a.size + (256 << 20), (name, ws1, ws2)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pages", [[MAX_N], [MAX_N - 1, 1]], ids=["one-page", "all-but-one-and-one"])
def test_wrapped_pages_at_the_size_limit(L, pages):
    """The u8 row through pco_gfx_compress_wrapped_chunks_ex under PagingSpec::Exact: one page of 2^24 numbers, and 2^24 - 1 numbers and a
    page of one.  ChunkMeta and pages equal the oracle's, guards intact, pco_gfx_decompress_pages gives the input back."""
    a, kw, _ = size_row("u8-walk-delta1")
    want = O.wrapped_compress(a, O.make_config(enable_8_bit=True, **kw), max_pages=len(pages) + 1, exact_pages=pages)
    c = Call(L, [a], G.make_config(enable_8_bit=True, **kw), [pages])
    G.check(c.encode())
    meta, pgs, ns = c.pieces()[0]
    assert ns == want[2] == pages and meta == want[0]
    assert [len(p) for p in pgs] == [len(p) for p in want[1]] and pgs == want[1]
    c.decode_and_compare()


def _status(L):
    return L.pco_gfx_last_status()


def test_one_number_beyond_the_limit_is_refused_everywhere(L):
    """n = 2^24 + 1 in one chunk: InvalidArgument from every encode entry point (like the oracle), nothing written; a page task that asks
    for 2^24 + 1 numbers reports InvalidArgument and writes nothing.  (Two kernels hold that check: the fast planner, decode_fast.hip, answers
    such a task with its internal "retry on the legacy path" status, and the wrapped branch of pco_decode_kernel, decode_kernel.hip, then names
    InvalidArgument.  The hand-over is not visible from outside: this test sees only the final status and the untouched destination.)"""
    import torch
    n = MAX_N + 1
    a = (np.arange(n) % 7).astype(np.uint8)
    dt = G.DTYPE_BYTE["uint8"]
    kw = dict(mode=1, delta=2, delta_order=1)
    cfg = G.make_config(enable_8_bit=True, **kw)
    for call in (lambda: O.simple_compress(a, O.make_config(max_page_n=n, enable_8_bit=True, **kw)),
                 lambda: O.wrapped_compress(a, O.make_config(enable_8_bit=True, **kw), max_pages=3, exact_pages=[MAX_N, 1])):
        with pytest.raises(O.OracleError) as ei:
            call()
        assert ei.value.kind == O.ERR_INVALID_ARGUMENT
    # host-buffer entry points
    cap = L.pco_gfx_guarantee_file_size(n, dt, n) + 64
    assert cap > n
    dst = np.full(cap, GUARD, np.uint8); nw = C.c_size_t(0)
    big = G.make_config(enable_8_bit=True, max_page_n=n, **kw)
    rc = L.pco_gfx_simple_compress_into_ex(a.ctypes.data_as(C.c_void_p), n, dt, C.byref(big), 0, dst.ctypes.data_as(C.c_void_p), cap, C.byref(nw))
    assert rc != 0 and _status(L) == G.ST_INVALID_ARGUMENT and (dst == GUARD).all(), (rc, _status(L))
    one = (C.c_size_t * 1)(n)
    rc = L.pco_gfx_simple_compress_into_exact(a.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.c_ubyte(dt), C.byref(cfg), C.c_int(0), one, C.c_size_t(1),
                                              dst.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(nw))
    assert rc != 0 and _status(L) == G.ST_INVALID_ARGUMENT and (dst == GUARD).all(), (rc, _status(L))
    for exact in (None, (C.c_size_t * 2)(MAX_N, 1)):
        handle = C.c_void_p(0)
        if exact is None:
            rc = L.pco_chunk_compressor_new(a.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.c_ubyte(dt), C.byref(cfg), C.byref(handle))
        else:
            rc = L.pco_chunk_compressor_new_exact(a.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.c_ubyte(dt), C.byref(cfg), exact, C.c_size_t(2), C.byref(handle))
        assert rc != 0 and _status(L) == G.ST_INVALID_ARGUMENT and not handle.value, (exact is None, rc, _status(L))
    # device-buffer entry points: real buffers of the full size, so that an entry point that did not refuse would stay inside them
    src = torch.from_numpy(a).cuda()
    cap = (L.pco_gfx_guarantee_chunk_size(n, dt) + 64 + 15) // 16 * 16
    assert cap > n
    d = torch.full((cap + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    task = (G.EncodeTask * 1)(G.EncodeTask(src.data_ptr(), n, d.data_ptr(), cap, dt, 0))
    res = (G.TaskResult * 1)()
    rc = L.pco_gfx_compress_chunks(1, task, C.byref(cfg), res, None, None)
    assert rc != 0 and _status(L) == G.ST_INVALID_ARGUMENT and bool((d == GUARD).all()), (rc, _status(L))
    infos = np.zeros(80, INFO_DT)
    rc = L.pco_gfx_compress_wrapped_chunks(1, task, C.byref(cfg), U.ptr(infos), None)
    assert rc != 0 and _status(L) == G.ST_INVALID_ARGUMENT and bool((d == GUARD).all()), (rc, _status(L))
    sizes = (C.c_uint64 * 2)(MAX_N, 1)
    wt = (G.WrappedTask * 1)(G.WrappedTask(src.data_ptr(), n, d.data_ptr(), cap // 16 * 16, dt, 2, C.cast(sizes, C.c_void_p)))
    rc = L.pco_gfx_compress_wrapped_chunks_ex(1, wt, C.byref(cfg), U.ptr(infos), None, None)
    assert rc != 0 and _status(L) == G.ST_INVALID_ARGUMENT and bool((d == GUARD).all()), (rc, _status(L))
    # decode: a page task of 2^24 + 1 numbers (a page task's count is the dst_cap of the decode task the kernels see: the wrapped branch of
    # pco_decode_kernel refuses it as InvalidArgument, and the fast planner hands it there)
    meta, pgs, _ = O.wrapped_compress(a[:1000], O.make_config(enable_8_bit=True, **kw))
    blob = torch.from_numpy(np.frombuffer(meta + bytes(16) + pgs[0] + bytes(16), np.uint8).copy()).cuda()
    pt = np.zeros(1, U.PAGE_DT)
    pt[0] = (blob.data_ptr(), len(meta), blob.data_ptr() + len(meta) + 16, len(pgs[0]), d.data_ptr(), n, dt, 4)
    pres = np.zeros(1, U.RES_DT)
    rc = L.pco_gfx_decompress_pages(1, U.ptr(pt), U.ptr(pres), None, None)
    assert rc != 0 and pres[0]["status"] == G.ST_INVALID_ARGUMENT and pres[0]["n_out"] == 0, (rc, pres[0])
    assert bool((d == GUARD).all()), "a refused page task wrote to its destination"
    pt[0]["page_n"] = 1000      # the same task with the page's own count is fine
    G.check(L.pco_gfx_decompress_pages(1, U.ptr(pt), U.ptr(pres), None, None))
    assert pres[0]["n_out"] == 1000 and np.array_equal(d[:1000].cpu().numpy(), a[:1000]) and bool((d[1000:] == GUARD).all())
    # a standalone-chunk task's dst_cap is a capacity, not a count: more room than any chunk can fill is no error
    d.fill_(GUARD)
    small = chunk_of(O.simple_compress(a[:1000], O.make_config(enable_8_bit=True, **kw)))
    blob = torch.from_numpy(np.frombuffer(small + bytes(16), np.uint8).copy()).cuda()
    dtask = (G.DecodeTask * 1)(G.DecodeTask(blob.data_ptr(), len(small), d.data_ptr(), n, dt, 0))
    dres = (G.TaskResult * 1)()
    G.check(L.pco_gfx_decompress_chunks(1, dtask, dres, None, None))
    assert dres[0].n_out == 1000 and np.array_equal(d[:1000].cpu().numpy(), a[:1000]) and bool((d[1000:] == GUARD).all())


def test_a_stream_cut_in_its_last_batch_at_the_size_limit(L):
    """The u8 row's stream, 16 bytes short (its last batch of 256 numbers takes more than that: five equally likely steps are over two bits
    each): InsufficientData, nothing written behind the chunk's numbers."""
    a, _, want = size_row("u8-walk-delta1")
    assert len(want) > 2 * (MAX_N // 8)
    decode_call([want[:-16]], [a], damaged={0})


# =============================================================================================================== (b) mode parameters
GRID_SIZES = (1, 255, 257, 3000)


def simple_compress_guarded(L, arr, cfg):
    dt = G.DTYPE_BYTE[arr.dtype.name]
    cap = L.pco_gfx_guarantee_file_size(arr.size, dt, cfg.max_page_n) + 64
    dst = np.full(cap + 64, GUARD, np.uint8); n = C.c_size_t(0)
    G.check(L.pco_gfx_simple_compress_into_ex(arr.ctypes.data_as(C.c_void_p), arr.size, dt, C.byref(cfg), 0, dst.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    assert (dst[cap:] == GUARD).all()
    return dst[: n.value].tobytes()


def simple_decompress_guarded(L, data, np_dtype, n):
    buf = np.frombuffer(bytes(data), np.uint8)
    out = np.full((n + 8) * np.dtype(np_dtype).itemsize, GUARD, np.uint8); k = C.c_size_t(0)
    G.check(L.pco_standalone_simple_decompress_into(buf.ctypes.data_as(C.c_void_p), len(buf), G.DTYPE_BYTE[np.dtype(np_dtype).name], out.ctypes.data_as(C.c_void_p), n, C.byref(k)))
    assert (out[n * np.dtype(np_dtype).itemsize:] == GUARD).all(), "written behind the numbers"
    return out[: k.value * np.dtype(np_dtype).itemsize].view(np_dtype)


def generator_file(arr, kw, **extra):
    return O.test_encode(arr, mode=kw["mode"], mode_f64=kw.get("mode_f64", 0.0), mode_u64=kw.get("mode_u64", 0), **extra)


@functools.lru_cache(maxsize=None)
def grid_rows(n):
    """[(id, array, keywords, oracle file, generator file)]: the oracle's work, once per size."""
    return [(i, a, kw, O.simple_compress(a, O.make_config(enable_8_bit=True, **kw)), generator_file(a, kw)) for i, a, kw in F.grid(n)]


@pytest.mark.parametrize("n", GRID_SIZES)
def test_mode_parameter_limits_through_the_standalone_entry_points(L, n):
    """Every row of the grid: the device's file equals the oracle's, the oracle's file decodes to the input, and so does the generator's
    (which keeps the mode where the encoder's fallback would write a classic chunk: the join runs on every row)."""
    bad = []
    for rid, a, kw, want, gen in grid_rows(n):
        try:
            got = simple_compress_guarded(L, a, G.make_config(enable_8_bit=True, **kw))
            if got != want: bad.append((rid, "encode bytes"))
            if not U.bits_equal(simple_decompress_guarded(L, want, a.dtype, a.size), a): bad.append((rid, "decode of the oracle's file"))
            if not U.bits_equal(simple_decompress_guarded(L, gen, a.dtype, a.size), a): bad.append((rid, "decode of the generator's file"))
        except G.PcoGfxError as e:
            bad.append((rid, f"status {e.status}: {e}"))
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("bits", [8, 16, 32, 64])
def test_mode_parameter_limits_in_batched_calls(L, bits):
    """All rows of a width, every size: ONE decode call over the oracle's and the generator's chunks (every mode, base and k side by side), and
    one encode call per config (a call has one config) over the rows that share it."""
    rows = [r for n in GRID_SIZES for r in grid_rows(n) if F.width(r[1].dtype) == bits]
    assert len(rows) >= 4 * 14
    blobs = [chunk_of(r[3]) for r in rows] + [chunk_of(r[4]) for r in rows]
    L.pco_gfx_profile_begin()
    decode_call(blobs, [r[1] for r in rows] * 2)
    print(f"{bits}-bit: {len(blobs)} chunks decoded by {sorted(profile_ms(L))}")
    by_cfg = {}
    for r in rows:
        by_cfg.setdefault(tuple(sorted(r[2].items())), []).append(r)
    for key, rs in by_cfg.items():
        chunks, _ = encode_call([r[1] for r in rs], G.make_config(enable_8_bit=True, **dict(key)))
        bad = [r[0] for r, c in zip(rs, chunks) if c != chunk_of(r[3])]
        assert not bad, (dict(key), bad)


@pytest.mark.parametrize("row", F.refused(), ids=[r[0] for r in F.refused()])
def test_parameters_beyond_the_ranges_are_refused_like_the_oracle_does(L, row):
    _, a, kw = row
    with pytest.raises(O.OracleError) as oe:
        O.simple_compress(a, O.make_config(enable_8_bit=True, **kw))
    with pytest.raises(G.PcoGfxError) as ge:
        U.gpu_simple_compress(a, G.make_config(enable_8_bit=True, **kw))
    assert oe.value.kind == O.ERR_INVALID_ARGUMENT and ge.value.status == G.ST_INVALID_ARGUMENT, (oe.value.kind, ge.value.status)
    with pytest.raises(G.PcoGfxError) as ge:
        U.gpu_batched([a, a], G.make_config(enable_8_bit=True, **kw))
    assert ge.value.status == G.ST_INVALID_ARGUMENT


def with_int_mult_base(f, w, base):
    """A standalone one-chunk int-mult file with the base in its ChunkMeta replaced (chunk: dtype byte, 24-bit n - 1, then ChunkMeta: 4 bits of
    mode, the base in w bits, least significant bit first)."""
    h = header_len(f); pos = 8 * (h + 4) + 4
    x = int.from_bytes(f, "little")
    assert (x >> (8 * (h + 4))) & 15 == 1, "not an int-mult chunk"
    x = (x & ~(((1 << w) - 1) << pos)) | (base << pos)
    return x.to_bytes(len(f), "little")


@pytest.mark.parametrize("dt", F.INT_TYPES, ids=lambda d: np.dtype(d).name)
def test_decode_int_mult_products_that_wrap_the_type(L, dt):
    """A stream no encoder writes: latents split by base 3 under a ChunkMeta that says 2^(w-1) + 1 (and 2^w - 1), so that p * base wraps and
    the secondary exceeds the base.  int_mult.rs joins with wrapping_mul / wrapping_add: the model's join names the numbers, the oracle's
    decoder agrees, and the device returns them in a single and in a batched call -- under no delta and with a delta'd secondary."""
    w = F.width(dt)
    blobs, wants = [], []
    for n in (1, 255, 257, 3000):
        a = F.int_data(dt, n, 3, np.random.default_rng([w, n]))
        p, s = F.split_int_mult(a, 3)
        for base in ((1 << (w - 1)) + 1, (1 << w) - 1):
            want = F.join_int_mult(p, s, base, dt)
            for extra in (dict(), dict(delta=O.TE_DELTA_CONSECUTIVE, order=1, secondary_uses_delta=True)):
                f = with_int_mult_base(generator_file(a, dict(mode=4, mode_u64=3), **extra), w, base)
                info, _ = O.inspect_first_chunk(f)
                assert info.mode_kind == 1 and info.mode_base_latent == base
                assert U.bits_equal(O.simple_decompress(f, dt, cap=n + 8), want)
                assert U.bits_equal(simple_decompress_guarded(L, f, dt, n), want), (np.dtype(dt).name, n, base, extra)
                blobs.append(chunk_of(f)); wants.append(want)
    assert any(not U.bits_equal(x, y) for x, y in zip(wants[::4], wants[2::4]))
    decode_call(blobs, wants)


@pytest.mark.parametrize("ft", F.FLOAT_TYPES, ids=lambda d: np.dtype(d).name)
def test_decode_float_quant_at_the_mantissa_width_with_a_delta_secondary(L, ft):
    """k = prec (the primary keeps sign and exponent only, the sign cutoff MID >> k is 2^(w - 1 - prec)) in streams whose SECONDARY is
    delta-encoded too, which no reference encoder writes."""
    w = F.width(ft); k = F.PREC[w]
    blobs, wants = [], []
    for n in (1, 255, 257, 3000):
        a = F.quant_data(ft, n, k, np.random.default_rng([w, n, 7]))
        for order in (1, 2):
            f = generator_file(a, dict(mode=3, mode_u64=k), delta=O.TE_DELTA_CONSECUTIVE, order=order, secondary_uses_delta=True)
            info, _ = O.inspect_first_chunk(f)
            assert info.mode_kind == 3 and info.mode_k == k
            assert U.bits_equal(O.simple_decompress(f, ft, cap=n + 8), a)
            assert U.bits_equal(simple_decompress_guarded(L, f, ft, n), a), (np.dtype(ft).name, n, order)
            blobs.append(chunk_of(f)); wants.append(a)
    decode_call(blobs, wants)


# =============================================================================================================== (c) other ends
@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float16, np.uint32, np.float32, np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_delta_state_longer_than_the_page(L, dt):
    """Consecutive orders 1..7 on chunks of 1..8 numbers (standalone and batched) and on a wrapped chunk in pages of 1..8 numbers: wherever the
    order exceeds the page, the page is all delta state (delta/consecutive.rs) and its body holds no latents."""
    rng = np.random.default_rng(F.width(dt))
    x = np.cumsum(rng.integers(-9, 10, 64)) + 40
    a = x.astype(dt)
    pages = [1, 2, 3, 4, 5, 6, 7, 8]
    paged = a[: sum(pages)]
    for order in range(1, 8):
        kw = dict(mode=1, delta=2, delta_order=order)
        cfg = G.make_config(enable_8_bit=True, **kw); ocfg = O.make_config(enable_8_bit=True, **kw)
        arrays = [np.ascontiguousarray(a[i: i + n]) for i, n in enumerate(pages)]
        files = [O.simple_compress(v, ocfg) for v in arrays]
        for v, f in zip(arrays, files):
            assert simple_compress_guarded(L, v, cfg) == f, (order, v.size)
            assert U.bits_equal(simple_decompress_guarded(L, f, dt, v.size), v), (order, v.size)
        chunks, _ = encode_call(arrays, cfg)
        assert chunks == [chunk_of(f) for f in files], order
        decode_call(chunks, arrays)
        want = O.wrapped_compress(paged, ocfg, max_pages=len(pages) + 1, exact_pages=pages)
        c = Call(L, [paged], cfg, [pages])
        G.check(c.encode())
        meta, pgs, ns = c.pieces()[0]
        assert (meta, pgs, ns) == (want[0], want[1], pages), order
        c.decode_and_compare()


@pytest.mark.parametrize("distinct", [3000, 65536])
def test_level_12_on_a_16_bit_type_at_2_to_the_20(L, distinct):
    """Level 12 asks for 2^12 unoptimised bins from n = 2^20 on (wrapped/chunk_compressor.rs:362-371).  A 16-bit type has at most 65 536
    distinct values -- sixteen per bin -- and with 3000 distinct values there are more bins asked for than values to put in them."""
    rng = np.random.default_rng(distinct)
    n = 1 << 20
    pool = rng.choice(65536, distinct, replace=False).astype(np.uint16)
    w = rng.random(distinct) ** 2
    for dt in (np.uint16, np.int16):
        a = pool[rng.choice(distinct, n, p=w / w.sum())].view(dt)
        for kw in (dict(mode=1, delta=1, level=12), dict(mode=1, delta=2, delta_order=1, level=12)):
            want = chunk_of(O.simple_compress(a, O.make_config(max_page_n=n, **kw)))
            chunks, _ = encode_call([a], G.make_config(**kw))
            assert chunks[0] == want, (np.dtype(dt).name, distinct, kw)
            decode_call([want], [a])
