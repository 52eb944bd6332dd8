"""-m gpu: Dict mode encode (PCO_GFX_CFG_DICT, ModeSpec::TryDict; encode_dict.hip) on the encode surfaces.

The dictionary is read back from the product's ChunkMeta (pco_gfx_chunk_meta_dict) and checked against a numpy model (distinct ordered
latents, most frequent first, ties by ascending ordered latent).  For the bytes, the input is relabelled: y = rank of x in the product's
dictionary, in the unsigned type of the same width.  The oracle's test-only generator writes y's dictionary in value order, i.e. the identity,
so its chunk for y must equal the product's chunk for x once the dtype byte and the dictionary payload are patched.  Both decoders must return
every input bit for bit."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as U
import oracle_lib as O
from pcodec_amd import _lib as G

pytestmark = pytest.mark.gpu

UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TE = {"noop": O.TE_DELTA_NONE, "cons": O.TE_DELTA_CONSECUTIVE, "lookback": O.TE_DELTA_LOOKBACK}


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def cfg(delta=G.DELTA_NOOP, order=0, level=8, dict_on=True, max_page_n=0):
    return G.make_config(level=level, mode=G.MODE_TRY_DICT, delta=delta, delta_order=order, max_page_n=max_page_n, enable_8_bit=True, dict=dict_on)


def ordered_latents(a):
    """to_latent_ordered as unsigned integers of the number's width (floats by bit pattern)."""
    a = np.ascontiguousarray(a)
    w = a.dtype.itemsize
    u = a.view(UNSIGNED[w])
    top = UNSIGNED[w](1) << UNSIGNED[w](8 * w - 1)
    if a.dtype.kind == "u":
        return u.copy()
    if a.dtype.kind == "i":
        return u ^ top
    return np.where(u & top, ~u, u | top).astype(UNSIGNED[w])


def model_dict(a):
    keys, counts = np.unique(ordered_latents(a), return_counts=True)
    order = np.lexsort((keys, -counts.astype(np.int64)))
    return keys[order]


def dict_of_chunk(chunk, dtype):
    """The dictionary of a standalone chunk (dtype byte + 24-bit n - 1 in front of its ChunkMeta), or None for a non-Dict chunk."""
    return G.chunk_meta_dict(chunk[4:], G.DTYPE_BYTE[np.dtype(dtype).name])


def relabel(a, d):
    lat = ordered_latents(a)
    pos = {int(v): i for i, v in enumerate(d)}
    return np.array([pos[int(v)] for v in lat], dtype=UNSIGNED[a.dtype.itemsize])


def patched_oracle_chunk(a, d, gpu_chunk, **te):
    """The oracle's chunk for the relabelled input, with the product's dtype byte and dictionary."""
    y = relabel(a, d)
    f = O.test_encode(y, mode=O.MODE_TRY_DICT, **te)
    ref = bytearray(U.chunk_of_file(f, len(gpu_chunk)))
    w = a.dtype.itemsize
    ref[0] = G.DTYPE_BYTE[a.dtype.name]
    ref[8:8 + len(d) * w] = np.ascontiguousarray(d).tobytes()
    return bytes(ref)


def delta_of_dict_chunk(chunk, k, w):
    """(kind, order or window_n_log) of the delta encoding behind a Dict chunk's dictionary."""
    rest = int.from_bytes(chunk[8 + k * w:8 + k * w + 8], "little")
    kind = rest & 0xF
    if kind == 1:
        return kind, (rest >> 4) & 0x7
    if kind == 2:
        return kind, ((rest >> 4) & 0x1F) + 1
    return kind, 0


def fallback_chunk(a):
    """fallback_chunk_compressor (wrapped/chunk_compressor.rs:396-438) as a standalone chunk: dtype byte, n - 1 in 24 bits, ChunkMeta
    Classic / NoOp / one bin {weight 1, lower 0, offset bits = the width}, then one page of the raw ordered latents."""
    bits = a.dtype.itemsize * 8
    fields = [(G.DTYPE_BYTE[a.dtype.name], 8), (a.size - 1, 24), (0, 4), (0, 4), (0, 4), (1, 15), (0, bits), (bits, OFFSET_BITS_BITS[bits])]
    acc = pos = 0
    for v, w in fields:
        acc |= int(v) << pos; pos += w
    pos = (pos + 7) // 8 * 8
    meta = acc.to_bytes(pos // 8, "little")
    return meta + ordered_latents(a).astype(UNSIGNED[a.dtype.itemsize]).tobytes()


OFFSET_BITS_BITS = {8: 4, 16: 5, 32: 6, 64: 7}
DELTA_MAX_BITS = 4 + 5 + 5 + 64 + 32 * 32   # DeltaEncoding::MAX_BIT_SIZE


def dict_margin(a, level=8):
    """baseline - worst case (bytes) of the Dict/NoOp chunk of `a`, as should_fallback (wrapped/chunk_compressor.rs:502-541) forms it, from
    the oracle's bins for the index latents: a Dict chunk when >= 0, the fallback chunk when < 0."""
    d = model_dict(a)
    y = relabel(a, d).astype(np.uint32)
    info, bins, _ = O.chunk_plan(y, O.make_config(level=level, mode=O.MODE_CLASSIC, delta=O.DELTA_NOOP))
    b = bins[1].astype(np.int64)
    asl = int(info.ans_size_log[1])
    counts = np.bincount(np.searchsorted(b[:, 1], y.astype(np.int64), side="right") - 1, minlength=len(b))
    worst_bits = 7 + sum(int(c) * (int(ob) + asl - (int(w).bit_length() - 1)) for c, (w, _, ob) in zip(counts, b))
    bits = a.dtype.itemsize * 8
    meta_bits = 4 + 25 + 7 + len(d) * bits + DELTA_MAX_BITS + 4 + 15 + len(b) * (asl + 32 + OFFSET_BITS_BITS[32])
    worst = (meta_bits + 7) // 8 + (4 * asl + 7) // 8 + (worst_bits + 7) // 8
    baseline = (4 + DELTA_MAX_BITS + 4 + 15 + bits + OFFSET_BITS_BITS[bits] + 7) // 8 + (a.size * bits + 7) // 8
    return baseline - worst


def datasets():
    rng = np.random.default_rng(7)
    out = []
    for dt in ("uint8", "int8", "uint16", "int16", "float16", "uint32", "int32", "float32", "uint64", "int64", "float64"):
        w = np.dtype(dt).itemsize
        pool = rng.integers(0, 1 << min(8 * w, 62), 300, dtype=np.uint64).astype(UNSIGNED[w]).view(dt)
        pool = pool[~np.isnan(pool)] if pool.dtype.kind == "f" else pool
        out.append((dt + "_zipf", pool[np.minimum(rng.zipf(1.3, 5000), len(pool)) - 1]))
        out.append((dt + "_k1", np.repeat(pool[:1], 777)))
        out.append((dt + "_k2_tie", np.tile(pool[:2], 400)))
        out.append((dt + "_ties", np.tile(pool[:50], 40)[rng.permutation(2000)]))
    for dt in ("float16", "float32", "float64"):
        f = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -1.5], dtype=dt)
        w = f.dtype.itemsize
        nan2 = (f[4:5].view(UNSIGNED[w]) | UNSIGNED[w](1)).view(dt)
        out.append((dt + "_specials", np.concatenate([f, nan2])[rng.integers(0, 8, 3000)]))
    ids = rng.integers(0, 1 << 63, 1 << 17, dtype=np.uint64)
    for k in (4096, 4097):   # on each side of the LDS table's capacity
        out.append((f"u64_k{k}", ids[:k][rng.integers(0, k, 40000)]))
    out.append(("u64_k70000", np.concatenate([ids[:70000], ids[:70000][rng.integers(0, 70000, (1 << 18) - 70000)]])))
    out.append(("u32_k70000", (ids[:70000] >> np.uint64(32)).astype(np.uint32)[rng.integers(0, 70000, 1 << 18)]))
    return out


DATA = datasets()


@pytest.mark.parametrize("name,a", DATA, ids=[d[0] for d in DATA])
def test_dictionary_matches_model(L, name, a):
    chunks, back = U.gpu_batched([a], cfg())
    d = dict_of_chunk(chunks[0], a.dtype)
    assert d is not None, name
    np.testing.assert_array_equal(d, model_dict(a))
    assert U.bits_equal(back[0], a)
    assert chunks[0] == patched_oracle_chunk(a, d, chunks[0])
    f = U.gpu_simple_compress(a, cfg())
    assert U.bits_equal(O.simple_decompress(f, a.dtype, a.size + 16), a)


def test_one_big_chunk(L):
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 1 << 63, 1000, dtype=np.uint64)
    a = ids[np.minimum(rng.zipf(1.2, 1 << 22), 1000) - 1]
    chunks, back = U.gpu_batched([a], cfg(G.DELTA_TRY_CONSECUTIVE, 1))
    np.testing.assert_array_equal(dict_of_chunk(chunks[0], a.dtype), model_dict(a))
    assert U.bits_equal(back[0], a)


@pytest.mark.parametrize("n", [1, 257, 1 << 18])
@pytest.mark.parametrize("spec", [("noop", 0, 8), ("noop", 0, 0), ("noop", 0, 12)] + [("cons", o, 8) for o in range(1, 8)] + [("lookback", 0, 8)])
def test_bytes_match_oracle(L, n, spec):
    kind, order, level = spec
    rng = np.random.default_rng(n + order)
    for dt in ("uint64", "float32"):
        pool = rng.integers(0, 1 << 30, 200).astype(dt)
        a = pool[rng.integers(0, 200, n)]
        delta = {"noop": G.DELTA_NOOP, "cons": G.DELTA_TRY_CONSECUTIVE, "lookback": G.DELTA_TRY_LOOKBACK}[kind]
        chunks, back = U.gpu_batched([a], cfg(delta, order, level))
        assert U.bits_equal(back[0], a)
        d = dict_of_chunk(chunks[0], a.dtype)
        if d is None:   # (a tiny chunk falls back: the fallback chunk of its numbers)
            assert chunks[0] == fallback_chunk(a), (dt, n, spec)
            continue
        te = dict(delta=TE[kind], order=order, level=level)
        if kind == "lookback":
            dk, win = delta_of_dict_chunk(chunks[0], len(d), a.dtype.itemsize)
            assert dk == 2
            te.update(window_n_log=win, state_n_log=0, lookback_seed=0)
        assert chunks[0] == patched_oracle_chunk(a, d, chunks[0], **te), (dt, n, spec)


def test_auto_delta(L):
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 1 << 62, 3000, dtype=np.uint64)
    walk = np.cumsum(rng.integers(-3, 4, 1 << 16)) % 3000
    for a in (pool[walk], pool[rng.integers(0, 3000, 1 << 16)]):
        chunks, back = U.gpu_batched([a], cfg(G.DELTA_AUTO))
        assert U.bits_equal(back[0], a)
        d = dict_of_chunk(chunks[0], a.dtype)
        got = delta_of_dict_chunk(chunks[0], len(d), 8)
        y = relabel(a, d).astype(np.uint32)
        ref = O.simple_compress(y, O.make_config(mode=O.MODE_CLASSIC, delta=O.DELTA_AUTO))
        hdr = np.zeros(64, np.uint8)
        h = G.lib().pco_gfx_write_standalone_header(hdr.ctypes.data_as(C.c_void_p), C.c_size_t(64), C.c_uint64(y.size), C.c_ubyte(0))
        # the oracle's Classic u32 chunk: dtype byte, 24-bit n - 1, then its ChunkMeta: 4 bits of mode, the delta encoding
        v = int.from_bytes(ref[h + 4:h + 12], "little") >> 4
        kind = v & 0xF
        want = (kind, (v >> 4) & 0x7) if kind == 1 else ((kind, ((v >> 4) & 0x1F) + 1) if kind == 2 else (kind, 0))
        assert got == want
        te = dict(delta=want[0], order=want[1] if want[0] == 1 else 0)
        if want[0] == 2:
            te.update(window_n_log=want[1], state_n_log=0, lookback_seed=0)
        assert chunks[0] == patched_oracle_chunk(a, d, chunks[0], **te)


def test_fallback(L):
    rng = np.random.default_rng(13)
    for dt in ("uint64", "float64"):
        a = rng.integers(0, 1 << 63, 5000, dtype=np.uint64).view(dt)
        a = a[~np.isnan(a)] if a.dtype.kind == "f" else a
        chunks, back = U.gpu_batched([a], cfg(G.DELTA_TRY_CONSECUTIVE, 1))
        assert dict_of_chunk(chunks[0], a.dtype) is None
        ref = O.simple_compress(a, O.make_config(mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=1))
        assert chunks[0] == U.chunk_of_file(ref, len(chunks[0]))
        assert U.bits_equal(back[0], a)


def test_fallback_chunk_model_is_the_oracles(L):
    a = np.random.default_rng(23).integers(0, 1 << 63, 3000, dtype=np.uint64)
    ref = O.simple_compress(a, O.make_config(mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=1))
    assert fallback_chunk(a) == U.chunk_of_file(ref, len(fallback_chunk(a)))


@pytest.mark.parametrize("dt", ["uint64", "uint16"])
def test_fallback_threshold(L, dt):
    """One chunk on each side of should_fallback's threshold: m distinct numbers once each, the rest copies of one more.  The threshold is
    found by bisection on the margin the oracle's bins give; the chunk just below it is Dict (the oracle's bytes, patched), the one just
    above it the fallback chunk."""
    n = 3000
    rng = np.random.default_rng(29)
    ids = rng.choice(1 << (16 if dt == "uint16" else 62), n, replace=False).astype(dt)

    def make(m):
        return np.concatenate([ids[:m], np.repeat(ids[m:m + 1], n - m)])[np.random.default_rng(m).permutation(n)]
    lo, hi = 1, n - 1
    assert dict_margin(make(lo)) >= 0 and dict_margin(make(hi)) < 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if dict_margin(make(mid)) >= 0:
            lo = mid
        else:
            hi = mid
    a_dict, a_fb = make(lo), make(hi)
    chunks, back = U.gpu_batched([a_dict, a_fb], cfg())
    d = dict_of_chunk(chunks[0], a_dict.dtype)
    assert d is not None, (dt, lo, dict_margin(a_dict))
    assert chunks[0] == patched_oracle_chunk(a_dict, d, chunks[0])
    assert dict_of_chunk(chunks[1], a_fb.dtype) is None, (dt, hi, dict_margin(a_fb))
    assert chunks[1] == fallback_chunk(a_fb)
    assert U.bits_equal(back[0], a_dict) and U.bits_equal(back[1], a_fb)


def test_wrapped_batched_chunks(L):
    """pco_gfx_compress_wrapped_chunks with Dict chunks of several widths: each ChunkMeta holds its dictionary within the capacity, the page
    offsets follow pco_gfx_wrapped_chunk_cap's layout, and every page decodes."""
    from test_gpu_wrapped_batched import decode_pages, wrapped_batch
    rng = np.random.default_rng(31)
    arrays = []
    for dt, k in (("uint64", 5000), ("int32", 300), ("float16", 900), ("uint8", 40), ("float64", 70000)):
        pool = rng.integers(0, 1 << min(8 * np.dtype(dt).itemsize - 2, 62), k, dtype=np.uint64).astype(UNSIGNED[np.dtype(dt).itemsize]).view(dt)
        arrays.append(pool[rng.integers(0, k, 150000)])
    c = cfg(G.DELTA_TRY_CONSECUTIVE, 1, max_page_n=40000)
    out, state = wrapped_batch(L, arrays, c)
    infos = state[1]
    at = 0
    for a, (meta, pages, ns) in zip(arrays, out):
        w = a.dtype.itemsize
        meta_cap = ((16 << 10) + (4 + a.size * w + 15) // 16 * 16)
        assert len(meta) <= meta_cap
        assert infos[at + 1].offset == meta_cap
        np.testing.assert_array_equal(G.chunk_meta_dict(meta, G.DTYPE_BYTE[a.dtype.name]), model_dict(a))
        assert sum(ns) == a.size and len(pages) == len(ns)
        at += 1 + len(ns)
    code, res, back, _ = decode_pages(L, arrays, state)
    G.check(code)
    for a, b in zip(arrays, back):
        assert U.bits_equal(b, a)


def compress_chunks(arrays, config, sync=True, order=None):
    import torch
    arrays = [np.ascontiguousarray(a) for a in arrays]
    k = len(arrays)
    srcs = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in arrays]
    caps = [(G.lib().pco_gfx_guarantee_chunk_size(a.size, G.DTYPE_BYTE[a.dtype.name]) + 64 + 15) // 16 * 16 for a in arrays]
    dsts = [torch.full((c + 64,), 0xA5, dtype=torch.uint8, device="cuda") for c in caps]
    idx = list(range(k)) if order is None else list(order)
    tasks = (G.EncodeTask * k)(*[G.EncodeTask(srcs[i].data_ptr() + 0, arrays[i].size, dsts[i].data_ptr() + 8, caps[i], G.DTYPE_BYTE[arrays[i].dtype.name], 0)
                                 for i in idx])
    if sync:
        res = (G.TaskResult * k)()
        G.check(G.lib().pco_gfx_compress_chunks(k, tasks, C.byref(config), res, None, None))
        got = [(res[j].n_out, res[j].status) for j in range(k)]
    else:
        d_res = torch.zeros(k * C.sizeof(G.TaskResult), dtype=torch.uint8, device="cuda")
        G.check(G.lib().pco_gfx_compress_chunks(k, tasks, C.byref(config), None, C.c_void_p(d_res.data_ptr()), None))
        torch.cuda.synchronize()
        raw = d_res.cpu().numpy().tobytes()
        rs = [G.TaskResult.from_buffer_copy(raw[j * C.sizeof(G.TaskResult):(j + 1) * C.sizeof(G.TaskResult)]) for j in range(k)]
        got = [(r.n_out, r.status) for r in rs]
    out = [None] * k
    for j, i in enumerate(idx):
        n_out, status = got[j]
        assert status == G.ST_OK
        host = dsts[i].cpu().numpy()
        assert (host[:8] == 0xA5).all() and (host[8 + caps[i]:] == 0xA5).all(), "bytes outside dst were written"
        out[i] = host[8:8 + n_out].tobytes()
    return out


def test_surfaces_agree(L):
    rng = np.random.default_rng(17)
    arrays = []
    for j, dt in enumerate(("uint64", "int32", "float32", "uint16", "float64", "uint8")):
        pool = rng.integers(0, 1 << 14, 40 + 500 * j).astype(dt)
        arrays.append(pool[rng.integers(0, len(pool), 3000 + 7000 * j)])
    arrays.append(rng.integers(0, 1 << 63, 1 << 16, dtype=np.uint64)[rng.integers(0, 1 << 16, 1 << 17)])   # (an HBM-table chunk)
    c = cfg(G.DELTA_TRY_CONSECUTIVE, 1)
    base = compress_chunks(arrays, c)
    assert compress_chunks(arrays, c, sync=False, order=list(reversed(range(len(arrays))))) == base
    assert compress_chunks(arrays, c, order=[3, 1, 6, 0, 5, 2, 4]) == base
    single = [compress_chunks([a], c)[0] for a in arrays]
    assert single == base
    dicts = [dict_of_chunk(ch, a.dtype) for a, ch in zip(arrays, base)]
    assert dicts[-1] is not None and dicts[-2] is None   # (256 equally frequent u8 values: the fallback chunk is smaller)
    for a, d in zip(arrays, dicts):
        if d is not None:
            np.testing.assert_array_equal(d, model_dict(a))


def test_python_surfaces(L):
    from pcodec_amd import ChunkConfig, ModeSpec, PagingSpec, standalone
    from pcodec_amd.wrapped import FileCompressor, FileDecompressor
    rng = np.random.default_rng(19)
    pool = rng.integers(0, 1 << 62, 900, dtype=np.uint64)
    a = pool[rng.integers(0, 900, 70000)]
    conf = ChunkConfig(mode_spec=ModeSpec.try_dict(), enable_dict=True)
    f = standalone.simple_compress(a, conf)
    np.testing.assert_array_equal(standalone.simple_decompress(f), a)
    np.testing.assert_array_equal(O.simple_decompress(f, a.dtype, a.size + 16), a)
    for paging in (PagingSpec.equal_pages_up_to(30000), PagingSpec.exact_page_sizes([10000, 50000, 10000])):
        conf = ChunkConfig(mode_spec=ModeSpec.try_dict(), enable_dict=True, paging_spec=paging)
        fc = FileCompressor()
        cc = fc.chunk_compressor(a, conf)
        meta = cc.write_meta()
        assert len(meta) == G.lib().pco_chunk_compressor_meta_size(cc._h)
        d = G.chunk_meta_dict(meta, G.DTYPE_BYTE["uint64"])
        np.testing.assert_array_equal(d, model_dict(a))
        pages = [cc.write_page(i) for i in range(len(cc.n_per_page()))]
        fd, _ = FileDecompressor.new(fc.write_header())
        cd, used = fd.chunk_decompressor(meta, "U64")
        got = []
        for pg, pn in zip(pages, cc.n_per_page()):
            dst = np.zeros(pn, np.uint64)
            cd.read_page_into(pg, pn, dst)
            got.append(dst)
        np.testing.assert_array_equal(np.concatenate(got), a)


def test_refusals(L):
    a = np.arange(1000, dtype=np.uint32) % 7
    def status(c, arr=a):
        try:
            U.gpu_batched([arr], c)
            return G.ST_OK
        except G.PcoGfxError as e:
            return e.status
    assert status(G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONV1, delta_order=2, conv1=True, dict=True)) == G.ST_UNSUPPORTED
    assert status(G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, dict=True), a.astype(np.uint8)) == G.ST_INVALID_ARGUMENT
    assert status(G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, conv1=True)) == G.ST_UNSUPPORTED
    assert status(G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP)) == G.ST_UNSUPPORTED
    assert status(cfg()) == G.ST_OK
