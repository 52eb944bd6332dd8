"""-m gpu: Conv1 delta encode (PCO_GFX_CFG_CONV1, DeltaSpec::TryConv1; encode_conv1.hip) on every encode surface.

The fit's parameters are read back from the product's ChunkMeta (pco_gfx_chunk_meta_conv1) and checked against the known-answer table and the
CPU model (tests/conv1_model.py); the chunk bytes after the fit are checked against the oracle's test-only generator given the same parameters
(oracle_lib.test_encode, delta=TE_DELTA_CONV1), and both decoders must return the input bit for bit."""
import ctypes as C

import numpy as np
import pytest

import conv1_model as M
import gpu_util as U
import oracle_lib as O
from pcodec_amd import _lib as G

pytestmark = pytest.mark.gpu

CLASSIC, AUTO, FLOAT_MULT = G.MODE_CLASSIC, G.MODE_AUTO, G.MODE_TRY_FLOAT_MULT


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def cfg(order, mode=CLASSIC, level=8, conv1=True, mode_f64=0.0, max_page_n=0):
    return G.make_config(level=level, mode=mode, mode_f64=mode_f64, delta=G.DELTA_TRY_CONV1, delta_order=order, max_page_n=max_page_n,
                         enable_8_bit=True, conv1=conv1)


def compress(arrays, config, sync=True, order=None):
    """One pco_gfx_compress_chunks call (device buffers through torch; synchronous, or asynchronous with device results).
    Returns ([chunk bytes], [aux]) in the order of `arrays`; `order` permutes the tasks of the call."""
    import torch
    L = G.lib()
    arrays = [np.ascontiguousarray(a) for a in arrays]
    k = len(arrays)
    srcs = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in arrays]
    caps = [(L.pco_gfx_guarantee_chunk_size(a.size, G.DTYPE_BYTE[a.dtype.name]) + 64 + 15) // 16 * 16 for a in arrays]
    dsts = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in caps]
    idx = list(range(k)) if order is None else list(order)
    tasks = (G.EncodeTask * k)(*[G.EncodeTask(srcs[i].data_ptr(), arrays[i].size, dsts[i].data_ptr(), caps[i], G.DTYPE_BYTE[arrays[i].dtype.name], 0)
                                 for i in idx])
    if sync:
        res = (G.TaskResult * k)()
        G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(config), res, None, None))
        got = [(res[j].n_out, res[j].status, res[j].aux) for j in range(k)]
    else:
        d_res = torch.zeros(k * C.sizeof(G.TaskResult), dtype=torch.uint8, device="cuda")
        G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(config), None, C.c_void_p(d_res.data_ptr()), None))
        torch.cuda.synchronize()
        raw = d_res.cpu().numpy().tobytes()
        res = [G.TaskResult.from_buffer_copy(raw[j * C.sizeof(G.TaskResult):(j + 1) * C.sizeof(G.TaskResult)]) for j in range(k)]
        got = [(r.n_out, r.status, r.aux) for r in res]
    chunks, aux = [None] * k, [None] * k
    for j, i in enumerate(idx):
        n_out, status, a = got[j]
        assert status == G.ST_OK, (i, status)
        chunks[i] = bytes(dsts[i][:n_out].cpu().numpy()); aux[i] = a
    return chunks, aux


def decode(chunks, arrays):
    """pco_gfx_decompress_chunks over standalone chunks."""
    import torch
    L = G.lib()
    k = len(chunks)
    srcs = [torch.from_numpy(np.frombuffer(c + bytes(16), np.uint8).copy()).cuda() for c in chunks]
    outs = [torch.zeros(max(a.nbytes, 1), dtype=torch.uint8, device="cuda") for a in arrays]
    tasks = (G.DecodeTask * k)(*[G.DecodeTask(s.data_ptr(), len(c), o.data_ptr(), a.size, G.DTYPE_BYTE[a.dtype.name], 0)
                                 for s, c, o, a in zip(srcs, chunks, outs, arrays)])
    res = (G.TaskResult * k)()
    G.check(L.pco_gfx_decompress_chunks(k, tasks, res, None, None))
    return [o[: a.nbytes].cpu().numpy().view(a.dtype) for o, a in zip(outs, arrays)]


def params(chunk, dtype):
    """Conv1 (quantization, bias, weights) of a standalone chunk (dtype byte | 24-bit n - 1 | ChunkMeta ...), None for another delta."""
    return G.chunk_meta_conv1(chunk[4:], G.DTYPE_BYTE[np.dtype(dtype).name])


# ---------------------------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------------------------
def kat_config(kid, order):
    return cfg(order, mode=AUTO if (kid, order) == ("K1", 2) else CLASSIC, level=8)


@pytest.mark.parametrize("kid,gen,order,q,bias,weights", M.KAT, ids=[f"{k[0]}-o{k[2]}" for k in M.KAT])
def test_kat_c_abi(L, kid, gen, order, q, bias, weights):
    nums = gen()
    chunks, aux = compress([nums], kat_config(kid, order))
    got = params(chunks[0], nums.dtype)
    assert got is not None and aux[0] == 0
    assert (got[0], got[1]) == (q, bias)
    assert len(got[2]) == order
    if weights is not None:
        assert got[2] == weights
    assert U.bits_equal(decode(chunks, [nums])[0], nums)


@pytest.mark.parametrize("kid,gen,order", [(k[0], k[1], k[2]) for k in M.KAT if k[0] != "K4"], ids=[f"{k[0]}-o{k[2]}" for k in M.KAT if k[0] != "K4"])
def test_kat_python_standalone(L, kid, gen, order):
    import pcodec_amd as P
    nums = gen()
    mode = P.ModeSpec.auto() if (kid, order) == ("K1", 2) else P.ModeSpec.classic()
    conf = P.ChunkConfig(compression_level=8, mode_spec=mode, delta_spec=P.DeltaSpec.try_conv1(order), enable_8_bit=True, enable_conv1=True)
    f = P.standalone.simple_compress(nums, conf)
    chunk = compress([nums], kat_config(kid, order))[0][0]
    assert chunk in f                       # the same chunk, hence the same (quantization, bias, weights) as the known-answer table
    assert U.bits_equal(P.standalone.simple_decompress(f), nums)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the bytes after the fit, against the oracle's generator given the product's parameters
# ---------------------------------------------------------------------------------------------------------------------------------------
def smooth(n, dtype, seed, mode=CLASSIC):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    period = rng.integers(50, 900)
    wave = np.sin(2 * np.pi * i / period) + 0.3 * np.sin(2 * np.pi * i / (period * 0.37 + 3))
    dt = np.dtype(dtype)
    if dt.kind == "f":
        amp = 300.0 if dt.itemsize == 2 else 40000.0
        x = np.round(amp * wave + rng.integers(-5, 6, n))
        return (x * 0.01).astype(dt) if mode == FLOAT_MULT else x.astype(dt)
    info = np.iinfo(dt)
    span = min(float(info.max) - float(info.min), 2.0**31) * 0.4
    mid = (float(info.max) + float(info.min)) / 2
    x = mid + span * wave / 2.6 + rng.integers(-3, 4, n) * max(1.0, span / 4000)
    return np.clip(np.round(x), info.min, info.max).astype(dt)


MATRIX = [("int32", CLASSIC), ("uint32", CLASSIC), ("float32", CLASSIC), ("float32", FLOAT_MULT), ("int16", CLASSIC), ("uint16", CLASSIC),
          ("float16", CLASSIC), ("uint8", CLASSIC), ("int8", CLASSIC)]
ORDERS = [1, 2, 3, 7, 16, 32]
LEVELS = [0, 4, 8, 12]
SIZES = [33, 1000, 4097, 70001, 1 << 18]


@pytest.mark.parametrize("dtype,mode", MATRIX, ids=[f"{d}-{'fmult' if m == FLOAT_MULT else 'classic'}" for d, m in MATRIX])
@pytest.mark.parametrize("order", ORDERS)
def test_bytes_after_fit_match_oracle(L, dtype, mode, order):
    level = LEVELS[(ORDERS.index(order) + [d for d, _ in MATRIX].index(dtype)) % 4]
    sizes = [s for s in SIZES if s > order] + [order, max(order - 1, 1)]   # (n <= order: no config, NoOp)
    arrays = [smooth(n, dtype, seed=order * 1000003 + n, mode=mode) for n in sizes]
    mf = 0.01 if mode == FLOAT_MULT else 0.0
    chunks, aux = compress(arrays, cfg(order, mode=mode, level=level, mode_f64=mf))
    back = decode(chunks, arrays)
    n_conv = 0
    for a, ch, fb, b in zip(arrays, chunks, aux, back):
        assert U.bits_equal(b, a), (dtype, order, a.size)
        p = params(ch, a.dtype)
        if a.size <= order:
            assert p is None
        if fb & 1:
            continue
        if p is None:   # NoOp: the product's NoOp chunk
            assert ch == compress([a], G.make_config(level=level, mode=mode, mode_f64=mf, delta=G.DELTA_NOOP, enable_8_bit=True))[0][0]
            continue
        n_conv += 1
        q, bias, w = p
        f = O.test_encode(a, mode=mode, mode_f64=mf, delta=O.TE_DELTA_CONV1, quantization=q, bias=bias, weights=w, level=level)
        assert U.chunk_of_file(f, len(ch)) == ch, (dtype, order, level, a.size)
        assert U.bits_equal(O.simple_decompress(f, a.dtype), a)
    assert n_conv >= 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model as the expected value: a seeded sweep of smooth and noisy series
# ---------------------------------------------------------------------------------------------------------------------------------------
def sweep_cases(count=320, seed=11):
    rng = np.random.default_rng(seed)
    out = {}
    for c in range(count):
        dtype = ["int32", "uint32", "int16", "uint16", "uint8", "float32"][c % 6]
        order = int(rng.choice([1, 2, 3, 4, 5, 8, 12, 16, 24, 32]))
        n = int(rng.integers(order + 1, 30000)) if c % 5 else int(rng.integers(order + 1, order + 600))
        if c % 3 == 0:   # noisy
            dt = np.dtype(dtype)
            if dt.kind == "f":
                a = rng.standard_normal(n).astype(dt)
            else:
                info = np.iinfo(dt)
                lo = int(rng.integers(info.min, info.max // 2 + 1)); hi = int(rng.integers(lo + 1, info.max + 1)) + 1
                a = rng.integers(lo, hi, n).astype(dt)
        else:
            a = smooth(n, dtype, seed=int(rng.integers(1 << 30)))
        out.setdefault((dtype, order), []).append(a)
    return out


def test_model_sweep(L):
    checked = 0
    for (dtype, order), arrays in sorted(sweep_cases().items()):
        chunks, aux = compress(arrays, cfg(order, level=8))
        for a, ch, fb in zip(arrays, chunks, aux):
            lat, bits = M.latents_of(a)
            want = M.choose_config(lat, order, bits)
            if fb & 1:   # the fallback chunk writes no delta
                continue
            assert params(ch, a.dtype) == want, (dtype, order, a.size)
            checked += 1
        back = decode(chunks, arrays)
        assert all(U.bits_equal(b, a) for a, b in zip(arrays, back))
    assert checked >= 200


# ---------------------------------------------------------------------------------------------------------------------------------------
# the wrapped surface: the fit over the whole chunk, the state per page
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_wrapped_equal_pages(L):
    from test_gpu_wrapped_batched import decode_pages, wrapped_batch
    arrays = [smooth(n, dt, seed=n) for n, dt in ((100000, "int32"), (1 << 15, "uint16"), (50001, "int16"), (20000, "uint8"))]
    for order in (1, 3, 32):
        config = cfg(order, max_page_n=1 << 14)
        out, state = wrapped_batch(L, arrays, config)
        for a, (meta, pages, ns) in zip(arrays, out):
            lat, bits = M.latents_of(a)
            assert G.chunk_meta_conv1(meta, G.DTYPE_BYTE[a.dtype.name]) == M.choose_config(lat, order, bits)
            assert sum(ns) == a.size and len(pages) == L.pco_gfx_wrapped_n_pages(a.size, 1 << 14)
        code, res, back, _ = decode_pages(L, arrays, state)
        assert code == 0
        assert all(U.bits_equal(b, a) for a, b in zip(arrays, back))


def test_wrapped_exact_pages_and_short_pages(L):
    import pcodec_amd as P
    a = smooth(30000, "int32", seed=3)
    sizes = [5000, 7, 12000, 993, 12000]
    order = 5
    conf = P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_conv1(order), paging_spec=P.PagingSpec.exact_page_sizes(sizes),
                         enable_conv1=True)
    fc = P.wrapped.FileCompressor()
    cc = fc.chunk_compressor(a, conf)
    meta = cc.write_meta()
    lat, bits = M.latents_of(a)
    assert G.chunk_meta_conv1(meta, G.DTYPE_BYTE["int32"]) == M.choose_config(lat, order, bits)   # the fit is over the whole chunk
    pages = [cc.write_page(i) for i in range(len(sizes))]
    fd = P.wrapped.FileDecompressor.new(fc.write_header())[0]
    cd, _ = fd.chunk_decompressor(meta, "I32")
    at = 0
    for pg, n in zip(pages, sizes):
        dst = np.empty(n, np.int32)
        cd.read_page_into(pg, n, dst)
        assert U.bits_equal(dst, a[at: at + n])
        at += n
    # a page shorter than the order: the reference panics (conv1.rs:428); INVALID_ARGUMENT here
    bad = P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_conv1(8), paging_spec=P.PagingSpec.exact_page_sizes([29000, 7, 993]),
                        enable_conv1=True)
    with pytest.raises(G.PcoGfxError) as e:
        fc.chunk_compressor(a, bad)
    assert e.value.status == G.ST_INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------------------------------------------------------
# consistency
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_identical_async_permuted(L):
    base = [smooth(n, dt, seed=n) for n, dt in ((1 << 18, "int32"), (77777, "int16"), (5000, "uint8"), (1 << 16, "float32"))]
    arrays = base + [base[0].copy(), base[1].copy()]
    config = cfg(8, level=8)
    sync, _ = compress(arrays, config)
    assert sync[4] == sync[0] and sync[5] == sync[1]
    asyn, _ = compress(arrays, config, sync=False)
    assert asyn == sync
    perm = [3, 5, 0, 2, 4, 1]
    assert compress(arrays, config, order=perm)[0] == sync
    assert compress([arrays[2]], config)[0][0] == sync[2]


def test_simple_compress_surfaces(L):
    a = smooth(300000, "int16", seed=9)
    config = cfg(4, max_page_n=1 << 16)
    f = U.gpu_simple_compress(a, config)
    assert U.bits_equal(U.gpu_simple_decompress(f, a.dtype, a.size), a)
    # _exact (pco_gfx_simple_compress_into_exact): one chunk per entry, each with its own fit
    import pcodec_amd as P
    sizes = [100000, 150000, 50000]
    conf = P.ChunkConfig(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_conv1(4), paging_spec=P.PagingSpec.exact_page_sizes(sizes),
                         enable_conv1=True)
    f2 = P.standalone.simple_compress(a, conf)
    assert U.bits_equal(U.gpu_simple_decompress(f2, a.dtype, a.size), a)
    at = 0
    for s in sizes:
        ch = compress([a[at: at + s]], config)[0][0]
        assert ch in f2
        at += s


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def _status_of(arr, config):
    L = G.lib()
    with pytest.raises(G.PcoGfxError):
        compress([arr], config)
    return L.pco_gfx_last_status()


def test_refusals(L):
    a32 = smooth(5000, "int32", seed=1)
    assert _status_of(a32, cfg(33)) == G.ST_INVALID_ARGUMENT
    for dt in ("int64", "uint64", "float64"):
        assert _status_of(np.arange(5000).astype(dt), cfg(2)) == G.ST_INVALID_ARGUMENT, dt
    dict_cfg = G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_NOOP, conv1=True)
    assert _status_of(a32, dict_cfg) == G.ST_UNSUPPORTED
    dict_conv = G.make_config(mode=G.MODE_TRY_DICT, delta=G.DELTA_TRY_CONV1, delta_order=2, conv1=True)
    assert _status_of(a32, dict_conv) == G.ST_UNSUPPORTED
    # without the flag Conv1 stays refused, as before
    assert _status_of(a32, cfg(2, conv1=False)) == G.ST_UNSUPPORTED
    # TryConv1(0) is NoOp
    assert compress([a32], cfg(0))[0][0] == compress([a32], G.make_config(mode=CLASSIC, delta=G.DELTA_NOOP))[0][0]
