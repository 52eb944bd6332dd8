"""-m gpu: the segmented encode walk at its meeting, redo and segment edges (the rows of walkseg_edges_util.py; what each row exercises is
checked on the CPU by test_walkseg_model.py against walkseg_model.py).

One synchronous pco_gfx_compress_chunks call per config over the rows of that config (test_gpu_width_paths.encode_call): enc_walkseg_kernel is
among the profiled kernels, every chunk equals the oracle's byte for byte, every chunk decodes bit for bit.  The page's bytes hold every word
of the walk and its four final states; they are the observable, nothing is read out of the kernel.  Then the same rows

  * twice in one call and once more in a shuffled order (copies are byte-identical wherever they sit);
  * through the asynchronous form with device results, and one by one through simple_compress;
  * as pages of wrapped chunks (PagingSpec::Exact and EqualPagesUpTo through pco_gfx_compress_wrapped_chunks_ex, Exact through
    pco_gfx_simple_compress_into_exact, max_page_n through simple_compress), decoded page by page;
  * in one call that mixes the numbers of rows of every class and level with short chunks that the unsegmented walkers keep.

The symbol-source rows (class S) are pinned by their bytes only: the profile names one kernel whichever way the walker's symbols reach it
("finds", "all_lds", "stages" are branches inside enc_walkseg_kernel), so that a row took the source it was built for rests on
walkseg_model.source and the CPU suite, not on anything the device reports.

Measured on an MI355X: see DESIGN.md section 2 (the segmented walk at its edges)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _imports():
    global torch, G, U, O, E, M, encode_call, decode_call
    import torch
    import gpu_util as U
    import oracle_lib as O
    import walkseg_edges_util as E
    import walkseg_model as M
    from pcodec_amd import _lib as G
    from test_gpu_width_paths import decode_call, encode_call


@pytest.fixture(scope="module")
def L():
    _imports()
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def _configs():
    import walkseg_edges_util as E_
    return list(E_.configs().items())


def _cfg_id(key):
    return "-".join(f"{k}{v}" for k, v in key if (k, v) not in (("mode", 1), ("delta", 1)))


CONFIGS = _configs()
IDS = [_cfg_id(k) for k, _ in CONFIGS]


def compare(names, chunks, what):
    bad = []
    for i, (n, c) in enumerate(zip(names, chunks)):
        want = E.oracle_chunk(n)
        if c != want:
            a = np.frombuffer(c[:min(len(c), len(want))], np.uint8); b = np.frombuffer(want[:len(a)], np.uint8)
            d = np.flatnonzero(a != b)
            bad.append(f"{what}: {n} (chunk {i}): {len(c)} bytes for {len(want)}, first difference at byte {int(d[0]) if d.size else min(len(c), len(want))}, {d.size} bytes differ")
    assert not bad, "\n" + "\n".join(bad[:30]) + f"\n({len(bad)} in all)"


def long_names(names):
    return [n for n in names if n not in E.SHORT]


@pytest.mark.parametrize("key,names", CONFIGS, ids=IDS)
def test_rows_give_the_oracles_bytes_and_decode(L, key, names):
    """One call per config: the segmented kernel ran, every chunk == the oracle's, every chunk decodes."""
    assert 0 < len(names) <= 64 and 3 * len(names) <= M.kWsMaxItems
    arrays = [E.numbers(n) for n in names]
    chunks, kernels = encode_call(arrays, G.make_config(enable_8_bit=True, **dict(key)))
    if long_names(names):
        assert "enc_walkseg_kernel" in kernels, kernels
    compare(names, chunks, "one call")
    decode_call(chunks, arrays)


@pytest.mark.parametrize("key,names", CONFIGS, ids=IDS)
def test_copies_agree_wherever_they_sit(L, key, names):
    """Every row twice in one call (positions i and k + i; every odd destination 8 bytes past a 16-byte boundary), then once in a shuffled
    order: all copies byte-identical, and equal to the oracle's."""
    cfg = G.make_config(enable_8_bit=True, **dict(key))
    twice = list(names) + list(names)
    chunks, kernels = encode_call([E.numbers(n) for n in twice], cfg, misalign=True)
    compare(twice, chunks, "two positions")
    assert chunks[:len(names)] == chunks[len(names):]
    order = [names[i] for i in np.random.default_rng(len(names)).permutation(len(names))]
    shuffled, _ = encode_call([E.numbers(n) for n in order], cfg)
    compare(order, shuffled, "shuffled")


def test_the_asynchronous_form_with_device_results(L):
    """pco_gfx_compress_chunks(results = NULL, d_results) on a caller stream, per config: sizes and statuses from the device, bytes == the oracle's."""
    s = torch.cuda.Stream()
    for key, names in CONFIGS:
        st = U.Staged(L, [E.numbers(n) for n in names])
        t = U.pinned(st.enc_tasks())
        cfg = G.make_config(enable_8_bit=True, **dict(key))
        G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(t), C.byref(cfg), None, st.d_res.data_ptr(), C.c_void_p(s.cuda_stream)))
        s.synchronize()
        res = st.results()
        assert (res["status"] == 0).all(), (key, res["status"])
        compare(names, st.slot_bytes(res["n_out"]), f"asynchronous form {_cfg_id(key)}")


def test_rows_through_simple_compress(L):
    """Each row as a file of its own: one long page, one call (the ordinary case the kernel serves)."""
    for key, names in CONFIGS:
        for n in long_names(names):
            a = E.numbers(n)
            got = U.gpu_simple_compress(a, G.make_config(enable_8_bit=True, **dict(key)))
            assert got == E.oracle_file(n), (n, len(got), len(E.oracle_file(n)))
    a = E.paged_numbers([40000, 40000, 40000])
    n, mp = E.SIMPLE_MAX_PAGE_N
    assert a.size == n
    got = U.gpu_simple_compress(a, G.make_config(enable_8_bit=True, max_page_n=mp, **E.PAGED_KW))
    assert got == O.simple_compress(a, O.make_config(max_page_n=mp, **E.PAGED_KW))
    assert U.bits_equal(U.gpu_simple_decompress(got, a.dtype, a.size), a)


def test_pages_of_wrapped_chunks(L):
    """One pco_gfx_compress_wrapped_chunks_ex call: two chunks under PagingSpec::Exact ([16 384, 16 383, 20 000, 300] and [20 736, 16 385]: long
    pages beside pages one latent short of the segmented walk, and a tail of 300) and two under EqualPagesUpTo 16 384 (40 000 numbers: three
    pages that stay with the unsegmented walkers; 49 152: three pages of 16 384).  The table is the chunk's; every page's top segment starts
    from T.  ChunkMeta and every page == the oracle's; every page decodes on its own."""
    from test_gpu_wrapped_writer import Call
    cases = [E.paged_case(k) for k in E.PAGED_KEYS]
    cfg = G.make_config(enable_8_bit=True, max_page_n=16384, **E.PAGED_KW)
    lists = [list(pages) if key[0] == "exact" else None for key, (_, pages, _) in zip(E.PAGED_KEYS, cases)]
    c = Call(L, [a for a, _, _ in cases], cfg, lists)
    L.pco_gfx_profile_begin()
    G.check(c.encode())
    assert "enc_walkseg_kernel" in U.profile_names(L)
    for key, (a, pages, want), got in zip(E.PAGED_KEYS, cases, c.pieces()):
        assert got[2] == want[2] == pages, key
        assert got[0] == want[0], f"{key}: ChunkMeta differs from the oracle's"
        for p, (x, y) in enumerate(zip(got[1], want[1])):
            assert x == y, f"{key}: page {p} ({pages[p]} numbers) differs from the oracle's"
    c.decode_and_compare()


def test_exact_pages_through_simple_compress(L):
    """pco_gfx_simple_compress_into_exact: one standalone chunk per entry, against the oracle's simple_compress under PagingSpec::Exact."""
    for sizes in E.EXACT_LISTS:
        a = E.paged_numbers(sizes)
        cfg = G.make_config(enable_8_bit=True, **E.PAGED_KW)
        want = O.simple_compress_exact(a, O.make_config(**E.PAGED_KW), sizes)
        cap = len(want) + (1 << 16)
        dst = np.zeros(cap, np.uint8); w = C.c_size_t(0)
        arr = (C.c_size_t * len(sizes))(*sizes)
        G.check(L.pco_gfx_simple_compress_into_exact(a.ctypes.data_as(C.c_void_p), C.c_size_t(a.size), C.c_ubyte(G.DTYPE_BYTE[a.dtype.name]), C.byref(cfg), C.c_int(0), arr,
                                                     C.c_size_t(len(sizes)), dst.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(w)))
        got = bytes(dst[: w.value])
        assert got == want, (sizes, len(got), len(want))
        assert U.bits_equal(U.gpu_simple_decompress(got, a.dtype, a.size), a)


def test_one_call_mixes_every_class_with_short_chunks(L):
    """The numbers of two rows of every class (every level among them) under ONE config, beside chunks of 1 .. 16 383 numbers that stay with
    the unsegmented walkers: every chunk == the oracle's under that config, every chunk decodes."""
    rows = E.ROWS()
    picked = []
    for cls in "GTMRASOVB":
        of = [r for r in rows if r.cls == cls and r.n_lat <= 1 << 17]
        picked += [of[0], of[-1]]
    picked.append(next(r for r in rows if r.kw["level"] == 2))
    assert {r.kw["level"] for r in picked} == {8, 6, 4, 2}
    rng = np.random.default_rng(3)
    arrays = []
    for i, r in enumerate(picked):
        arrays.append(E.numbers(r.name))
        n = (1, 255, 256, 257, 4097, 16383)[i % 6]
        arrays.append(np.where(rng.random(n) < 0.01, 77, 5).astype(np.uint32))
    kw = dict(level=8, mode=1, delta=1)
    chunks, kernels = encode_call(arrays, G.make_config(enable_8_bit=True, **kw), misalign=True)
    assert "enc_walkseg_kernel" in kernels, kernels
    for i, (a, c) in enumerate(zip(arrays, chunks)):
        assert c == U.oracle_chunk(a, O.make_config(**kw)), (i, a.size)
    decode_call(chunks, arrays)
