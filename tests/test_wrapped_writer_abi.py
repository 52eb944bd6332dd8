"""CPU-side checks of the batched wrapped writer (include/pco_gfx.h section 4c): the symbols are exported, PcoGfxWrappedTask keeps its layout,
pco_gfx_wrapped_chunk_cap_exact agrees with pco_gfx_wrapped_chunk_cap on the page lists PagingSpec::EqualPagesUpTo cuts (chunk_config.rs:145-161,
restated here in Python), and pcodec_amd.paged imports without a GPU and fails loudly when called."""
import ctypes as C

import numpy as np
import pytest

from pcodec_amd import _lib as G
from pcodec_amd import build as B


@pytest.fixture(scope="module")
def lib():
    if B.needs_build():
        B.build()
    return G.lib()


def equal_pages_up_to(n, max_page_n):
    """chunk_config.rs:145-161: ceil(n / max) pages, the first n % pages of them one number longer"""
    k = -(-n // max_page_n)
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def test_new_entry_points_are_exported(lib):
    for name in ("pco_gfx_wrapped_chunk_cap_exact", "pco_gfx_compress_wrapped_chunks_ex", "pco_gfx_compact_wrapped_chunks", "pco_gfx_wrapped_scratch_estimate"):
        assert hasattr(lib, name), name


def test_wrapped_task_layout():
    assert C.sizeof(G.WrappedTask) == 48
    assert [getattr(G.WrappedTask, f).offset for f in ("src", "n", "dst", "dst_cap", "dtype", "n_pages", "page_sizes")] == [0, 8, 16, 24, 32, 36, 40]
    assert C.sizeof(G.PageInfo) == 32


@pytest.mark.parametrize("dict_mode", [False, True])
def test_exact_cap_equals_the_equal_pages_cap(lib, dict_mode):
    kw = dict(mode=G.MODE_TRY_DICT, delta=1, dict=True) if dict_mode else dict(mode=1, delta=2, delta_order=1)
    for level in (8, 12):
        for max_page_n in (1, 7, 256, 700, 16384, 1 << 18):
            cfg = G.make_config(level=level, max_page_n=max_page_n, enable_8_bit=True, **kw)
            for n in (1, 2, 255, 256, 257, 699, 700, 701, 5000, 20001, (1 << 18) + 1):
                if n / max_page_n > 30000:
                    continue
                sizes = equal_pages_up_to(n, max_page_n)
                assert len(sizes) == lib.pco_gfx_wrapped_n_pages(n, max_page_n) and sum(sizes) == n
                arr = (C.c_uint64 * len(sizes))(*sizes)
                for dt in range(1, 12):
                    want = lib.pco_gfx_wrapped_chunk_cap(n, dt, C.addressof(cfg))
                    assert want > 0 and lib.pco_gfx_wrapped_chunk_cap_exact(arr, len(sizes), dt, C.addressof(cfg)) == want, (n, max_page_n, dt, level)


def test_exact_cap_grows_with_the_page_count_and_rejects_nonsense(lib):
    cfg = G.make_config(mode=1, delta=1)
    one = (C.c_uint64 * 1)(1000); ten = (C.c_uint64 * 10)(*[100] * 10)
    assert lib.pco_gfx_wrapped_chunk_cap_exact(ten, 10, 1, C.addressof(cfg)) > lib.pco_gfx_wrapped_chunk_cap_exact(one, 1, 1, C.addressof(cfg)) > 1000 * 4
    assert lib.pco_gfx_wrapped_chunk_cap_exact(one, 1, 0, C.addressof(cfg)) == 0      # invalid dtype
    assert lib.pco_gfx_wrapped_chunk_cap_exact(one, 1, 12, C.addressof(cfg)) == 0
    assert lib.pco_gfx_wrapped_chunk_cap_exact(one, 0, 1, C.addressof(cfg)) == 0      # empty list
    assert lib.pco_gfx_wrapped_chunk_cap_exact(None, 0, 1, C.addressof(cfg)) == 0
    assert lib.pco_gfx_wrapped_chunk_cap_exact((C.c_uint64 * 2)(5, 0), 2, 1, C.addressof(cfg)) == 0   # a page of 0 numbers
    assert lib.pco_gfx_wrapped_chunk_cap_exact(one, 1, 1, None) == lib.pco_gfx_wrapped_chunk_cap(1000, 1, None) > 0   # NULL config = the default


def test_scratch_estimate_is_host_arithmetic(lib):
    """Needs no device: grows with the chunk count and with the page count, 0 for an invalid task."""
    cfg = G.make_config(mode=1, delta=2, delta_order=1, max_page_n=1000)
    def est(k, n, n_pages=0, sizes=None):
        t = (G.WrappedTask * k)(*[G.WrappedTask(0, n, 0, 1 << 40, 2, n_pages, C.cast(sizes, C.c_void_p) if sizes is not None else None) for _ in range(k)])
        return lib.pco_gfx_wrapped_scratch_estimate(k, t, C.addressof(cfg))
    a, b = est(100, 5000), est(200, 5000)
    assert a > 100 * 5000 * 8 and b == 2 * a
    many = (C.c_uint64 * 5000)(*[1] * 5000)
    assert est(100, 5000, 5000, many) > a
    assert est(3, 5000, 2, (C.c_uint64 * 2)(1, 2)) == 0 and lib.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT


def test_paged_imports_without_a_gpu_and_fails_loudly(lib):
    import pcodec_amd as P
    from pcodec_amd import paged
    assert P.paged is paged and callable(paged.compress_chunks) and callable(paged.decompress_chunks)
    assert P.ChunkConfig(paging_spec=P.PagingSpec.exact_page_sizes([3, 4])).paging_spec.exact == (3, 4)
    if lib.pco_gfx_device_count() == 0:
        with pytest.raises(G.PcoGfxError) as ei:
            paged.compress_chunks([], P.ChunkConfig())
        assert ei.value.status == G.ST_DEVICE_ERROR and "no CPU fallback" in str(ei.value)
        with pytest.raises(G.PcoGfxError) as ei:
            paged.decompress_chunks(None, [], [])
        assert ei.value.status == G.ST_DEVICE_ERROR
        t = (G.WrappedTask * 1)(G.WrappedTask(0, 10, 0, 1 << 20, 1, 0, None))
        infos = (G.PageInfo * 2)()
        assert lib.pco_gfx_compress_wrapped_chunks_ex(1, t, None, infos, None, None) == G.PcoCompressionError and lib.pco_gfx_last_status() == G.ST_DEVICE_ERROR
        assert lib.pco_gfx_compact_wrapped_chunks(1, t, None, None, 0, None, 0, 0, None, None, None) == G.PcoCompressionError and lib.pco_gfx_last_status() == G.ST_DEVICE_ERROR
