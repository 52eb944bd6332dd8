"""-m gpu: the lookback search on the device -- enc_lookback_hash_kernel, enc_lookback_pipe_kernel<small | large>, enc_lookback_seq_kernel and
enc_lookback_kernel<LbSmall | LbFull> -- at its ring, count, window, sweep, bucket, hazard, crossing, screen and hand-back edges.

The rows, the plain model that says what each page's lookbacks are and which kernel decides it, and what every row claims are in
tests/lookback_model.py; tests/test_lookback_edges.py pins all of it on the CPU (the model against the oracle, the claims against the model's
event log, the coverage of every body on every route that can carry it) before anything here runs.

Rows that share a config and a call shape share ONE call, whatever their width and route (five calls in all): the pipeline instantiation and
the one-wave layout are properties of the CALL (its largest page and window), a call takes chunks of any number type, and the routes are
per page -- so one call per shape already mixes every route and width, and a call per (route, width) would launch the same kernels 20 times.  For every call: the bytes equal the oracle's; the device decodes
them bit for bit with guard bytes behind every chunk's numbers; pco_gfx_debug_lookback_routes equals the model's prediction page for page, so a
row built for the one-wave kernel that never reached it fails instead of quietly testing the pipeline; and the profile names the pipeline
instantiation and the one-wave layout the model predicts, and not the other.  The call of the large shape also carries copies of rows of the
small shape at its first, middle and last slot: their bytes are what the small call gave.  The same calls are then made once in the
asynchronous form.  Nothing is skipped."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_util as U
import lookback_model as M
import oracle_lib as O
from pcodec_amd import _lib as G
from test_gpu_width_paths import decode_call, encode_call
from test_gpu_wrapped_writer import Call

pytestmark = pytest.mark.gpu

GROUPS = M.groups()
GROUP_IDS = [f"{'int-mult' if g[0].kw['mode'] == 4 else 'classic'}-{g[0].paging or 'standalone'}-{g[0].shape[0]}-{g[0].shape[1]}" for g in GROUPS]
ROUTE_CODE = {"pipe": 0, "seq": 1, "back": 2}


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


@functools.lru_cache(maxsize=None)
def want(name):
    """The oracle's bytes of a row, once: a standalone chunk, or (ChunkMeta, [pages]) of a wrapped one."""
    r = M.BY_NAME()[name]
    if r.paging is None:
        return U.oracle_chunk(r.arr, O.make_config(enable_8_bit=True, **r.kw))
    meta, pages, ns = O.wrapped_compress(r.arr, O.make_config(enable_8_bit=True, **r.kw), max_pages=len(r.pages) + 1, exact_pages=r.pages if r.paging == "exact" else None)
    assert ns == r.pages
    return meta, pages


def with_copies(gi):
    """The rows of call gi; the large standalone call also carries three rows of the small one -- a pipeline page, a screened page and a
    handed-back page -- at its first, middle and last slot."""
    rows = list(GROUPS[gi])
    if rows[0].paging is None and rows[0].shape == ("large", "LbFull"):
        small = next(g for g in GROUPS if g[0].paging is None and g[0].shape == ("small", "LbSmall") and g[0].kw == rows[0].kw)
        picks = [next(r for r in small if r.routes == [rt]) for rt in ("pipe", "seq", "back")]
        rows = [picks[0]] + rows[:len(rows) // 2] + [picks[1]] + rows[len(rows) // 2:] + [picks[2]]
        assert M.call_shape([r.arr.size for r in rows], [p for r in rows for p in r.pages]) == ("large", "LbFull")
    return rows


def predicted_routes(rows):
    return [ROUTE_CODE[pr.route] for r in rows for pr in M.analysis_of(r.name)]


def device_routes(L, n_pages):
    out = np.full(n_pages + 8, 255, np.uint8)
    n = L.pco_gfx_debug_lookback_routes(out.ctypes.data_as(C.c_void_p), n_pages)
    assert n == n_pages and (out[n_pages:] == 255).all(), (n, n_pages)
    return out[:n_pages].tolist()


def check_routes_and_kernels(L, rows, names, shape):
    got, pred = device_routes(L, sum(len(r.pages) for r in rows)), predicted_routes(rows)
    pages = [(r.name, pi) for r in rows for pi in range(len(r.pages))]
    wrong = [(nm, pi, g, p) for (nm, pi), g, p in zip(pages, got, pred) if g != p]
    print(f"{len(rows)} chunks, {len(pages)} pages, {shape}: pipeline {pred.count(0)}, seq {pred.count(1)}, handed back {pred.count(2)}")
    assert not wrong, (len(wrong), wrong[:6])
    lb = {n for n in names if n.startswith("enc_lookback")}
    expect = {"enc_lookback_hash_kernel", M.PIPE_KERNEL[shape[0]], M.ONEWAVE_KERNEL[shape[1]]}
    if min(p for r in rows for p in r.pages) <= M.kLbSeqMaxPage: expect.add("enc_lookback_seq_kernel")
    assert lb == expect, (sorted(lb), sorted(expect))


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_bytes_routes_and_kernels_of_every_call(L, gi):
    rows = with_copies(gi)
    if rows[0].paging is None:
        chunks, names = encode_call([r.arr for r in rows], G.make_config(enable_8_bit=True, **rows[0].kw))
        check_routes_and_kernels(L, rows, names, GROUPS[gi][0].shape)
        bad = [r.name for r, c in zip(rows, chunks) if c != want(r.name)]
        print("chunks that differ from the oracle's:", bad)
        assert not bad, (len(bad), bad[:8])
        decode_call(chunks, [r.arr for r in rows])
        return
    c = Call(L, [r.arr for r in rows], G.make_config(enable_8_bit=True, **rows[0].kw), [r.pages if r.paging == "exact" else None for r in rows])
    L.pco_gfx_profile_begin()
    G.check(c.encode())
    names = U.profile_names(L)
    check_routes_and_kernels(L, rows, names, GROUPS[gi][0].shape)
    bad = [r.name for r, (meta, pages, ns) in zip(rows, c.pieces()) if (meta, pages) != want(r.name) or ns != r.pages]
    assert not bad, (len(bad), bad[:8])
    c.decode_and_compare()


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=GROUP_IDS)
def test_the_same_calls_in_the_asynchronous_form(L, gi):
    """results == NULL: nothing is read back between the kernels, every kernel is launched for every chunk; the bytes are the same."""
    import torch
    rows = with_copies(gi)
    cfg = G.make_config(enable_8_bit=True, **rows[0].kw)
    if rows[0].paging is None:
        s = U.Staged(L, [r.arr for r in rows])
        tasks = s.enc_tasks()
        G.check(L.pco_gfx_compress_chunks(s.k, U.ptr(tasks), C.byref(cfg), None, s.d_res.data_ptr(), None))
        torch.cuda.synchronize()
        res = s.results()
        assert (res["status"] == 0).all(), res["status"]
        got = s.slot_bytes(res["n_out"])
        assert [r.name for r, c in zip(rows, got) if c != want(r.name)] == []
        return
    c = Call(L, [r.arr for r in rows], cfg, [r.pages if r.paging == "exact" else None for r in rows])
    G.check(c.encode(sync=False))
    torch.cuda.synchronize()
    pieces = c.pieces(c.device_infos())
    assert [r.name for r, (m, p, ns) in zip(rows, pieces) if (m, p) != want(r.name) or ns != r.pages] == []
    c.decode_and_compare(c.device_infos())
