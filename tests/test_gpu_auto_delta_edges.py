"""-m gpu: DeltaSpec::Auto on the device -- split_gather_kernel's sample, the trial encodes in waves, enc_trial_summary_kernel and the host
replay in resolve_auto_delta -- at its sample, tie, wave and batch edges.

The rows, the edge each one sits on and the plain model of the decision and of the wave schedule are in tests/auto_delta_edges_util.py and
tests/auto_delta_model.py; tests/test_auto_delta_model.py pins all of it on the CPU (every row on its edge by the oracle's own estimates,
the model against the oracle, every wrong reading changing the rows that name it) before anything here runs.

For every row: the bytes equal the oracle's; the device decodes them bit for bit; and pco_gfx_debug_auto_delta -- the copies
resolve_auto_delta keeps of what it held -- shows the oracle's sample length and decision, the model's set of trial-encoded candidates,
and for each of them the oracle's size estimate as an f32 bit pattern: both sides are whole bytes, there is no tolerance.  Rows of one
config share one batched call.  One call of some 25 chunks in shuffled order, in its synchronous and asynchronous form, is compared chunk
by chunk with the same chunks encoded alone; two wrapped chunks of three odd pages take their decision from the whole chunk.  Nothing is
skipped."""
import ctypes as C

import numpy as np
import pytest

import auto_delta_edges_util as E
import auto_delta_model as M
import gpu_util as U
import oracle_lib as O
from pcodec_amd import _lib as G

pytestmark = pytest.mark.gpu

GROUPS = E.groups()
PAGE = 1 << 20          # one chunk per row, the 2^20 row included


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def device_records(L, n_chunks):
    out = (G.AutoDeltaRecord * (n_chunks + 1))()
    n = L.pco_gfx_debug_auto_delta(out, n_chunks + 1)
    assert n == n_chunks, (n, n_chunks)
    return [out[i] for i in range(n_chunks)]


def f32_bits(x): return int(np.array(x, dtype=np.float32).view(np.uint32))


def record_view(d): return (d.sample_n, d.eval_mask, tuple(f32_bits(c) for c in d.cost), (d.delta_kind, d.delta_order, d.window_n_log))


def check_record(name, d, n, oracle):
    """the device's record of one chunk against the oracle's estimates and decision and the model's wave schedule"""
    sn, costs, dec = oracle
    got_sn, got_mask, got_bits, got_dec = record_view(d)
    want_mask = M.schedule(costs, n)
    want_bits = tuple(f32_bits(costs[c]) if want_mask >> c & 1 else 0 for c in range(9))
    print(name, "sample", got_sn, sn, "mask", bin(got_mask), bin(want_mask), "costs", [float(c) for c in d.cost], None if costs is None else costs.tolist(), "plan", got_dec, dec)
    assert got_sn == sn, (name, got_sn, sn)
    assert got_dec == dec, (name, got_dec, dec)
    assert got_mask == want_mask, (name, bin(got_mask), bin(want_mask))
    assert got_bits == want_bits, (name, [float(c) for c in d.cost], costs.tolist() if costs is not None else None)


def configs(kw): return G.make_config(max_page_n=PAGE, enable_8_bit=True, **kw), O.make_config(max_page_n=PAGE, enable_8_bit=True, **kw)


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=["-".join(f"{k}{v}" for k, v in sorted(kw.items())) + f"-{len(rows)}rows" for kw, rows in GROUPS])
def test_rows_bytes_decode_and_record(L, g):
    """the rows of one config in one batched call"""
    kw, rows = GROUPS[g]
    cfg, ocfg = configs(kw)
    arrays = [r.arr for r in rows]
    got, back = U.gpu_batched(arrays, cfg)
    devs = device_records(L, len(rows))
    for r, d in zip(rows, devs): check_record(r.name, d, r.arr.size, E.oracle(r.name))
    bad = [r.name for r, b in zip(rows, got) if b != U.oracle_chunk(r.arr, ocfg)]
    assert not bad, bad
    bad = [r.name for r, b in zip(rows, back) if not U.bits_equal(b, r.arr)]
    assert not bad, bad


_ALONE = {}


def alone(L, name, a):
    """(bytes, record) of the chunk encoded in a call of its own"""
    if name not in _ALONE:
        got, _ = U.gpu_batched([a], configs(E.DEFAULT)[0])
        _ALONE[name] = (got[0], record_view(device_records(L, 1)[0]))
    return _ALONE[name]


@pytest.mark.parametrize("form", ["synchronous", "asynchronous"])
def test_one_shuffled_call_equals_its_chunks_alone(L, form):
    """Every stop 0..7 and both lookback outcomes in one call: the deeper waves run over scattered, shrinking sub-lists whose summaries lie
    candidate-major with another stride in every wave; unsampled chunks between them; equal n at different widths on one pooled index
    list; a 10-byte sample in front of a u64 one."""
    import torch
    chunks = E.batch_call()
    names = [n for n, _ in chunks]; arrays = [a for _, a in chunks]
    cfg, ocfg = configs(E.DEFAULT)
    st = U.Staged(L, arrays)
    tasks = st.enc_tasks()
    stream = torch.cuda.Stream() if form == "asynchronous" else None
    res = np.zeros(st.k, U.RES_DT) if form == "synchronous" else None
    G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(cfg), U.ptr(res) if res is not None else None, st.d_res.data_ptr(),
                                      C.c_void_p(stream.cuda_stream) if stream is not None else None))
    devs = device_records(L, st.k)                                            # (the records are the host's: nothing to wait for)
    torch.cuda.synchronize()
    d_res = st.results()
    if res is not None: assert all(np.array_equal(res[f], d_res[f]) for f in U.RES_DT.names)
    assert (d_res["status"] == 0).all(), d_res["status"]
    got = st.slot_bytes(d_res["n_out"])
    oracles = [O.auto_delta_costs(a, ocfg) for a in arrays]
    for nm, a, d, o in zip(names, arrays, devs, oracles): check_record(nm, d, a.size, o)
    bad = [nm for nm, a, b in zip(names, arrays, got) if b != U.oracle_chunk(a, ocfg)]
    assert not bad, bad
    for nm, a, b, d in zip(names, arrays, got, devs):
        assert (b, record_view(d)) == alone(L, nm, a), nm
    dres = np.zeros(st.k, U.RES_DT); dtasks = st.dec_tasks(d_res["n_out"])     # (held in a name: U.ptr keeps no reference to the array it points into)
    G.check(L.pco_gfx_decompress_chunks(st.k, U.ptr(dtasks), U.ptr(dres), None, None))
    assert (dres["status"] == 0).all() and st.outputs_equal() == []


@pytest.mark.parametrize("name,pages", E.WRAPPED, ids=[n for n, _ in E.WRAPPED])
def test_a_wrapped_chunk_of_three_odd_pages_decides_from_the_whole_chunk(L, name, pages):
    """the sample spans the pages, the lookback's window log comes from the chunk's n"""
    from test_gpu_wrapped_writer import Call, oracle_pieces
    r = E.by_name()[name]
    assert sum(pages) == r.arr.size and len(pages) == 3
    kw = dict(E.DEFAULT)
    c = Call(L, [r.arr], G.make_config(enable_8_bit=True, **kw), [pages])
    G.check(c.encode())
    check_record(name, device_records(L, 1)[0], r.arr.size, E.oracle(name))
    (meta, page_bytes, page_ns), = c.pieces()
    want = oracle_pieces(r.arr, kw, pages)
    assert page_ns == want[2] == pages
    assert meta == want[0] and page_bytes == want[1], name
    info = G.ChunkMetaInfo()
    buf = (C.c_uint8 * len(meta)).from_buffer_copy(meta)
    G.check(L.pco_gfx_chunk_meta_info(buf, len(meta), G.DTYPE_BYTE[r.arr.dtype.name], 4, C.byref(info)))
    assert (info.delta_kind, info.delta_order, info.window_n_log) == E.oracle(name)[2]
    c.decode_and_compare()


def test_hook_keeps_the_first_chunks_of_the_last_auto_delta_call_only(L):
    """an explicit delta spec leaves no records; a call of more than PCO_GFX_AUTO_DEBUG_MAX chunks keeps that many; a chunk without a sample
    leaves an all-zero record"""
    a = E.by_name()["monotone_stop2_u64"].arr; small = np.arange(9, dtype=np.uint16)
    U.gpu_simple_compress(a, G.make_config(delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))
    assert L.pco_gfx_debug_auto_delta(None, 0) == 0
    U.gpu_batched([small] + [a] * (G.AUTO_DEBUG_MAX + 2), G.make_config(enable_8_bit=True))
    out = (G.AutoDeltaRecord * (G.AUTO_DEBUG_MAX + 3))()
    assert L.pco_gfx_debug_auto_delta(out, G.AUTO_DEBUG_MAX + 3) == G.AUTO_DEBUG_MAX
    assert record_view(out[0]) == (0, 0, (0,) * 9, (0, 0, 0))
    sn, costs, dec = E.oracle("monotone_stop2_u64")
    assert all(record_view(out[i])[0] == sn and record_view(out[i])[3] == dec and out[i].eval_mask == 0x3f for i in range(1, G.AUTO_DEBUG_MAX))
    assert record_view(out[G.AUTO_DEBUG_MAX]) == (0, 0, (0,) * 9, (0, 0, 0))
    assert L.pco_gfx_debug_auto_delta(out, 1) == G.AUTO_DEBUG_MAX                  # a short buffer gets the first record and the full count
