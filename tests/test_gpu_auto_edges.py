"""-m gpu: ModeSpec::Auto detection on the device -- auto_int_gcd_kernel, auto_float_stats_kernel, auto_saved_kernel and the host step of
resolve_plans between them -- at its capacity, count and threshold edges.

The cases, the gate each one sits on and the plain model that says what every stage holds for it are in tests/auto_edges_util.py and
tests/auto_mode_model.py; tests/test_auto_mode_model.py pins all of it on the CPU (the model against the oracle, every case on its gate,
every wrong reading of a gate changing the cases that name it) before anything here runs.

For every case, with ModeSpec::Auto and no delta: the bytes equal the oracle's (or the error kind, should the oracle raise); the device
decodes them bit for bit; and pco_gfx_debug_auto_mode -- the copies resolve_plans keeps of what it held between the kernels -- equals the
model's record field for field: the route, the counts and flags exactly, the centred base and stage 2's sums as bit patterns.  For chunks
that take the host path only the route and the final bytes are compared.  A subset runs with both specs Auto, and one batched call in
shuffled order carries chunks of every route, 0 to 3 stage-2 candidates and equal sizes.  Nothing is skipped."""
import ctypes as C
import functools

import numpy as np
import pytest

import auto_edges_util as E
import auto_mode_model as M
import gpu_util as U
import oracle_lib as O
from pcodec_amd import _lib as G

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in E.cases()]
PAGE = 1 << 19          # one chunk per case, the capacity cases included


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def device_records(L, n_chunks):
    out = (G.AutoModeRecord * (n_chunks + 1))()
    n = L.pco_gfx_debug_auto_mode(out, n_chunks + 1)
    assert n == n_chunks, (n, n_chunks)
    return [out[i] for i in range(n_chunks)]


def device_view(d):
    v = {"route": d.route, "n_entries": d.n_entries, "overflow": d.overflow, "s_size": d.s_size, "tz5": d.tz5, "n_ints": d.n_ints, "n_gcd": d.n_gcd,
         "sim": list(d.sim), "has_euclid": d.has_euclid, "k": d.k, "base_c": d.base_c, "cand_mask": d.cand_mask, "bk": d.bk}
    for q in range(4): v.update({f"base{q}": d.base[q], f"inv{q}": d.inv[q], f"s_int{q}": d.s_int[q], f"s_dbl{q}": d.s_dbl[q]})
    return v


def compare_record(name, d, rec):
    """every field the model predicts equals the device's; a candidate that did not go to stage 2 left its slot empty"""
    want, got = M.hook_view(rec), device_view(d)
    wrong = {k: (got[k], w) for k, w in want.items() if got[k] != w}
    for q in range(4):
        if not (want.get("cand_mask", 0) >> q) & 1: wrong.update({f"{f}{q}": (got[f"{f}{q}"], 0) for f in ("base", "inv", "s_int", "s_dbl") if got[f"{f}{q}"] != 0})
    print(name, M.ROUTES[want["route"]], {k: want[k] for k in ("cand_mask", "n_entries", "s_size") if k in want})
    assert not wrong, (name, wrong)


def encode_or_kind(fn, *a):
    try: return fn(*a), None
    except O.OracleError as e: return None, e.kind
    except G.PcoGfxError as e: return None, e.status


@functools.lru_cache(maxsize=None)
def oracle_bytes(name, delta):
    return encode_or_kind(O.simple_compress, E.by_name()[name].arr, O.make_config(delta=delta, max_page_n=PAGE, enable_8_bit=True))


@pytest.mark.parametrize("name", NAMES)
def test_case_bytes_decode_and_record(L, name):
    c = E.by_name()[name]
    want, want_kind = oracle_bytes(name, O.DELTA_NOOP)
    got, got_kind = encode_or_kind(U.gpu_simple_compress, c.arr, G.make_config(delta=G.DELTA_NOOP, max_page_n=PAGE, enable_8_bit=True))
    assert got_kind == want_kind, (name, got_kind, want_kind)
    compare_record(name, device_records(L, 1)[0], E.record(name))
    if want is None: return
    assert got == want, (name, c.gate)
    assert U.bits_equal(U.gpu_simple_decompress(got, c.arr.dtype, c.arr.size), c.arr), name


@pytest.mark.parametrize("name", [c.name for c in E.cases() if c.both_auto])
def test_both_specs_auto(L, name):
    """the delta sample is split by the mode chosen here"""
    c = E.by_name()[name]
    want, want_kind = oracle_bytes(name, O.DELTA_AUTO)
    got, got_kind = encode_or_kind(U.gpu_simple_compress, c.arr, G.make_config(max_page_n=PAGE, enable_8_bit=True))
    assert got_kind == want_kind and got == want, (name, got_kind, want_kind)
    compare_record(name, device_records(L, 1)[0], E.record(name))
    assert U.bits_equal(U.gpu_simple_decompress(got, c.arr.dtype, c.arr.size), c.arr), name


def test_mixed_call_keeps_its_slots_apart(L):
    """One batched call: stage-2 tasks numbered over chunks with 0 to 3 candidates, overflowed chunks folded into the host list, chunks of
    equal n sharing one entry of the index pool."""
    chunks = E.mixed_call()
    names = [n for n, _ in chunks]; arrays = [a for _, a in chunks]
    sizes = [a.size for a in arrays]
    assert len(sizes) - len(set(sizes)) >= 2, sizes                                   # at least two pairs of equal n
    recs = [M.analyse(a) for a in arrays]
    routes = [r["route"] for r in recs]
    assert set(routes) == set(M.ROUTES), routes
    assert {len(r.get("cands", {})) for r in recs if r["route"] == "dev_float"} == {0, 1, 2, 3}
    assert {len(r["cands"]) for r in recs if r["route"] == "dev_int"} == {0, 1}
    got, back = U.gpu_batched(arrays, G.make_config(delta=G.DELTA_NOOP, max_page_n=PAGE, enable_8_bit=True))
    devs = device_records(L, len(arrays))
    for nm, d, r in zip(names, devs, recs): compare_record(nm, d, r)
    ocfg = O.make_config(delta=O.DELTA_NOOP, max_page_n=PAGE, enable_8_bit=True)                      # (one chunk each, the oversize one included)
    bad = [nm for nm, a, g in zip(names, arrays, got) if g != U.oracle_chunk(a, ocfg)]
    assert not bad, bad
    assert all(U.bits_equal(b, a) for a, b in zip(arrays, back))


def test_hook_keeps_the_first_chunks_of_the_last_call_only(L):
    """an explicit mode leaves no records; a call of more than PCO_GFX_AUTO_DEBUG_MAX chunks keeps that many"""
    a = np.arange(64, dtype=np.uint32) * 7
    U.gpu_simple_compress(a, G.make_config(mode=G.MODE_CLASSIC, delta=G.DELTA_NOOP))
    assert L.pco_gfx_debug_auto_mode(None, 0) == 0
    U.gpu_batched([a] * (G.AUTO_DEBUG_MAX + 3), G.make_config(delta=G.DELTA_NOOP))
    out = (G.AutoModeRecord * (G.AUTO_DEBUG_MAX + 3))()
    assert L.pco_gfx_debug_auto_mode(out, G.AUTO_DEBUG_MAX + 3) == G.AUTO_DEBUG_MAX
    want = M.hook_view(M.analyse(a))
    assert all(device_view(out[i])["route"] == want["route"] and out[i].base[3] == want.get("base3", 0) for i in range(G.AUTO_DEBUG_MAX))
    assert device_view(out[G.AUTO_DEBUG_MAX])["route"] == 0 and out[G.AUTO_DEBUG_MAX].cand_mask == 0
