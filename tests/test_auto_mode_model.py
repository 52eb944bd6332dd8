"""-m "not gpu": the plain model of Auto mode detection (auto_mode_model.py) and the case table (auto_edges_util.py) that
test_gpu_auto_edges.py runs on the device, pinned on the CPU.

For every case: the model's final mode and base are the oracle's (chunk_plan without delta); the pieces the oracle exposes -- the sample
positions, choose_candidate_base on u32, the float-quant bid on f32 -- and the product's host-path bids (FloatDetect<L>::mult_bid /
quant_bid of pco_auto_host.inc, compiled on their own as test_host_logic.py does) agree with the model's; the case sits on the gate it
names; and every wrong reading of a gate that a case names changes that case's record, so an input that would let an off-by-one through
cannot stay in the table unnoticed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import auto_edges_util as E
import auto_mode_model as M
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pcodec_amd", "csrc")
NAMES = [c.name for c in E.cases()]
MODE_NAME = {0: "classic", 1: "int_mult", 2: "float_mult", 3: "float_quant"}
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_sample_positions_are_the_oracles():
    for n in (0, 9, 10, 11, 49, 50, 410, 2010, 46400, 265889, 265890):
        got, want = M.sample_indices(n), O.mode_sample_indices(n)
        assert (got is None and len(want) == 0) or got == list(want), n
    assert len(M.sample_indices(265889)) == M.AUTO_CAP and len(M.sample_indices(265850)) == M.AUTO_CAP and len(M.sample_indices(265849)) == M.AUTO_CAP - 1


@pytest.mark.parametrize("name", NAMES)
def test_case_mode_is_the_oracles_and_sits_on_its_gate(name):
    c = E.by_name()[name]; r = E.record(name)
    info, _, _ = O.chunk_plan(c.arr, O.make_config(delta=O.DELTA_NOOP, max_page_n=1 << 19, enable_8_bit=True))
    want = (MODE_NAME[info.mode_kind], info.mode_k if info.mode_kind == 3 else (info.mode_base_latent if info.mode_kind else 0))
    assert tuple(r["mode"]) == want, (name, r["mode"], want)
    assert c.claim(r) is True, (name, c.gate)
    if r.get("has_euclid"): assert r["weight_sum"] > 0, name             # (see auto_edges_util's docstring: no sample divides 0 by 0)
    if r["route"] in ("dev_int", "dev_float"): assert r["sample_n"] <= M.AUTO_CAP and not (r.get("gcd") or {}).get("overflow")


@pytest.mark.parametrize("name", [c.name for c in E.cases() if c.arr.dtype == np.uint32 and c.arr.size >= 10])
def test_int_candidate_is_the_oracles(name):
    c = E.by_name()[name]; r = E.record(name)
    s = np.ascontiguousarray(c.arr[O.mode_sample_indices(c.arr.size)])
    base, score, found = C.c_uint32(0), C.c_double(0), C.c_int(0)
    assert O.lib().pco_oracle_choose_candidate_base_u32(s.ctypes.data_as(C.c_void_p), C.c_size_t(len(s)), C.byref(base), C.byref(score), C.byref(found)) == 0
    cand = r["cands"].get("int")
    assert bool(found.value) == (cand is not None), name
    if cand: assert (base.value, score.value) == (cand["base"], cand["score"]), name
    assert sum(c_ for _, c_ in r["gcd"]["counts"]) <= len(s) // 3 and r["gcd"]["n_listed"] <= r["gcd"]["n_distinct"]


def _kept(c):
    K = E.FK[c.arr.dtype.type]; s = c.arr[O.mode_sample_indices(c.arr.size)]
    bits = s.view(K.U) & K.U(K.mid - 1)
    e = bits >> K.U(K.prec)
    return np.ascontiguousarray(bits[(e != 0) & (e != (1 << (K.bits - 1 - K.prec)) - 1) & (bits <= K.max_for_sampling)].view(c.arr.dtype))


@pytest.mark.parametrize("name", [c.name for c in E.cases() if c.arr.dtype == np.float32 and c.arr.size >= 10])
def test_float_quant_bid_is_the_oracles(name):
    c = E.by_name()[name]; r = E.record(name)
    s = _kept(c)
    assert len(s) == r["kept"]
    if len(s) < M.MIN_SAMPLE: return
    k, saved, found = C.c_uint32(0), C.c_double(0), C.c_int(0)
    assert O.lib().pco_oracle_float_quant_bid_f32(s.ctypes.data_as(C.c_void_p), C.c_size_t(len(s)), C.byref(k), C.byref(saved), C.byref(found)) == 0
    assert bool(found.value) == (r["quant_est"] > M.QUANT_REQUIRED), name
    if found.value: assert (k.value, saved.value) == (r["bk"], r["quant_est"]), name
    assert ("quant" in r["cands"]) == (r["best"] > M.QUANT_PREFILTER) and (r["quant_est"] <= r["best"] or r["best"] > M.QUANT_REQUIRED)


@pytest.fixture(scope="module")
def host_bids(tmp_path_factory):
    d = tmp_path_factory.mktemp("autobids")
    src = d / "bids.cpp"; out = d / "libbids.so"
    src.write_text(f'''
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>
#include <cmath>
#include "{CSRC}/pco_half.h"
#include "{CSRC}/pco_auto_host.inc"
using namespace pcogfx::autodetect;
template <class L> static int bids(const L* bits, size_t n, uint64_t* out, double* v) {{
  typedef typename FloatTraits<L>::F F;
  std::vector<F> s(n); for (size_t i = 0; i < n; i++) s[i] = fbits<L>(bits[i]);
  MultConfig<L> c{{}}; v[0] = v[1] = 0; out[0] = out[1] = out[2] = 0; uint32_t k = 0;
  const bool m = FloatDetect<L>::mult_bid(s, c, v[0]); if (m) {{ out[0] = tobits<L>(c.base); out[1] = tobits<L>(c.inv_base); }}
  const bool q = FloatDetect<L>::quant_bid(s, k, v[1]); out[2] = k;
  return (m ? 1 : 0) | (q ? 2 : 0);
}}
extern "C" int bids32(const uint32_t* b, size_t n, uint64_t* out, double* v) {{ return bids<uint32_t>(b, n, out, v); }}
extern "C" int bids64(const uint64_t* b, size_t n, uint64_t* out, double* v) {{ return bids<uint64_t>(b, n, out, v); }}
''')
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-w", "-o", str(out), str(src)])
    return C.CDLL(str(out))


@needs_gxx
def test_host_path_bids_agree_with_the_model(host_bids):
    n_mult = n_quant = 0
    for c in E.cases():
        if c.arr.dtype.kind != "f" or c.arr.size < 10: continue
        r = E.record(c.name)
        if r["kept"] < M.MIN_SAMPLE: continue
        K = E.FK[c.arr.dtype.type]; s = _kept(c).view(K.U)
        out = (C.c_uint64 * 3)(); v = (C.c_double * 2)()
        got = (host_bids.bids32 if K.bits == 32 else host_bids.bids64)(s.ctypes.data_as(C.c_void_p), C.c_size_t(len(s)), out, v)
        fm = [n for n in ("tz", "euclid") if n in r["cands"] and r["cands"][n]["stage2"]["est"] >= M.MULT_REQUIRED]
        best = None
        for n in fm:
            if best is None or not r["cands"][n]["stage2"]["est"] < r["cands"][best]["stage2"]["est"]: best = n
        assert bool(got & 1) == (best is not None), c.name
        if best:
            assert (out[0], out[1], v[0]) == (r["cands"][best]["base_bits"], r["cands"][best]["inv_bits"], r["cands"][best]["stage2"]["est"]), c.name
            n_mult += 1
        assert bool(got & 2) == (r["quant_est"] > M.QUANT_REQUIRED), c.name
        if got & 2: assert (out[2], v[1]) == (r["bk"], r["quant_est"]), c.name; n_quant += 1
    assert n_mult >= 10 and n_quant >= 10


def test_every_named_wrong_reading_changes_its_cases():
    seen = {v: 0 for v in M.VARIANTS}
    for c in E.cases():
        for v in c.variants:
            rv = M.analyse(c.arr, v)
            assert rv != E.record(c.name), (c.name, v)
            assert M.hook_view(rv) != M.hook_view(E.record(c.name)) or rv["mode"] != E.record(c.name)["mode"], (c.name, v, "nothing the device tests compare changes")
            seen[v] += 1
    assert all(seen.values()), seen


def test_the_table_reaches_every_route_and_capacity():
    recs = [E.record(n) for n in NAMES]
    assert {r["route"] for r in recs} == set(M.ROUTES)
    assert {r["gcd"]["n_listed"] for r in recs if r.get("gcd")} >= {M.GCD_MAX_ENTRIES, M.GCD_MAX_ENTRIES + 1}
    assert {r["gcd"]["n_distinct"] for r in recs if r.get("gcd")} >= {M.GCD_SLOTS - 1, M.GCD_SLOTS}
    assert {r["sample_n"] for r in recs} >= {0, 10, 255, 256, 511, 512, M.AUTO_CAP, M.AUTO_CAP + 1}
    assert {r["kept"] for r in recs if "kept" in r} >= {9, 10, 1000, 1001, M.AUTO_CAP}
    mixed = [M.analyse(a) for _, a in E.mixed_call()]
    assert {r["route"] for r in mixed} == set(M.ROUTES)


@needs_gxx
def test_hook_record_layout_is_the_headers(tmp_path):
    """pcodec_amd._lib.AutoModeRecord mirrors PcoGfxAutoModeRecord of include/pco_gfx.h field for field"""
    from pcodec_amd import _lib as G
    fields = [f[0] for f in G.AutoModeRecord._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "%s/include/pco_gfx.h"\nint main() { printf("%%zu %%d", sizeof(PcoGfxAutoModeRecord), PCO_GFX_AUTO_DEBUG_MAX); %s return 0; }\n'
                   % (ROOT, " ".join('printf(" %%zu", offsetof(PcoGfxAutoModeRecord, %s));' % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-w", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(G.AutoModeRecord), G.AUTO_DEBUG_MAX] + [getattr(G.AutoModeRecord, f).offset for f in fields]
