"""-m gpu: the ORDERED list of launches, repeats kept, of a matrix of small calls against tests/golden/launch_sequences.json.

The host drivers (launch_decode, run_encode's phases, resolve_auto_mode / resolve_auto_delta, the wrapped writer) decide which kernels a call
launches, in which order and how often; the other tests compare SETS of launched names for a few calls.  Here every call of the matrix runs in
its synchronous form and in its asynchronous form (results null, d_results given), and the names pco_gfx_profile_end reports -- kernels, the
`~` kernels of the side streams, the spans -- must be the recorded list, entry for entry.  A change of launch order, a launch gained or lost,
a renamed profile entry all fail here; a refactor of the drivers must leave the file as it is.

Every call's encoded bytes are also compared with the oracle, and every decode with the input.  The calls run in ONE child process whose
environment holds no PCO_GFX_* variable (as in test_gpu_switch_defaults.py): the switches are at their defaults.

The golden file is a recording: `python tests/test_gpu_launch_sequences.py` runs the same child and rewrites it (do that only with a library
whose launch sequences are known to be the intended ones, and say in the commit why they changed)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "launch_sequences.json")
pytestmark = pytest.mark.gpu

FORMS = ("sync", "async")
C2 = dict(mode=1, delta=2, delta_order=1)


def ramp(n, seed, dtype=np.uint64):
    """Classic + Consecutive(1) data: a noisy ramp, narrow first differences (gpu_util.synth("c2") at any width)."""
    r = np.random.default_rng(seed)
    step = {1: 0, 2: 3, 4: 1000, 8: 1000}[np.dtype(dtype).itemsize]
    noise = {1: 8, 2: 8, 4: 512, 8: 512}[np.dtype(dtype).itemsize]
    x = np.uint64(step) * np.arange(n, dtype=np.uint64) + r.integers(0, noise, n).astype(np.uint64)
    if np.dtype(dtype).itemsize == 8:
        x += np.uint64(1 << 40)
    return x.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the matrix: name -> (arrays, config keywords)
# ---------------------------------------------------------------------------------------------------------------------------------------
def batched_cases():
    import gpu_util as U
    from pcodec_amd import _lib as G
    rng = np.random.default_rng(77)
    cases = {}
    # width grouping (launch_decode: a null id list for one width, the grouped list for several; the encode side's per-width launches)
    cases["width_u64_only"] = ([ramp(3000, s) for s in range(3)], C2)
    cases["width_u32_u64"] = ([ramp(3000, 1, np.uint32), ramp(3000, 2), ramp(2500, 3, np.uint32), ramp(2000, 4)], C2)
    cases["width_all_four"] = ([ramp(3000, 1, np.uint8), ramp(3000, 2, np.uint16), ramp(3000, 3, np.uint32), ramp(3000, 4)], C2)
    cases["width_8x4096"] = ([ramp(4096, s) for s in range(8)], C2)
    # encode branches under Classic + Consecutive(1)
    cases["c2_segmented_walk_8x2p15"] = ([ramp(1 << 15, s) for s in range(8)], C2)
    cases["c2_fused_walk_1100x2048"] = (U.tile([ramp(2048, s) for s in range(5)], 1100), C2)
    # other encode modes
    cases["int_mult"] = ([(rng.integers(0, 5000, 6000) * 1000 + 7).astype(np.int64), (rng.integers(0, 900, 5000) * 1000).astype(np.uint32)], dict(mode=G.MODE_TRY_INT_MULT, mode_u64=1000, delta=1))
    cases["float_mult"] = ([U.synth("c3", 6000, seed=s) for s in range(2)], dict(mode=G.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=1))
    cases["lookback_4x2p16"] = ([U.synth("c4", 1 << 16, seed=s) for s in range(4)], dict(mode=1, delta=G.DELTA_TRY_LOOKBACK))
    cases["level12_big_bins_2x2p13"] = ([ramp(1 << 13, s) for s in range(2)], dict(level=12, **C2))
    cases["strict_histogram"] = ([ramp(5000, s) for s in range(2)], dict(strict_histogram=True, **C2))
    # a value range beyond the counting tiers: the select and sort tiers
    cases["wide_range_2x2p14"] = ([rng.integers(0, 1 << 63, 1 << 14, dtype=np.uint64) for _ in range(2)], dict(mode=1, delta=1))
    # Auto mode + Auto delta: stage 1 and 2 on ints and floats, both waves of delta trials (the cubic ramp goes on past order 2)
    i = np.arange(1 << 14, dtype=np.uint64)
    auto = [ramp(1 << 14, 1), ramp(1 << 14, 2), (rng.integers(0, 40000, 1 << 14) * 1000).astype(np.int64), (rng.integers(0, 3000, 1 << 14) * 77).astype(np.uint32),
            U.synth("c3", 1 << 14, seed=5), (rng.integers(1000, 90000, 1 << 14) / 100.0).astype(np.float32),
            i * i * i // np.uint64(7) + rng.integers(0, 4, 1 << 14).astype(np.uint64), np.cumsum(np.cumsum(rng.integers(-3, 4, 1 << 14))).astype(np.int32)]
    cases["auto_mode_auto_delta_8x2p14"] = (auto, dict())
    return cases


def reference_chunks(arrays, kw):
    """The oracle's standalone chunk for every array of a batched case (an array that is in the call several times is encoded once)."""
    import gpu_util as U
    import oracle_lib as O
    okw = {k: v for k, v in kw.items() if k != "strict_histogram"}   # (the strict histogram IS the reference's; the oracle has no flag for it)
    ocfg = O.make_config(**okw)
    memo = {}
    out = []
    for a in arrays:
        if id(a) not in memo:
            memo[id(a)] = U.oracle_chunk(a, ocfg)
        out.append(memo[id(a)])
    return out


def run_batched(L, name, arrays, kw, asynchronous):
    """pco_gfx_compress_chunks, then pco_gfx_decompress_chunks over what it wrote: (encode launches, decode launches)."""
    import torch
    import gpu_util as U
    from pcodec_amd import _lib as G
    cfg = G.make_config(enable_8_bit=True, **kw)
    s = U.Staged(L, arrays)
    et = s.enc_tasks()
    L.pco_gfx_profile_begin()
    if asynchronous:
        G.check(L.pco_gfx_compress_chunks(s.k, U.ptr(et), C.byref(cfg), None, s.d_res.data_ptr(), None))
        torch.cuda.synchronize()
        res = s.results()
    else:
        res = np.zeros(s.k, U.RES_DT)
        G.check(L.pco_gfx_compress_chunks(s.k, U.ptr(et), C.byref(cfg), U.ptr(res), None, None))
    enc = U.profile_launches(L)
    assert (res["status"] == 0).all(), res["status"]
    chunks = s.slot_bytes(res["n_out"])
    want = reference_chunks(arrays, kw)
    bad = [i for i, (c, w) in enumerate(zip(chunks, want)) if c != w]
    assert not bad, f"{name}: chunks {bad[:8]} differ from the oracle's"
    dt = s.dec_tasks(res["n_out"])
    L.pco_gfx_profile_begin()
    if asynchronous:
        G.check(L.pco_gfx_decompress_chunks(s.k, U.ptr(dt), None, s.d_dres.data_ptr(), None))
        torch.cuda.synchronize()
        dres = s.results(s.d_dres)
    else:
        dres = np.zeros(s.k, U.RES_DT)
        G.check(L.pco_gfx_decompress_chunks(s.k, U.ptr(dt), U.ptr(dres), None, None))
    dec = U.profile_launches(L)
    assert (dres["status"] == 0).all() and np.array_equal(dres["n_out"], s.n) and np.array_equal(dres["consumed"], res["n_out"]), dres
    assert s.outputs_equal() == [], f"{name}: decoded chunks differ from the input"
    return enc, dec


def run_conv1(L, asynchronous):
    """Conv1 order 2 under PCO_GFX_CFG_CONV1: the bytes against the oracle's generator given the product's fit (the oracle does not fit)."""
    import gpu_util as U
    import oracle_lib as O
    import test_gpu_conv1_encode as TC
    from pcodec_amd import _lib as G
    arrays = [TC.smooth(6000, np.int32, 3), TC.smooth(5000, np.uint16, 4)]
    cfg = TC.cfg(2)
    L.pco_gfx_profile_begin()
    chunks, aux = TC.compress(arrays, cfg, sync=not asynchronous)
    enc = U.profile_launches(L)
    for a, ch in zip(arrays, chunks):
        p = TC.params(ch, a.dtype)
        assert p is not None, "the fit gave Conv1 up on smooth data"
        f = O.test_encode(a, mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, quantization=p[0], bias=p[1], weights=p[2], level=8)
        assert U.chunk_of_file(f, len(ch)) == ch, "Conv1 chunk differs from the oracle's"
    dec = decode_chunks(L, chunks, arrays, asynchronous)
    return enc, dec


def run_dict(L, asynchronous):
    """Dict mode under PCO_GFX_CFG_DICT: the bytes against the oracle's chunk for the relabelled input, with the product's dictionary."""
    import gpu_util as U
    import test_gpu_conv1_encode as TC
    import test_gpu_dict_encode as TD
    rng = np.random.default_rng(9)
    pool = rng.integers(0, 1 << 62, 300, dtype=np.uint64)
    arrays = [pool[np.minimum(rng.zipf(1.3, 5000), len(pool)) - 1], pool[:50].astype(np.uint32)[rng.integers(0, 50, 4000)]]
    L.pco_gfx_profile_begin()
    chunks, aux = TC.compress(arrays, TD.cfg(), sync=not asynchronous)
    enc = U.profile_launches(L)
    for a, ch in zip(arrays, chunks):
        d = TD.dict_of_chunk(ch, a.dtype)
        assert d is not None, "a Dict call wrote a chunk without a dictionary"
        assert ch == TD.patched_oracle_chunk(a, d, ch), "Dict chunk differs from the oracle's"
    dec = decode_chunks(L, chunks, arrays, asynchronous)
    return enc, dec


def decode_chunks(L, chunks, arrays, asynchronous, flags=0):
    """One pco_gfx_decompress_chunks call over host chunk bytes; the numbers must be the input's.  Returns the launches."""
    import torch
    import gpu_util as U
    from pcodec_amd import _lib as G
    k = len(chunks)
    srcs = [torch.from_numpy(np.frombuffer(bytes(c) + bytes(64), np.uint8).copy()).cuda() for c in chunks]
    outs = [torch.zeros(max(a.nbytes, 1) + 16, dtype=torch.uint8, device="cuda") for a in arrays]
    tasks = (G.DecodeTask * k)(*[G.DecodeTask(s.data_ptr(), len(c), o.data_ptr(), a.size, G.DTYPE_BYTE[a.dtype.name], flags) for s, c, o, a in zip(srcs, chunks, outs, arrays)])
    d_res = torch.zeros(k * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.pco_gfx_profile_begin()
    if asynchronous:
        G.check(L.pco_gfx_decompress_chunks(k, tasks, None, d_res.data_ptr(), None))
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(U.RES_DT)
    else:
        res = np.zeros(k, U.RES_DT)
        G.check(L.pco_gfx_decompress_chunks(k, tasks, U.ptr(res), None, None))
    dec = U.profile_launches(L)
    assert (res["status"] == 0).all(), res["status"]
    for o, a, r, c in zip(outs, arrays, res, chunks):
        assert int(r["n_out"]) == a.size and int(r["consumed"]) == len(c)
        assert U.bits_equal(o[: a.nbytes].cpu().numpy().view(a.dtype), a), "decoded chunk differs from the input"
    return dec


def run_wrapped(L, asynchronous):
    """The wrapped writer on 4 chunks x 4 pages, then pco_gfx_decompress_pages over them."""
    import torch
    import gpu_util as U
    import test_gpu_wrapped_writer as T
    from pcodec_amd import _lib as G
    arrays = [ramp(4000, s) for s in range(2)] + [ramp(3000, 7, np.uint32), ramp(2600, 8, np.uint16)]
    lists = [[1000] * 4, [1, 999, 2000, 1000], [750] * 4, [650] * 4]
    c = T.Call(L, arrays, G.make_config(enable_8_bit=True, **C2), lists)
    L.pco_gfx_profile_begin()
    G.check(c.encode(sync=not asynchronous))
    enc = U.profile_launches(L)
    infos = c.device_infos() if asynchronous else c.infos
    for a, pl, g in zip(c.arrays, lists, c.pieces(infos)):
        want = T.oracle_pieces(a, C2, pl)
        assert g[2] == want[2] == pl and g[0] == want[0] and g[1] == want[1], "wrapped pieces differ from the oracle's"
    pt = c.page_tasks(infos)
    d_res = torch.zeros(len(pt) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
    c.out.zero_(); torch.cuda.synchronize()
    L.pco_gfx_profile_begin()
    if asynchronous:
        G.check(L.pco_gfx_decompress_pages(len(pt), U.ptr(pt), None, d_res.data_ptr(), None))
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(U.RES_DT)
    else:
        res = np.zeros(len(pt), U.RES_DT)
        G.check(L.pco_gfx_decompress_pages(len(pt), U.ptr(pt), U.ptr(res), None, None))
    dec = U.profile_launches(L)
    assert (res["status"] == 0).all() and np.array_equal(res["n_out"], pt["page_n"]) and np.array_equal(res["consumed"], pt["page_len"])
    host = c.out.cpu().numpy()
    assert np.array_equal(host[: c.in_off[-1]], c.host_in[: c.in_off[-1]]), "decoded pages differ from the input"
    return enc, dec


def run_decode_retry(L, asynchronous):
    """A legal stream no reference encoder writes: 16384 bins under ans_size_log 14, tables beyond pco_decode_kernel's LDS.  A synchronous call
    gets the task back with the need-scratch status and decodes it in a second pass; an asynchronous one holds the table scratch from the start."""
    import foreign_tables_util as F
    import gpu_util as U
    import oracle_lib as O
    from pcodec_amd import _lib as G
    x = F.clustered(np.uint32, 17000, seed=232)
    y = ramp(3000, 5, np.uint32)
    f = O.test_encode(x, tbl_vars=O.TBL_PRIMARY, tbl_n_bins=16384, tbl_ans_size_log=14, tbl_weight_style=O.TBL_W_ONES, tbl_seed=1)
    assert U.bits_equal(O.simple_decompress(f, x.dtype, cap=x.size + 8), x)
    files = [f, O.simple_compress(y, O.make_config(**C2))]
    return [], decode_chunks(L, files, [x, y], asynchronous, flags=G.TASK_HAS_FILE_HEADER)


def child():
    """Every case in both forms; prints `REPORT {case: {form: {"encode": [...], "decode": [...]} or {"error": text}}}`."""
    import traceback
    sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
    from pcodec_amd import _lib as G
    L = G.lib()
    assert L.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    runs = {name: (lambda a, name=name, arrays=arrays, kw=kw: run_batched(L, name, arrays, kw, a)) for name, (arrays, kw) in batched_cases().items()}
    runs["conv1_order2"] = lambda a: run_conv1(L, a)
    runs["dict"] = lambda a: run_dict(L, a)
    runs["wrapped_4x4_pages"] = lambda a: run_wrapped(L, a)
    runs["decode_retry_with_scratch"] = lambda a: run_decode_retry(L, a)
    rep = {}
    for name, fn in runs.items():
        rep[name] = {}
        for form in FORMS:
            try:
                enc, dec = fn(form == "async")
                rep[name][form] = {"encode": enc, "decode": dec}
            except Exception:
                rep[name][form] = {"error": traceback.format_exc()[-1500:]}
    print("REPORT " + json.dumps(rep))


def run_child():
    env = {k: v for k, v in os.environ.items() if not k.startswith("PCO_GFX_")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("REPORT ")][-1][7:])


CASES = ("width_u64_only", "width_u32_u64", "width_all_four", "width_8x4096", "c2_segmented_walk_8x2p15", "c2_fused_walk_1100x2048", "int_mult", "float_mult",
         "lookback_4x2p16", "level12_big_bins_2x2p13", "strict_histogram", "wide_range_2x2p14", "auto_mode_auto_delta_8x2p14", "conv1_order2", "dict",
         "wrapped_4x4_pages", "decode_retry_with_scratch")


@pytest.fixture(scope="module")
def report():
    return run_child()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_matrix_is_the_recorded_one(report, golden):
    assert set(report) == set(golden) == set(CASES)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_launch_sequence(report, golden, case, form):
    got, want = report[case][form], golden[case][form]
    assert "error" not in got, got["error"]
    for side in ("encode", "decode"):
        assert got[side] == want[side], (case, form, side, [(i, a, b) for i, (a, b) in enumerate(zip(got[side], want[side])) if a != b][:4], len(got[side]), len(want[side]))


def test_the_recording_reaches_what_the_matrix_names(golden):
    """The calls were chosen for the branches they take; the recording must show them (else a case has quietly stopped covering its branch)."""
    def names(case, form="sync", side="encode"):   # (without the `~` of a launch under a span)
        return [n.lstrip("~") for n in golden[case][form][side]]
    assert "enc_walkseg_kernel" in names("c2_segmented_walk_8x2p15") and "enc_walkp_kernel" not in names("c2_segmented_walk_8x2p15")
    fused = names("c2_fused_walk_1100x2048")
    assert "enc_walkp_kernel" in fused and "enc_place+pack" in fused and "enc_place_kernel" in fused and "enc_pack_kernel" in fused
    assert "dec_walk+trail<u64>" in names("c2_fused_walk_1100x2048", side="decode") and "dec_trail2_kernel<u64>" in names("c2_fused_walk_1100x2048", side="decode")
    assert [n for n in names("width_all_four", side="decode") if n.startswith("pco_decode_kernel")] == ["pco_decode_kernel<u64>", "pco_decode_kernel<u32>", "pco_decode_kernel<u16>", "pco_decode_kernel<u8>"]
    assert "enc_lookback_hash_kernel" in names("lookback_4x2p16") and "enc_pack1_kernel<lb>" in names("lookback_4x2p16")
    assert "enc_pack1_kernel<sec>" in names("int_mult") and "enc_pack1_kernel<sec>" in names("float_mult")
    assert "enc_conv1_solve_kernel" in names("conv1_order2") and "enc_dict_lds_kernel" in names("dict") and "enc_dict_place_kernel" in names("dict")
    assert "enc_train_big_kernel" in names("level12_big_bins_2x2p13") and "enc_hist_literal_kernel" in names("strict_histogram")
    assert "enc_hist_select_kernel" in names("wide_range_2x2p14") and "enc_hist_sort_kernel" in names("wide_range_2x2p14")
    auto = names("auto_mode_auto_delta_8x2p14")
    assert auto.count("enc_train_kernel") >= 3, "Auto delta: the first wave of trials, a deeper one, and the final encode"
    assert "wrapped_infos_kernel" in names("wrapped_4x4_pages")
    assert names("decode_retry_with_scratch", side="decode").count("pco_decode_kernel<u32>") == 2
    assert names("decode_retry_with_scratch", "async", "decode").count("pco_decode_kernel<u32>") == 1


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:   # the recorder
        rep = run_child()
        errors = {(c, f): v["error"] for c, forms in rep.items() for f, v in forms.items() if "error" in v}
        assert not errors, errors
        out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
        with open(out, "w") as f:
            json.dump(rep, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"recorded {len(rep)} cases into {out}")
