"""-m gpu: verified encodes (include/pco_gfx.h section 3b): PCO_GFX_CFG_VERIFY on the standalone, wrapped and host-buffer encoders,
pco_gfx_verify_chunks / pco_gfx_verify_wrapped_chunks as steps of their own, and pcodec_amd.paged's `verified` / verify_chunks.

References: the unflagged call of the same library for "the flag changes no byte"; the inputs themselves for every comparison (a verify IS the
comparison with the input, so a changed input is the failing case that needs no damaged stream); for damaged streams the outcomes
tests/test_verify_abi.py certifies with the oracle's decoder (tests/verify_util.py) -- none of the expected values comes from the code under test.
Nothing here is built to fault: the damage is a flipped offset bit, a mode nibble that names no mode, or offsets overwritten with zeros.

Shapes: chunks of 1, 255, 256, 257, 1000 and 4097 numbers; one chunk of 2^20 numbers for the compare kernel's pieces.

Measured on an MI355X: the module adds about 14 s to the -m gpu suite (46 tests; the two that start child processes take 4 s each)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import gpu_util as U  # noqa: E402
import verify_util as V  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from test_gpu_wrapped_writer import Call, INFO_DT  # noqa: E402

pytestmark = pytest.mark.gpu

ONES = (1 << 64) - 1
SIZES = [1, 255, 256, 257, 1000, 4097]
INTS = ["uint32", "uint64", "int32", "int64", "uint16", "int16", "uint8", "int8"]
FLOATS = ["float32", "float64", "float16"]


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def handle(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def nums(name, n, seed):
    """n smooth numbers of type `name`: multiples of 10 (of 0.01 for floats), so that every mode has something to find"""
    r = np.random.default_rng(seed)
    dt = np.dtype(name)
    if dt.kind == "f":
        return (r.integers(1000, 2000, n) / 100.0).astype(dt)
    return (r.integers(0, 12, n) * 10).astype(dt) if dt.itemsize == 1 else (r.integers(0, 50, n) * 10 + 1000).astype(dt)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the flag changes no byte
# ---------------------------------------------------------------------------------------------------------------------------------------
SPECS = {   # name -> (config, number types, sizes)
    "classic": (dict(mode=1, delta=1), INTS + FLOATS, SIZES),
    "int_mult": (dict(mode=4, mode_u64=10, delta=1), ["uint32", "int64", "uint16"], SIZES),
    "float_mult": (dict(mode=2, mode_f64=0.01, delta=1), ["float32", "float64"], SIZES),
    "float_quant": (dict(mode=3, mode_u64=8, delta=1), ["float32", "float64"], SIZES),
    "dict": (dict(mode=5, delta=1, dict=True), ["uint32", "float64", "int16"], SIZES),
    "conv1": (dict(mode=1, delta=4, delta_order=2, conv1=True), ["uint32", "float32", "int16"], SIZES),
    "consecutive0": (dict(mode=1, delta=2, delta_order=0), ["uint32", "int64"], SIZES),
    "consecutive1": (dict(mode=1, delta=2, delta_order=1), ["uint32", "int64", "float32", "uint16"], SIZES),
    "consecutive7": (dict(mode=1, delta=2, delta_order=7), ["uint32", "int64"], SIZES),
    "lookback": (dict(mode=1, delta=3), ["uint32", "int64"], SIZES),
    "auto": (dict(), ["uint32", "float64", "int16"], SIZES),
    "level0": (dict(mode=1, delta=1, level=0), ["uint32", "uint64", "uint8"], SIZES),
    "level12": (dict(mode=1, delta=2, delta_order=1, level=12), ["uint32", "uint64"], SIZES),
}


def spec_arrays(name):
    kw, types, sizes = SPECS[name]
    arrays = [nums(t, n, 100 * i + j) for i, t in enumerate(types) for j, n in enumerate(sizes)]
    if name == "consecutive1":   # an incompressible chunk: the delta's moments make it longer than the plain numbers, and it falls back
        arrays.append(np.random.default_rng(9).integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32))
    return arrays


def std_call(L, st, cfg, sync, stream=None):
    """one pco_gfx_compress_chunks call over st into slots filled with 0xff: (code, host results or None, device results, the whole slot area)"""
    import torch
    st.slots.fill_(0xff); st.d_res.zero_(); torch.cuda.synchronize()
    tasks = st.enc_tasks(); res = np.zeros(st.k, U.RES_DT)
    code = L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(cfg), U.ptr(res) if sync else None, st.d_res.data_ptr(), handle(stream))
    torch.cuda.synchronize()
    return code, (res if sync else None), st.results(), st.slots.cpu().numpy().copy()


def assert_flag_only_adds_the_bit(plain, flagged, what):
    """per task or piece: an OK one differs by PCO_GFX_AUX_VERIFIED alone, a failed one not at all"""
    assert len(plain) == len(flagged)
    for i, (p, f) in enumerate(zip(plain, flagged)):
        if p["status"] == 0:
            assert f["status"] == 0 and f["aux"] == p["aux"] | G.AUX_VERIFIED and not p["aux"] & G.AUX_VERIFIED, (what, i, p, f)
            assert all(f[k] == p[k] for k in p.dtype.names if k not in ("status", "aux")), (what, i, p, f)
        else:
            assert f == p, (what, i, p, f)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_the_flag_changes_no_byte_of_a_standalone_call(L, name):
    import torch
    kw = SPECS[name][0]
    arrays = spec_arrays(name)
    st = U.Staged(L, arrays)
    plain_cfg, flag_cfg = G.make_config(enable_8_bit=True, **kw), G.make_config(enable_8_bit=True, verify=True, **kw)
    code_p, res_p, dres_p, slots_p = std_call(L, st, plain_cfg, True)
    assert (res_p["status"] == 0).sum() >= len(arrays) - len(SPECS[name][1])   # (Conv1: a chunk shorter than the order is refused on the device)
    s = torch.cuda.Stream()
    for sync, stream in ((True, None), (False, s), (True, s)):
        code_f, res_f, dres_f, slots_f = std_call(L, st, flag_cfg, sync, stream)
        assert code_f == (code_p if sync else G.PcoSuccess)
        assert np.array_equal(slots_f, slots_p), "the flag changed a byte of the dst area"
        assert_flag_only_adds_the_bit(dres_p, dres_f, (name, sync))
        if sync:
            assert np.array_equal(res_f, dres_f)
        assert np.array_equal(st.src.cpu().numpy(), st.host_in), "src was written"
    if name == "consecutive1":
        assert dres_p["aux"][-1] == 1 and dres_f["aux"][-1] == 1 | 2, "the incompressible chunk fell back, and verifies"


def wrapped_call(c, cfg, sync, stream=None):
    import torch
    c.cfg = cfg
    c.slots.fill_(0xff); c.d_infos.zero_(); c.infos[:] = 0; torch.cuda.synchronize()
    code = c.encode(sync=sync, stream=stream)
    torch.cuda.synchronize()
    return code, (c.infos.copy() if sync else None), c.device_infos(), c.slots.cpu().numpy().copy()


@pytest.mark.parametrize("name", sorted(SPECS))
def test_the_flag_changes_no_byte_of_a_wrapped_call(L, name):
    import torch
    kw, types, _ = SPECS[name]
    arrays = [nums(t, 1000, 7 * i + j) for i, t in enumerate(types) for j in range(2)]
    lists = [V.PAGES, None] * len(types)   # Exact pages beside EqualPagesUpTo(256)
    plain_cfg, flag_cfg = G.make_config(enable_8_bit=True, max_page_n=256, **kw), G.make_config(enable_8_bit=True, max_page_n=256, verify=True, **kw)
    c = Call(L, arrays, plain_cfg, lists)
    code_p, infos_p, dinfos_p, slots_p = wrapped_call(c, plain_cfg, True)
    assert np.array_equal(infos_p, dinfos_p)
    s = torch.cuda.Stream()
    for sync, stream in ((True, None), (False, s)):
        code_f, infos_f, dinfos_f, slots_f = wrapped_call(c, flag_cfg, sync, stream)
        assert code_f == (code_p if sync else G.PcoSuccess)
        assert np.array_equal(slots_f, slots_p), "the flag changed a byte of the dst area"
        assert_flag_only_adds_the_bit(dinfos_p, dinfos_f, (name, sync))
        if sync:
            assert np.array_equal(infos_f, dinfos_f)
        assert np.array_equal(c.src.cpu().numpy(), c.host_in), "src was written"
    # without d_infos the synchronous call keeps its directory in the workspace
    c.cfg = flag_cfg; c.infos[:] = 0
    assert c.encode(sync=True, d_infos=False) == code_p
    assert np.array_equal(c.infos, dinfos_f)
    if name != "conv1":   # (the Exact chunks have a page of one number, shorter than the order: refused, and left as they are)
        assert (dinfos_f["status"] == 0).all() and (dinfos_f["aux"] & 2 == 2).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the verify entry point over one encode's chunks and any sources
# ---------------------------------------------------------------------------------------------------------------------------------------
def verify(L, tasks, d_encoded, sync=True, d_results=None, stream=None):
    """pco_gfx_verify_chunks: (code, results): the host's (sync) or, after a synchronisation, the device's"""
    import torch
    k = len(tasks)
    res = np.zeros(k, U.RES_DT)
    if d_results is None:
        d_results = torch.zeros(max(k, 1) * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
    code = L.pco_gfx_verify_chunks(k, U.ptr(tasks), d_encoded.data_ptr(), U.ptr(res) if sync else None, d_results.data_ptr(), handle(stream))
    torch.cuda.synchronize()
    dev = d_results.cpu().numpy()[: k * U.RES_DT.itemsize].view(U.RES_DT).copy()
    if sync:
        assert np.array_equal(res, dev)
    return code, dev


def encoded(L, arrays, kw):
    """`arrays` encoded WITHOUT the flag: (Staged, the encode's results)"""
    import torch
    st = U.Staged(L, arrays)
    cfg = G.make_config(enable_8_bit=True, **kw)
    tasks = st.enc_tasks()
    G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(cfg), None, st.d_res.data_ptr(), None))
    torch.cuda.synchronize()
    res = st.results()
    assert (res["status"] == 0).all()
    return st, res


def corrupt(at):
    return (0, at, G.ST_CORRUPTION)


def verdicts(res):
    return [(int(r["n_out"]), int(r["consumed"]), int(r["status"])) for r in res]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. bit patterns
# ---------------------------------------------------------------------------------------------------------------------------------------
def special_floats(name):
    """1000 floats among which NaNs of several payloads, both zeros, both infinities and subnormals, by bit pattern; (array, index of a -0.0, index of a NaN)"""
    f = np.dtype(name); u = np.dtype(f"u{f.itemsize}"); bits = 8 * f.itemsize
    mant = {16: 10, 32: 23, 64: 52}[bits]
    exp_ones = ((1 << (bits - 1 - mant)) - 1) << mant
    sign = 1 << (bits - 1)
    a = nums(name, 1000, 5).view(u).copy()
    specials = [exp_ones | 1, exp_ones | (1 << (mant - 1)), exp_ones | (1 << (mant - 1)) | 5, sign | exp_ones | 3,   # NaNs: signalling, quiet, payloads, negative
                sign, 0, exp_ones, sign | exp_ones, 1, sign | 2, (1 << mant) - 1]                                   # -0.0, +0.0, +inf, -inf, subnormals
    for j, s in enumerate(specials * 3):
        a[17 + 29 * j] = s
    neg_zero, nan = 17 + 29 * 4, 17 + 29 * 2
    assert a[neg_zero] == sign and a[nan] == exp_ones | (1 << (mant - 1)) | 5
    return a.view(f), neg_zero, nan


def test_special_floats_verify_and_one_changed_bit_pattern_does_not(L):
    import torch
    made = [special_floats(t) for t in FLOATS]
    arrays = [m[0] for m in made]
    st = U.Staged(L, arrays)
    code, _, res, _ = std_call(L, st, G.make_config(mode=1, delta=1, verify=True), True)
    assert code == G.PcoSuccess and (res["status"] == 0).all() and (res["aux"] & 2 == 2).all()
    st.d_res.copy_(torch.from_numpy(res.view(np.uint8).copy()))   # (the verify below reads the encode's results from there)
    # the same chunks against sources with ONE bit pattern changed: -0.0 -> +0.0, then a NaN's payload
    for which, change in ((1, lambda u, i: 0), (2, lambda u, i: int(u[i]) ^ 4)):
        host = st.host_in.copy()
        want = []
        for a, o, m in zip(arrays, st.in_off, made):
            u = host[o: o + a.nbytes].view(f"u{a.dtype.itemsize}")
            u[m[which]] = change(u, m[which])
            want.append(corrupt(m[which]))
            assert (a.view(u.dtype) != u).sum() == 1
        if which == 1:
            assert all(np.array_equal(host[o: o + a.nbytes].view(a.dtype), a, equal_nan=True) for a, o in zip(arrays, st.in_off)), "as floats the two compare equal"
        src = torch.from_numpy(host).cuda()
        code, got = verify(L, st.enc_tasks(src=src), st.d_res)
        assert code == G.PcoCompressionError and L.pco_gfx_last_status() == G.ST_CORRUPTION
        assert verdicts(got) == want and (got["aux"] == 0).all()
    code, got = verify(L, st.enc_tasks(), st.d_res)
    assert code == G.PcoSuccess and np.array_equal(got, res)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. damaged chunks
# ---------------------------------------------------------------------------------------------------------------------------------------
def expectation(want):
    return corrupt(want[1]) if want[0] == "differs" else corrupt(ONES)


def test_damaged_standalone_chunks_give_the_outcome_the_oracle_certified(L):
    import torch
    a = V.numbers()
    names = sorted(V.STANDALONE_CASES)
    st, res = encoded(L, [a] * (1 + len(names)), V.SPEC)
    chunks = st.slot_bytes(res["n_out"])
    assert all(c == U.oracle_chunk(a, O.make_config(**V.SPEC)) for c in chunks), "the positions of tests/verify_util.py are the oracle's chunk's"
    damaged = st.put_chunks([chunks[0]] + [V.STANDALONE_CASES[n][0](c) for n, c in zip(names, chunks[1:])])   # a copy of dst, edited
    want = [(int(res["n_out"][0]), 0, 0)] + [expectation(V.STANDALONE_CASES[n][1]) for n in names]
    before = damaged.cpu().numpy().copy()
    s = torch.cuda.Stream()
    for sync, stream in ((True, None), (False, s)):
        code, got = verify(L, st.enc_tasks(slots=damaged), st.d_res, sync, stream=stream)
        assert code == (G.PcoCompressionError if sync else G.PcoSuccess)
        assert verdicts(got) == want, list(zip(["undamaged"] + names, verdicts(got)))
        assert got["aux"].tolist() == [2] + [0] * len(names)
    assert np.array_equal(damaged.cpu().numpy(), before) and np.array_equal(st.results(), res), "a verify writes neither the chunks nor, unaliased, the encode's results"


def test_damaged_wrapped_chunks_give_the_outcome_the_oracle_certified(L):
    import torch
    a = V.numbers()
    names = sorted(V.WRAPPED_CASES)
    k = 1 + len(names)
    cfg = G.make_config(**V.SPEC)
    c = Call(L, [a] * k, cfg, [V.PAGES] * k)
    G.check(c.encode())
    meta, pages, _ = O.wrapped_compress(a, O.make_config(**V.SPEC), exact_pages=V.PAGES)
    assert all(p[0] == meta and p[1] == pages for p in c.pieces()), "the positions of tests/verify_util.py are the oracle's pieces'"
    host = c.slots.cpu().numpy().copy()
    want_status = np.zeros((k, 4), np.uint32)   # per chunk: the ChunkMeta's piece, then the three pages
    for i, n in enumerate(names, 1):
        piece, damage, want = V.WRAPPED_CASES[n]
        e = c.infos[c.piece_first[i] + piece]
        at = int(c.slot_off[i]) + int(e["offset"])
        host[at: at + int(e["len"])] = np.frombuffer(damage(host[at: at + int(e["len"])].tobytes()), np.uint8)
        want_status[i, 0] = G.ST_CORRUPTION
        want_status[i, 1:] = G.ST_CORRUPTION if piece == 0 else 0
        if piece:
            want_status[i, piece] = G.ST_CORRUPTION
    damaged = torch.from_numpy(host).cuda()   # a copy of dst, edited
    tasks = c.make_tasks({i: dict(dst=damaged.data_ptr() + int(c.slot_off[i])) for i in range(k)})
    s = torch.cuda.Stream()
    for sync, stream in ((True, None), (False, s)):
        infos = np.zeros(c.n_pieces, INFO_DT)
        d_out = torch.zeros(c.n_pieces * INFO_DT.itemsize, dtype=torch.uint8, device="cuda")
        code = L.pco_gfx_verify_wrapped_chunks(k, tasks, C.addressof(cfg), c.d_infos.data_ptr(), U.ptr(infos) if sync else None, d_out.data_ptr(), handle(stream))
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(INFO_DT)
        assert code == (G.PcoCompressionError if sync else G.PcoSuccess)
        if sync:
            assert np.array_equal(infos, got)
        assert got["status"].reshape(k, 4).tolist() == want_status.tolist()
        assert (got["aux"] == np.where(got["status"] == 0, 2, 0)).all()
        assert all(np.array_equal(got[f], c.infos[f]) for f in ("offset", "len", "n")), "a wrapped piece reports status and aux only"
    assert np.array_equal(damaged.cpu().numpy(), host) and np.array_equal(c.device_infos(), c.infos)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. alignment and tails of the compare kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def positions(n, w):
    """where one number is changed, in turn: index 0, inside the unaligned head, the first and the last aligned vector, the tail, n - 1 (the source starts
    one number behind a 16-byte boundary, so its first boundary is at index 16 / w - 1)"""
    per = 16 // w
    vectors = n * w // 16
    want = {0, max(per - 2, 0), per - 1, per, (vectors - 1) * per, vectors * per - 1, min(vectors * per, n - 1), n - 1}
    return sorted(p for p in want if 0 <= p < n)


@pytest.mark.parametrize("name", ["uint8", "uint16", "uint32", "uint64"])
def test_the_compare_kernel_finds_the_first_difference_at_every_alignment_and_tail(L, name):
    import torch
    w = np.dtype(name).itemsize
    arrays = [nums(name, 1024 // w + r, r) for r in range(16 // w)]   # n * w mod 16 through every residue the width allows
    st, res = encoded(L, arrays, dict(mode=1, delta=1))
    # one task per (chunk, changed position), and per chunk one with two changes and one unchanged; every source one number behind a 16-byte boundary
    plan = [(i, (p,)) for i, a in enumerate(arrays) for p in positions(a.size, w)]
    plan += [(i, (a.size // 3, a.size - 1)) for i, a in enumerate(arrays)] + [(i, ()) for i in range(len(arrays))]
    stride = (max(a.nbytes for a in arrays) + w + 15) // 16 * 16
    host = np.zeros(stride * len(plan) + 64, np.uint8)
    tasks = np.zeros(len(plan), U.ENC_DT)
    enc = st.enc_tasks()
    for t, (i, changed) in enumerate(plan):
        a = arrays[i].copy()
        for p in changed:
            a[p] ^= 1
        host[t * stride + w: t * stride + w + a.nbytes] = a.view(np.uint8)
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    for t, (i, changed) in enumerate(plan):
        tasks[t] = enc[i]
        tasks[t]["src"] = src.data_ptr() + t * stride + w
    d_enc = torch.from_numpy(res[[i for i, _ in plan]].view(np.uint8).copy()).cuda()
    code, got = verify(L, tasks, d_enc)
    want = [corrupt(min(changed)) if changed else (int(res["n_out"][i]), 0, 0) for i, changed in plan]
    assert verdicts(got) == want, [(plan[t], verdicts(got)[t], want[t]) for t in range(len(plan)) if verdicts(got)[t] != want[t]]
    assert code == G.PcoCompressionError


def test_a_difference_in_the_last_piece_of_a_long_chunk_and_in_the_first_and_the_last(L):
    import torch
    n = 1 << 20   # 4 MiB of u32: 64 pieces of the compare kernel
    a = (np.arange(n, dtype=np.uint32) * 7 + np.random.default_rng(3).integers(0, 64, n).astype(np.uint32))
    st, res = encoded(L, [a], dict(mode=1, delta=2, delta_order=1))
    for changed in ((n - 5,), (3, n - 5), (70000, 70001, n - 1)):
        b = a.copy()
        for p in changed:
            b[p] ^= 0x80000000
        code, got = verify(L, st.enc_tasks(src=torch.from_numpy(b.view(np.uint8)).cuda()), st.d_res)
        assert verdicts(got) == [corrupt(min(changed))]
    code, got = verify(L, st.enc_tasks(), st.d_res)
    assert code == G.PcoSuccess and verdicts(got) == [(int(res["n_out"][0]), 0, 0)] and got["aux"][0] == 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. isolation
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_damaged_chunks_among_65_and_a_task_that_was_not_encoded(L):
    import torch
    types = INTS + FLOATS
    arrays = [nums(types[i % len(types)], SIZES[i % len(SIZES)], i) for i in range(65)]
    arrays[3] = V.numbers(); arrays[64] = V.numbers(); arrays[10] = V.numbers()
    st, res = encoded(L, arrays, V.SPEC)
    chunks = st.slot_bytes(res["n_out"])
    chunks[3] = V.flip_offset(chunks[3], V.N, 300); chunks[64] = V.flip_offset(chunks[64], V.N, 5)
    damaged = st.put_chunks(chunks)
    code, got = verify(L, st.enc_tasks(slots=damaged), st.d_res)
    want = [(int(r["n_out"]), 0, 0) for r in res]
    want[3] = corrupt(300); want[64] = corrupt(5)
    assert verdicts(got) == want and got["aux"].tolist() == [0 if i in (3, 64) else 2 for i in range(65)]
    # task 10's dst holds a canary pattern.  Under its own OK result it decodes, to Corruption; under a result that says it was never encoded it
    # is left alone, word for word
    host = damaged.cpu().numpy().copy()
    host[st.slot_off[10]: st.slot_off[10] + st.caps[10]] = 0xA5
    canary = torch.from_numpy(host).cuda()
    code, got = verify(L, st.enc_tasks(slots=canary), st.d_res)
    assert got[10]["status"] == G.ST_CORRUPTION and got[10]["n_out"] == 0, "the canary pattern does not pass for a chunk"
    stale = res.copy()
    stale[10] = (123, 456, G.ST_INVALID_ARGUMENT, 1)
    d_enc = torch.from_numpy(stale.view(np.uint8).copy()).cuda()
    for sync in (True, False):
        code, got = verify(L, st.enc_tasks(slots=canary), d_enc, sync)
        assert tuple(got[10]) == (123, 456, G.ST_INVALID_ARGUMENT, 1)
        assert verdicts(np.delete(got, 10)) == [w for i, w in enumerate(want) if i != 10]
    # a result that names more bytes than the dst holds: refused, nothing of it is read
    stale[10] = (int(st.caps[10]), 0, 0, 0)
    code, got = verify(L, st.enc_tasks(slots=canary), torch.from_numpy(stale.view(np.uint8).copy()).cuda())
    assert verdicts(got)[10] == corrupt(ONES)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. pipelines: encode -> damage -> verify -> compact -> decode, one synchronisation at the end
# ---------------------------------------------------------------------------------------------------------------------------------------
def flip_on_device(torch, stream, tensor, at):
    with torch.cuda.stream(stream):
        tensor[at: at + 1].bitwise_xor_(1)


def test_a_standalone_pipeline_drops_the_two_chunks_that_do_not_verify(L):
    import torch
    arrays = [V.numbers() + np.uint32(0) for _ in range(3)] + [nums("int64", 4097, 1), nums("float32", 257, 2), V.numbers(), nums("uint16", 1000, 3)]
    k = len(arrays); bad = (1, 5)
    st = U.Staged(L, arrays)
    cfg = G.make_config(**V.SPEC)
    tasks = U.pinned(st.enc_tasks())
    s = torch.cuda.Stream()
    cap = int(st.slot_off[-1])
    with torch.cuda.stream(s):
        blob = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda"); offsets = torch.zeros(k + 1, dtype=torch.int64, device="cuda")
        out = torch.zeros(st.host_in.size, dtype=torch.uint8, device="cuda"); d_dec = torch.zeros(k * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
    G.check(L.pco_gfx_compress_chunks(k, U.ptr(tasks), C.byref(cfg), None, st.d_res.data_ptr(), handle(s)))
    chunk_len = len(U.oracle_chunk(arrays[1], O.make_config(**V.SPEC)))   # (host arithmetic: where number 300's offset lies in chunks 1 and 5)
    for i in bad:
        flip_on_device(torch, s, st.slots, int(st.slot_off[i]) + chunk_len - 2 * V.N + 2 * 300)
    G.check(L.pco_gfx_verify_chunks(k, U.ptr(tasks), st.d_res.data_ptr(), None, st.d_res.data_ptr(), handle(s)))   # d_results aliases d_encoded
    G.check(L.pco_gfx_compact_chunks(k, U.ptr(tasks), st.d_res.data_ptr(), blob.data_ptr(), cap, 0, offsets.data_ptr(), None, handle(s)))
    directory = G.Directory(blob.data_ptr(), cap, offsets.data_ptr(), k, 0, 0)
    dtasks = (G.DirChunkTask * k)(*[G.DirChunkTask(out.data_ptr() + int(st.in_off[i]), arrays[i].size, i, i, int(st.dtb[i]), 4) for i in range(k)])
    G.check(L.pco_gfx_decompress_chunks_dir(k, dtasks, C.addressof(directory), None, d_dec.data_ptr(), handle(s)))
    s.synchronize()
    res = st.results(); offs = offsets.cpu().numpy(); dec = d_dec.cpu().numpy().view(U.RES_DT)
    assert verdicts(res[list(bad)]) == [corrupt(300)] * 2
    assert all(offs[i] == offs[i + 1] for i in bad) and all(offs[i + 1] - offs[i] == res["n_out"][i] > 0 for i in range(k) if i not in bad)
    assert all(dec["status"][i] == (G.ST_INSUFFICIENT_DATA if i in bad else 0) for i in range(k))
    assert sorted(st.outputs_equal(out)) == list(bad), "every kept chunk decodes to its input; the dropped ones wrote nothing"


def test_a_wrapped_pipeline_drops_the_chunk_with_one_bad_page(L):
    import torch
    arrays = [V.numbers(), nums("int64", 1000, 1), V.numbers(), nums("float32", 1000, 2)]
    k = len(arrays); bad = 2
    cfg = G.make_config(**V.SPEC)
    c = Call(L, arrays, cfg, [V.PAGES] * k)
    s = torch.cuda.Stream()
    cap = int(c.slot_off[-1])
    with torch.cuda.stream(s):
        blob = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda"); offsets = torch.zeros(c.n_pieces + 1, dtype=torch.int64, device="cuda")
        d_dec = torch.zeros(3 * k * U.RES_DT.itemsize, dtype=torch.uint8, device="cuda")
    assert c.encode(sync=False, stream=s) == G.PcoSuccess
    # the last page of chunk 2 ends where the oracle's does: offset of its piece (host arithmetic over the caps) + its length
    meta, pages, _ = O.wrapped_compress(arrays[bad], O.make_config(**V.SPEC), exact_pages=V.PAGES)
    page_off = L.pco_gfx_wrapped_chunk_cap_exact(c.keep[bad], 3, c.dtb[bad], C.addressof(cfg)) - (L.pco_gfx_guarantee_chunk_size(V.PAGES[2], c.dtb[bad]) + 64 + 15) // 16 * 16
    flip_on_device(torch, s, c.slots, int(c.slot_off[bad]) + page_off + len(pages[2]) - 2 * V.PAGES[2] + 2 * 100)
    G.check(L.pco_gfx_verify_wrapped_chunks(k, c.tasks, C.addressof(cfg), c.d_infos.data_ptr(), None, c.d_infos.data_ptr(), handle(s)))
    G.check(L.pco_gfx_compact_wrapped_chunks(k, c.tasks, C.addressof(cfg), c.d_infos.data_ptr(), 0, blob.data_ptr(), cap, 0, offsets.data_ptr(), None, handle(s)))
    directory = G.Directory(blob.data_ptr(), cap, offsets.data_ptr(), c.n_pieces, 0, 0)
    dt = []
    for i, a in enumerate(arrays):
        start = 0
        for p, n in enumerate(V.PAGES):
            dt.append(G.DirPageTask(c.out.data_ptr() + int(c.in_off[i]) + start * a.dtype.itemsize, n, 4 * i, 4 * i + 1 + p, c.dtb[i], 4)); start += n
    G.check(L.pco_gfx_decompress_pages_dir(len(dt), (G.DirPageTask * len(dt))(*dt), C.addressof(directory), None, d_dec.data_ptr(), handle(s)))
    s.synchronize()
    infos = c.device_infos(); offs = offsets.cpu().numpy(); dec = d_dec.cpu().numpy().view(U.RES_DT)
    assert infos["status"].reshape(k, 4).tolist() == [[0] * 4, [0] * 4, [1, 0, 0, 1], [0] * 4]
    assert (infos["aux"].reshape(k, 4) == np.where(infos["status"].reshape(k, 4) == 0, 2, 0)).all()
    assert len(set(offs[4 * bad: 4 * bad + 5].tolist())) == 1, "the chunk with a bad page contributes nothing"
    assert (dec["status"].reshape(k, 3) == np.array([[0] * 3, [0] * 3, [G.ST_INSUFFICIENT_DATA] * 3, [0] * 3])).all()
    host = c.out.cpu().numpy()
    for i, a in enumerate(arrays):
        same = np.array_equal(host[c.in_off[i]: c.in_off[i] + a.nbytes], c.host_in[c.in_off[i]: c.in_off[i] + a.nbytes])
        assert same == (i != bad)


def test_a_verified_standalone_encode_asks_for_the_documented_dst_cap_before_it_launches_anything(L):
    """The decode behind the encode may read 16 bytes past a chunk and the encoders fill dst to within 8 of dst_cap: under the flag a dst_cap below
    pco_gfx_guarantee_chunk_size + 16 is PCO_GFX_INVALID_ARGUMENT and nothing is written; the unflagged call takes it as before."""
    import torch
    a = nums("uint32", 1000, 1)
    st = U.Staged(L, [a], cap_extra=15)
    st.caps[0] = L.pco_gfx_guarantee_chunk_size(a.size, G.DTYPE_BYTE["uint32"]) + 15
    tasks = st.enc_tasks(); res = np.zeros(1, U.RES_DT)
    plain, flagged = G.make_config(mode=1, delta=1), G.make_config(mode=1, delta=1, verify=True)
    assert L.pco_gfx_compress_chunks(1, U.ptr(tasks), C.byref(flagged), U.ptr(res), None, None) == G.PcoCompressionError
    torch.cuda.synchronize()
    assert L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT and not st.slots.any().item() and tuple(res[0]) == (0, 0, 0, 0)
    assert L.pco_gfx_compress_chunks(1, U.ptr(tasks), C.byref(plain), U.ptr(res), None, None) == G.PcoSuccess and res[0]["n_out"] > 0
    tasks["dst_cap"] += 1
    assert L.pco_gfx_compress_chunks(1, U.ptr(tasks), C.byref(flagged), U.ptr(res), None, None) == G.PcoSuccess and res[0]["aux"] == 2


@pytest.mark.parametrize("standalone", [False, True])
def test_reading_verified_does_not_wait_for_the_stream(L, standalone):
    """`verified` behind ~60 ms of queued device work (a fixed chain of copies): the property returns while the stream is still busy."""
    import torch
    import pcodec_amd as P
    from pcodec_amd import paged
    tensors = [torch.from_numpy(nums("int64", 4097, i).view(np.uint8).copy()).cuda().view(torch.int64) for i in range(3)]
    cfg = P.ChunkConfig(verify=True, mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_consecutive(1))
    s = torch.cuda.Stream()
    compress = (lambda: paged.compress_standalone_chunks(tensors, cfg, stream=s)) if standalone else (lambda: paged.compress_chunks(tensors, cfg, stream=s))
    compress().verified   # (a first call grows the workspace and torch's pools, which may wait for the device: outside the part that counts)
    U.device_delay(s, 0)   # (likewise: allocates its two buffers and synchronises once)
    torch.cuda.synchronize()
    U.device_delay(s, 60)
    out = compress()
    v = out.verified
    busy = not s.query()
    s.synchronize()
    assert busy, "the stream had drained: reading `verified` (or the encode) waited for it"
    assert v.cpu().tolist() == [True] * 3


@pytest.mark.parametrize("standalone", [False, True])
def test_paged_verified_and_verify_chunks(L, standalone):
    import torch
    import pcodec_amd as P
    from pcodec_amd import paged
    arrays = [V.numbers(), nums("int64", 1000, 1), V.numbers(), nums("float32", 257, 2)]
    tensors = [torch.from_numpy(a.view(np.uint8).copy()).cuda().view(getattr(torch, a.dtype.name)) for a in arrays]
    spec = dict(compression_level=0, mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.no_op())
    compress = (lambda cfg, s: paged.compress_standalone_chunks(tensors, cfg, stream=s, file_frame=False)) if standalone else (lambda cfg, s: paged.compress_chunks(tensors, cfg, stream=s))
    s = torch.cuda.Stream()
    def verified(cfg):   # (`verified` is valid in the order of the call's stream, like everything the call leaves)
        v = compress(cfg, s).verified
        s.synchronize()
        return v.cpu().tolist()
    assert verified(P.ChunkConfig(**spec)) == [False] * 4, "without the flag nothing is verified"
    assert verified(P.ChunkConfig(verify=True, **spec)) == [True] * 4
    out = compress(P.ChunkConfig(**spec), s)
    # chunk 2's last number: its offset is the chunk's (the one page's) last two bytes, which end where the oracle's do
    if standalone:
        end = int(out._tasks[2].dst) - out.slots.data_ptr() + len(U.oracle_chunk(arrays[2], O.make_config(**V.SPEC)))
    else:
        meta, pages, _ = O.wrapped_compress(arrays[2], O.make_config(**V.SPEC))
        cfg = out._cfg
        end = int(out._tasks[2].dst) - out.slots.data_ptr() + L.pco_gfx_wrapped_chunk_cap(V.N, G.DTYPE_BYTE["uint32"], C.addressof(cfg)) - (L.pco_gfx_guarantee_chunk_size(V.N, G.DTYPE_BYTE["uint32"]) + 64 + 15) // 16 * 16 + len(pages[0])
    flip_on_device(torch, s, out.slots, end - 2)
    ok = paged.verify_chunks(tensors, out, stream=s)
    back, results = paged.decompress_chunks_async(out, stream=s)
    again = out.verified
    s.synchronize()
    assert ok.cpu().tolist() == [True, True, False, True] == again.cpu().tolist()
    res = results.cpu().numpy().view(U.RES_DT)
    assert res["status"].tolist() == [0, 0, G.ST_INSUFFICIENT_DATA, 0]
    for i, (a, b) in enumerate(zip(arrays, back)):
        assert U.bits_equal(a, b.cpu().numpy().view(a.dtype)) == (i != 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. passes (a child process: PCO_GFX_WORKSPACE_GB is read once, when the library is loaded)
# ---------------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], ".."))
import numpy as np
import gpu_util as U
import test_gpu_wrapped_writer as T
from pcodec_amd import _lib as G
L = G.lib()
dist = [U.synth("c2", 20000, seed=1), np.cumsum(np.random.default_rng(4).integers(-5, 6, 20000)).astype(np.int32), U.synth("c2", 15000, seed=2)]
lists = [None, [1, 9999, 10000], [7000, 8000]]
out = {}
for verify in (False, True):
    cfg = G.make_config(max_page_n=6000, verify=verify, **T.C2)
    c = T.Call(L, U.tile(dist, 200), cfg, U.tile(lists, 200))
    est = L.pco_gfx_wrapped_scratch_estimate(c.k, c.tasks, C.addressof(cfg))
    L.pco_gfx_profile_begin()
    G.check(c.encode())
    names = C.create_string_buffer(1 << 18); ms = (C.c_float * 16384)()
    nk = L.pco_gfx_profile_end(names, len(names), ms, 16384)
    kernels = names.raw.split(b"\0")[:nk]
    out["flag" if verify else "plain"] = dict(estimate=est, inits=kernels.count(b"enc_init_kernel"), compares=kernels.count(b"verify_compare_kernel"),
        slots=hashlib.sha256(c.slots.cpu().numpy().tobytes()).hexdigest(), ok=bool((c.infos["status"] == 0).all()), aux=sorted(set(c.infos["aux"].tolist())),
        same=bool(np.array_equal(c.infos, c.device_infos())))
print("RESULT " + json.dumps(out))
"""


def _child(env_gb):
    env = dict(os.environ); env.pop("PCO_GFX_WORKSPACE_GB", None); env.pop("PCO_GFX_VERIFY", None)
    if env_gb is not None:
        env["PCO_GFX_WORKSPACE_GB"] = env_gb
    r = subprocess.run([sys.executable, "-c", CHILD, HERE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_a_flagged_call_beyond_the_budget_verifies_pass_by_pass():
    """200 wrapped chunks under a budget of 0.55 x the library's own estimate for the FLAGGED call (which counts the verify's scratch and the decode's
    buffers): two passes, each verifying its own chunks -- every piece verified, the bytes those of the unflagged call."""
    whole = _child(None)
    assert whole["flag"]["estimate"] > whole["plain"]["estimate"] > 0, "the flag grows the per-chunk figure"
    assert whole["plain"]["inits"] == whole["flag"]["inits"] == 1 and whole["plain"]["compares"] == 0 and whole["flag"]["compares"] == 1
    cut = _child(repr(whole["flag"]["estimate"] * 0.55 / 1e9))
    print(f"[passes] flagged estimate {whole['flag']['estimate']} B (unflagged {whole['plain']['estimate']} B) for 200 chunks: enc_init_kernel x {cut['flag']['inits']}, "
          f"verify_compare_kernel x {cut['flag']['compares']}")
    assert cut["flag"]["inits"] == cut["flag"]["compares"] == 2, "more than one pass, each with its own verify"
    for run in (whole, cut):
        assert run["flag"]["ok"] and run["flag"]["aux"] == [2] and run["plain"]["aux"] == [0] and run["flag"]["same"]
        assert run["flag"]["slots"] == run["plain"]["slots"] == whole["plain"]["slots"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8. work: what a call launches
# ---------------------------------------------------------------------------------------------------------------------------------------
# pco_gfx_compress_chunks over 12 u64 chunks of 4097 numbers under Classic / TryConsecutive(1), synchronous, as the commit before the flag launches it
PARENT_KERNELS = ["enc_init_kernel", "enc_presample_kernel", "enc_lat_slots_kernel", "enc_split_kernel<c16>", "enc_lat_slots_kernel", "enc_hist_kernel", "enc_train_kernel",
                  "enc_dissect_kernel", "enc_vlut_kernel", "enc_walkp_kernel", "enc_walkd_kernel", "enc_scan_kernel", "enc_place+pack", "~enc_place_kernel",
                  "~enc_pack1_kernel", "~enc_pack1_kernel<wide>", "~enc_pack_kernel", "enc_page_kernel"]   # recorded from that commit's library on an MI355X


def launches(L, st, cfg, call):
    L.pco_gfx_profile_begin()
    call()
    return U.profile_launches(L)


def test_the_unflagged_call_launches_what_it_always_did_and_the_flag_adds_the_decode_and_two_kernels(L):
    import torch
    arrays = [U.synth("c2", 4097, seed=i) for i in range(12)]
    st = U.Staged(L, arrays)
    tasks = st.enc_tasks(); res = np.zeros(st.k, U.RES_DT)
    plain_cfg, flag_cfg = G.make_config(mode=1, delta=2, delta_order=1), G.make_config(mode=1, delta=2, delta_order=1, verify=True)
    plain = launches(L, st, plain_cfg, lambda: G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(plain_cfg), U.ptr(res), st.d_res.data_ptr(), None)))
    sizes = res["n_out"].copy()
    assert plain == PARENT_KERNELS
    flagged = launches(L, st, flag_cfg, lambda: G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(flag_cfg), U.ptr(res), st.d_res.data_ptr(), None)))
    dres = np.zeros(st.k, U.RES_DT)
    dtasks = st.dec_tasks(sizes)
    decode = launches(L, st, None, lambda: G.check(L.pco_gfx_decompress_chunks(st.k, U.ptr(dtasks), U.ptr(dres), None, None)))
    assert decode and not any(n.startswith("verify") for n in decode)
    assert flagged == plain + ["verify_resolve_kernel"] + decode + ["verify_compare_kernel", "verify_finish_kernel"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. the host-buffer surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_simple_compress_with_verify_returns_the_bytes_of_the_unflagged_call(L):
    import pcodec_amd as P
    from pcodec_amd import standalone
    x = U.synth("c2", 5000)
    spec = dict(mode_spec=P.ModeSpec.classic(), delta_spec=P.DeltaSpec.try_consecutive(1), paging_spec=P.PagingSpec.equal_pages_up_to(2000))
    plain = standalone.simple_compress(x, P.ChunkConfig(**spec))
    L.pco_gfx_profile_begin()
    flagged = standalone.simple_compress(x, P.ChunkConfig(verify=True, **spec))
    names = U.profile_launches(L)
    assert flagged == plain == O.simple_compress(x, O.make_config(mode=1, delta=2, delta_order=1, max_page_n=2000))
    assert names.count("verify_compare_kernel") == 1 and names.count("verify_finish_kernel") == 1
    assert U.bits_equal(U.gpu_simple_decompress(flagged, x.dtype, x.size), x)


ENV_CHILD = r"""
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], ".."))
import numpy as np
import gpu_util as U
from pcodec_amd import _lib as G
L = G.lib()
x = U.synth("c2", 5000)
cap = L.pco_standalone_guarantee_file_size(x.size, 2) + 64
dst = np.zeros(cap, np.uint8); n = C.c_size_t(0)
L.pco_gfx_profile_begin()
code = L.pco_standalone_simple_compress_into(x.ctypes.data_as(C.c_void_p), x.size, 2, None, dst.ctypes.data_as(C.c_void_p), cap, C.byref(n))
names = U.profile_launches(L)
import hashlib
print("RESULT", code, names.count("verify_compare_kernel"), hashlib.sha256(dst[: n.value].tobytes()).hexdigest())
"""


def test_the_environment_variable_sets_the_flag_for_the_three_function_abi():
    runs = {}
    for value in (None, "1"):
        env = dict(os.environ); env.pop("PCO_GFX_VERIFY", None)
        if value is not None:
            env["PCO_GFX_VERIFY"] = value
        r = subprocess.run([sys.executable, "-c", ENV_CHILD, HERE], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        runs[value] = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()[1:]
    assert runs[None][0] == runs["1"][0] == "0" and runs[None][2] == runs["1"][2], "the same file either way"
    assert runs[None][1] == "0" and int(runs["1"][1]) >= 1, "the verify ran under PCO_GFX_VERIFY=1 only"
