"""GPU: resolve Auto specs once, encode later calls from per-chunk specs (include/pco_gfx.h section 3c).

The chunks of chunk_specs_util.cases() reach every Auto outcome (tests/test_chunk_specs_abi.py confirms each against the oracle on the CPU).  Their specs
are resolved once by pco_gfx_resolve_chunk_specs; every encode from them -- synchronous, asynchronous, wrapped under Exact and EqualPagesUpTo pages,
through pcodec_amd.paged -- must write the bytes the Auto call and the oracle's Auto encode write, launch exactly the explicit path's kernels and, in
its asynchronous form, return without waiting for the stream."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import chunk_specs_util as S  # noqa: E402
import gpu_util as U  # noqa: E402
import oracle_lib as O  # noqa: E402
import test_gpu_wrapped_writer as T  # noqa: E402  (Call: arrays staged for a wrapped writer call, its pieces and their decode)
from pcodec_amd import _lib as G  # noqa: E402

pytestmark = pytest.mark.gpu

AUTO_ONLY_KERNELS = ("gather_kernel", "split_gather_kernel", "auto_int_gcd_kernel", "auto_float_stats_kernel", "auto_saved_kernel", "enc_trial_summary_kernel")
NAMES = [n for n, _, _ in S.cases()]
ARRAYS = [a for _, a, _ in S.cases()]


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def auto_cfg(**kw):
    return G.make_config(enable_8_bit=True, **kw)


def fill_slots(st, byte=0xFF):
    import torch
    st.slots.fill_(byte); st.d_res.fill_(0xFF); torch.cuda.synchronize()


def resolve(L, st, cfg=None, stream=None):
    tasks = st.enc_tasks(); tasks["dst"] = 0; tasks["dst_cap"] = 0   # (ignored: may be NULL / 0)
    out = (G.ChunkSpec * st.k)()
    cfg = cfg if cfg is not None else auto_cfg()
    G.check(L.pco_gfx_resolve_chunk_specs(st.k, U.ptr(tasks), C.byref(cfg), out, stream))
    return [G.ChunkSpec.from_buffer_copy(out[i]) for i in range(st.k)]


def encode_specs(L, st, specs, cfg=None, sync=True, stream=None, check=True):
    """pco_gfx_compress_chunks_specs over the staged arrays: (results as RES_DT, [chunk bytes])"""
    import torch
    tasks = st.enc_tasks(); res = np.zeros(st.k, U.RES_DT)
    cfg = cfg if cfg is not None else auto_cfg()
    code = L.pco_gfx_compress_chunks_specs(st.k, U.ptr(tasks), C.byref(cfg), S.spec_array(specs), U.ptr(res) if sync else None, st.d_res.data_ptr(),
                                           C.c_void_p(stream.cuda_stream) if stream is not None else None)
    if check:
        G.check(code)
    torch.cuda.synchronize()
    dev = st.results()
    if sync:
        assert np.array_equal(dev, res), "the host results of a synchronous call are not its device results"
    return dev, st.slot_bytes(dev["n_out"])


def encode_config(L, st, cfg):
    """pco_gfx_compress_chunks, synchronous: (results, [chunk bytes])"""
    tasks = st.enc_tasks(); res = np.zeros(st.k, U.RES_DT)
    G.check(L.pco_gfx_compress_chunks(st.k, U.ptr(tasks), C.byref(cfg), U.ptr(res), st.d_res.data_ptr(), None))
    return res, st.slot_bytes(res["n_out"])


def decode_and_compare(L, st, sizes):
    import torch
    st.out.zero_(); torch.cuda.synchronize()
    dt = st.dec_tasks(sizes); dres = np.zeros(st.k, U.RES_DT)
    G.check(L.pco_gfx_decompress_chunks(st.k, U.ptr(dt), U.ptr(dres), None, None))
    assert (dres["status"] == 0).all() and np.array_equal(dres["n_out"], st.n) and np.array_equal(dres["consumed"], np.asarray(sizes, np.uint64))
    assert st.outputs_equal() == [], "decoded chunks differ from the input"


class Resolved:
    """The cases staged once, their Auto call's bytes, the oracle's Auto bytes and the specs resolved from them: computed once, never changed."""

    def __init__(self, L):
        self.st = U.Staged(L, ARRAYS)
        fill_slots(self.st)
        self.auto_res, self.auto = encode_config(L, self.st, auto_cfg())
        self.oracle = [U.oracle_chunk(a, O.make_config()) for a in ARRAYS]
        self.specs = resolve(L, self.st)


@pytest.fixture(scope="module")
def R(L):
    return Resolved(L)


def three_pages(n):
    return [n] if n < 3 else [n // 3, n // 3, n - 2 * (n // 3)]


class SpecCall(T.Call):
    def fill(self, byte=0xFF):
        import torch
        for o, c in zip(self.slot_off[:-1], self.caps):
            self.slots[int(o): int(o) + int(c)].fill_(byte)
        torch.cuda.synchronize()

    def encode_specs(self, specs, sync=True, stream=None):
        return self.L.pco_gfx_compress_wrapped_chunks_specs(self.k, self.tasks, C.addressof(self.cfg), S.spec_array(specs), U.ptr(self.infos) if sync else None,
                                                            self.d_infos.data_ptr(), T.handle(stream))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 0. what was resolved
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_specs_are_what_the_names_say_and_one_inverse_is_not_one_over_the_base(L, R):
    assert all(r == 0 for r in R.auto_res["status"]) and R.auto == R.oracle, [n for n, a, o in zip(NAMES, R.auto, R.oracle) if a != o]
    differs = []
    for name, a, want, s in zip(NAMES, ARRAYS, [w for _, _, w in S.cases()], R.specs):
        assert (s.mode_kind, s.delta_kind) == want and s.reserved == 0, (name, s)
        info, _ = O.inspect_first_chunk(O.simple_compress(a, O.make_config()))
        assert S.META_MODE[info.mode_kind] == s.mode_kind and S.META_DELTA[info.delta_kind] == s.delta_kind and s.delta_order == info.delta_order and s.mode_k == info.mode_k, name
        if s.mode_kind == G.MODE_TRY_INT_MULT:
            assert s.mode_base == info.mode_base_latent
        if s.mode_kind == G.MODE_TRY_FLOAT_MULT:
            assert s.mode_base == S.base_from_latent(int(info.mode_base_latent), a.dtype) and s.mode_inv != 0, name
            if not S.inv_is_one_over_base(s, a.dtype):
                differs.append(name)
        else:
            assert s.mode_inv == 0
    # the reason for mode_inv, tested and not assumed: Auto snapped an inverse that TryFloatMult(base) would not compute
    assert "f64_multiples_of_1/49" in differs and "f32_decimal_0.001" in differs, differs
    i = NAMES.index("f64_multiples_of_1/49")
    assert R.specs[i].mode_inv == S.float_bits(49.0, np.float64) and R.specs[i].mode_base == S.float_bits(1.0 / 49.0, np.float64)
    # resolving again gives the same specs; an explicit config resolves on the device machine as it does without one
    assert [S.spec_key(s) for s in resolve(L, R.st)] == [S.spec_key(s) for s in R.specs]
    got = resolve(L, R.st, G.make_config(enable_8_bit=True, mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK))
    assert all(S.spec_key(s) == (G.MODE_CLASSIC, G.DELTA_TRY_LOOKBACK, 0, 0, 0, 0, 0) for s in got)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. round trip, five ways
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_standalone_chunks_from_specs_are_the_auto_call_s_and_the_oracle_s_bytes(L, R, form):
    import torch
    st = U.Staged(L, ARRAYS)
    fill_slots(st)
    stream = torch.cuda.Stream() if form == "async" else None
    res, chunks = encode_specs(L, st, R.specs, sync=form == "sync", stream=stream)
    assert (res["status"] == 0).all() and np.array_equal(res["aux"], R.auto_res["aux"]) and np.array_equal(res["n_out"], R.auto_res["n_out"])
    for name, got, auto, want in zip(NAMES, chunks, R.auto, R.oracle):
        assert got == auto == want, name
    host = st.slots.cpu().numpy()
    for o, n, cap in zip(st.slot_off[:-1], res["n_out"], st.caps):   # behind a chunk and the encoder's 8 bytes of slack the fill is intact
        assert (host[int(o) + int(n) + 8: int(o) + int(cap)] == 0xFF).all()
    decode_and_compare(L, st, res["n_out"])


@pytest.mark.parametrize("paging", ["three_exact_pages", "equal_pages_up_to_5000"])
@pytest.mark.parametrize("form", ["sync", "async"])
def test_wrapped_chunks_from_specs_are_the_auto_call_s_and_the_oracle_s_pieces(L, R, paging, form):
    import torch
    lists = [three_pages(a.size) for a in ARRAYS] if paging == "three_exact_pages" else None
    cfg = auto_cfg(max_page_n=0 if lists else 5000)
    auto = SpecCall(L, ARRAYS, cfg, lists); auto.fill()
    G.check(auto.encode())
    want = auto.pieces()
    c = SpecCall(L, ARRAYS, cfg, lists); c.fill()
    stream = torch.cuda.Stream() if form == "async" else None
    G.check(c.encode_specs(R.specs, sync=form == "sync", stream=stream))
    torch.cuda.synchronize()
    if form == "sync":
        assert np.array_equal(c.device_infos(), c.infos)
    c.infos = c.device_infos()
    assert np.array_equal(c.infos, auto.infos)
    got = c.pieces()
    for name, a, g, w, pl in zip(NAMES, ARRAYS, got, want, c.pages):
        assert g == w, name
        o = O.wrapped_compress(a, O.make_config(max_page_n=0 if lists else 5000), max_pages=len(pl) + 1, exact_pages=pl if lists else None)
        assert g == (o[0], o[1], o[2]), name
    c.decode_and_compare()


def test_paged_with_specs_writes_the_same_blob_as_the_auto_config(L, R):
    import torch
    import pcodec_amd as P
    from pcodec_amd import paged
    tensors = [torch.from_numpy(a.view(np.uint8).copy()).cuda().view(getattr(torch, a.dtype.name)) for a in ARRAYS]
    assert [S.spec_key(s) for s in paged.resolve_specs(tensors)] == [S.spec_key(s) for s in R.specs]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    config = P.ChunkConfig(paging_spec=P.PagingSpec.equal_pages_up_to(5000))
    out = paged.compress_chunks(tensors, config, stream=stream, specs=R.specs)
    auto = paged.compress_chunks(tensors, config, stream=stream)
    assert out.total == auto.total and out.directory == auto.directory
    assert torch.equal(out.blob[: out.total], auto.blob[: auto.total])
    back = paged.decompress_chunks(out.blob, out.directory, [a.dtype.name for a in ARRAYS], stream=stream)
    for a, b in zip(ARRAYS, back):
        assert U.bits_equal(a, b.cpu().numpy().view(a.dtype))
    # standalone chunks: the framed blob is the file of the Auto chunks
    sc = paged.compress_standalone_chunks(tensors, stream=stream, specs=R.specs)
    f = sc.file.cpu().numpy().tobytes()
    assert f[sc.header_len:-1] == b"".join(R.oracle)
    # a single spec for all: every chunk under it
    u32 = [i for i, a in enumerate(ARRAYS) if a.dtype == np.uint32]
    assert len(u32) >= 2
    one = paged.compress_standalone_chunks([tensors[i] for i in u32], specs=S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=1), file_frame=False)
    want = b"".join(U.oracle_chunk(ARRAYS[i], O.make_config(mode=O.MODE_CLASSIC, delta=O.DELTA_TRY_CONSECUTIVE, delta_order=1)) for i in u32)
    assert one.file.cpu().numpy().tobytes() == want
    assert paged.spec_from_meta(O.wrapped_compress(ARRAYS[0], O.make_config())[0], ARRAYS[0].dtype) == S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. one mixed call
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_shuffled_call_gives_every_chunk_the_bytes_of_its_own_explicit_call(L, R):
    order = np.random.default_rng(5).permutation(len(ARRAYS))
    assert not np.array_equal(order, np.arange(len(ARRAYS)))
    arrays = [ARRAYS[i] for i in order]; specs = [R.specs[i] for i in order]
    st = U.Staged(L, arrays); fill_slots(st)
    res, chunks = encode_specs(L, st, specs)
    assert (res["status"] == 0).all()
    n_exact = 0
    for j, i in enumerate(order):
        assert chunks[j] == R.oracle[i], NAMES[i]   # (a snapped inverse included: the oracle's Auto bytes)
        if S.inv_is_one_over_base(specs[j], arrays[j].dtype):   # the explicit config says all the spec says
            cfg, ocfg = S.configs_of_spec(specs[j], arrays[j].dtype)
            one = U.Staged(L, [arrays[j]]); fill_slots(one)
            r1, c1 = encode_config(L, one, cfg)
            assert r1["status"][0] == 0 and chunks[j] == c1[0] == U.oracle_chunk(arrays[j], ocfg), NAMES[i]
            n_exact += 1
    assert 0 < n_exact < len(ARRAYS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. stale specs
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_stale_specs_cost_compression_never_correctness(L, R):
    """specs resolved on data A applied to data B of another distribution: B decodes bit for bit and the bytes are the oracle's explicit-spec encode of B"""
    r = np.random.default_rng(77)
    spec_of = {n: s for n, s in zip(NAMES, R.specs)}
    pairs = [
        ("f64_decimal_0.01", r.normal(0.0, 1.0, 3001)),                                           # a FloatMult base that no longer fits
        ("f32_decimal_0.01", r.normal(0.0, 1e6, 2050).astype(np.float32)),
        ("i64_periodic", r.integers(-(1 << 62), 1 << 62, 4097).astype(np.int64)),               # Lookback on random data
        ("u64_ramp", r.integers(0, 1 << 63, 1000).astype(np.uint64)),                           # Consecutive on random data
        ("i32_multiples_of_1000", (r.integers(-(1 << 20), 1 << 20, 5000) * 7 + 3).astype(np.int32)),   # an IntMult base that divides nothing
        ("f32_quantised", r.normal(0.0, 1.0, 2000).astype(np.float32)),                          # FloatQuant k on full mantissas
        ("u32_random", np.arange(3000, dtype=np.uint32) * 3),                                     # Classic / NoOp on a ramp
    ]
    arrays = [b for _, b in pairs]; specs = [spec_of[n] for n, _ in pairs]
    for s, b in zip(specs, arrays):
        assert S.inv_is_one_over_base(s, b.dtype)   # (so that an explicit config of the oracle says the same)
    # ... and an f16 FloatMult spec nobody resolved, on the f16 column
    arrays.append(ARRAYS[NAMES.index("f16_decimal_0.01")]); specs.append(S.spec(mode=G.MODE_TRY_FLOAT_MULT, base=0x211F))
    st = U.Staged(L, arrays); fill_slots(st)
    res, chunks = encode_specs(L, st, specs)
    assert (res["status"] == 0).all()
    for (name, _), b, s, got in zip(pairs + [("f16 TryFloatMult(0.01)", None)], arrays, specs, chunks):
        assert got == U.oracle_chunk(b, S.configs_of_spec(s, b.dtype)[1]), name
    lb = [n for n, _ in pairs].index("i64_periodic")
    assert res["aux"][lb] & 1, "Lookback on random data should fall back to the uncompressed-equivalent chunk"
    decode_and_compare(L, st, res["n_out"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the work
# ---------------------------------------------------------------------------------------------------------------------------------------
def launches(L, f):
    import torch
    torch.cuda.synchronize()
    L.pco_gfx_profile_begin()
    f()
    return U.profile_launches(L)


@pytest.mark.parametrize("kind", ["c1", "c2", "c3", "c4"])
def test_a_specs_call_launches_the_explicit_call_s_kernels_in_order(L, kind):
    cfg, _ = U.cfg_pair(kind)
    arrays = [U.synth(kind, 5000 + 100 * i, seed=i) for i in range(3)]
    st = U.Staged(L, arrays); fill_slots(st)
    specs = resolve(L, st, cfg)   # (explicit: no launch)
    encode_config(L, st, cfg); want_bytes = st.slots.cpu().numpy().copy()   # (warm: first-use allocations are not launches, but keep both sides alike)
    want = launches(L, lambda: encode_config(L, st, cfg))
    fill_slots(st)
    got = launches(L, lambda: encode_specs(L, st, specs))
    assert got == want and len(want) > 3, (got, want)
    assert not set(got) & set(AUTO_ONLY_KERNELS)
    assert np.array_equal(st.slots.cpu().numpy(), want_bytes), "the specs call's slots differ from the explicit call's"
    # the wrapped surface likewise
    c = SpecCall(L, arrays, G.make_config(enable_8_bit=True, max_page_n=2000, mode=cfg.mode_kind, mode_f64=cfg.mode_f64, delta=cfg.delta_kind, delta_order=cfg.delta_order))
    G.check(c.encode())
    want = launches(L, lambda: G.check(c.encode()))
    c.cfg = auto_cfg(max_page_n=2000)
    got = launches(L, lambda: G.check(c.encode_specs(specs)))
    assert got == want and not set(got) & set(AUTO_ONLY_KERNELS)


def test_no_specs_call_launches_a_resolution_kernel_and_resolve_launches_nothing_of_the_final_encode(L, R):
    st = U.Staged(L, ARRAYS); fill_slots(st)
    encode_config(L, st, auto_cfg())
    auto = launches(L, lambda: encode_config(L, st, auto_cfg()))
    res = launches(L, lambda: resolve(L, st))
    enc = launches(L, lambda: encode_specs(L, st, R.specs))
    assert not set(enc) & set(AUTO_ONLY_KERNELS) and len(enc) > 3
    # the Auto call is the resolution followed by the final encode: its list minus the final encode's kernels is the resolve's
    assert auto == res + enc, (auto, res, enc)
    assert len(res) > 3, "the resolution of these chunks launches trial encodes"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the asynchronous form: encode(specs) -> compact -> directory decode on one stream, one synchronisation at the end
# ---------------------------------------------------------------------------------------------------------------------------------------
def pipeline(L, R, cfg, specs):
    import torch
    st = U.Staged(L, ARRAYS); fill_slots(st)
    tasks = st.enc_tasks()
    stream = torch.cuda.Stream(); sh = C.c_void_p(stream.cuda_stream)
    cap = int(st.caps.sum())
    blob = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device="cuda"); offs = torch.zeros(st.k + 1, dtype=torch.int64, device="cuda")
    d_dres = torch.full((st.k * U.RES_DT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    rec = (G.DirChunkTask * st.k)(*[G.DirChunkTask(st.out.data_ptr() + int(st.in_off[i]), int(st.n[i]), i, i, int(st.dtb[i]), 4) for i in range(st.k)])
    d = G.Directory(blob.data_ptr(), cap, offs.data_ptr(), st.k, 0, 0)
    sa = S.spec_array(specs)
    torch.cuda.synchronize()
    U.device_delay(stream, 60)   # (the three calls below return while the stream is still busy: none of them waits for it)
    G.check(L.pco_gfx_compress_chunks_specs(st.k, U.ptr(tasks), C.byref(cfg), sa, None, st.d_res.data_ptr(), sh))
    G.check(L.pco_gfx_compact_chunks(st.k, U.ptr(tasks), st.d_res.data_ptr(), blob.data_ptr(), cap, 0, offs.data_ptr(), None, sh))
    G.check(L.pco_gfx_decompress_chunks_dir(st.k, rec, C.addressof(d), None, d_dres.data_ptr(), sh))
    busy = not stream.query()
    stream.synchronize()   # the one synchronisation
    return st, st.results(), st.results(d_dres), blob.cpu().numpy(), offs.cpu().numpy(), busy


def test_encode_from_specs_compact_and_decode_are_one_stream_ordered_pipeline(L, R):
    pipeline(L, R, auto_cfg(), R.specs)   # (warm: the workspace's first allocations synchronise the device)
    st, enc, dec, blob, offs, busy = pipeline(L, R, auto_cfg(), R.specs)
    assert busy, "the stream drained before the three calls returned: one of them waited for it"
    assert (enc["status"] == 0).all() and (dec["status"] == 0).all() and np.array_equal(dec["n_out"], st.n)
    assert st.outputs_equal() == []
    assert blob[: int(offs[-1])].tobytes() == b"".join(R.oracle) and (enc["aux"] & G.AUX_VERIFIED == 0).all()


def test_the_pipeline_with_verify_marks_every_chunk_and_changes_no_byte(L, R):
    plain = U.Staged(L, ARRAYS); fill_slots(plain)
    encode_specs(L, plain, R.specs, sync=False)
    want = plain.slots.cpu().numpy()
    cfg = auto_cfg(verify=True)
    pipeline(L, R, cfg, R.specs)
    st, enc, dec, blob, offs, busy = pipeline(L, R, cfg, R.specs)
    assert busy, "the verified specs call waited for the stream"
    assert (enc["status"] == 0).all() and (enc["aux"] & G.AUX_VERIFIED == G.AUX_VERIFIED).all()
    assert np.array_equal(enc["aux"] & 1, R.auto_res["aux"] & 1)
    assert np.array_equal(st.slots.cpu().numpy(), want), "a byte of dst differs from the unflagged call's"
    assert st.outputs_equal() == [] and blob[: int(offs[-1])].tobytes() == b"".join(R.oracle)
    # the synchronous form, and the wrapped surface: every piece verified
    sres, chunks = encode_specs(L, plain, R.specs, cfg=cfg)
    assert (sres["aux"] & G.AUX_VERIFIED == G.AUX_VERIFIED).all() and chunks == R.oracle
    c = SpecCall(L, ARRAYS, auto_cfg(verify=True, max_page_n=5000)); c.fill()
    G.check(c.encode_specs(R.specs))
    assert (c.infos["status"] == 0).all() and (c.infos["aux"] & G.AUX_VERIFIED == G.AUX_VERIFIED).all()


def test_strict_histograms_hold_for_a_specs_call_as_for_the_explicit_call(L, R):
    idx = [i for i, (s, a) in enumerate(zip(R.specs, ARRAYS)) if S.inv_is_one_over_base(s, a.dtype)]
    specs = [R.specs[i] for i in idx]
    st = U.Staged(L, [ARRAYS[i] for i in idx]); fill_slots(st)
    res, chunks = encode_specs(L, st, specs, cfg=auto_cfg(strict_histogram=True), sync=False)
    assert (res["status"] == 0).all()
    for j, i in enumerate(idx):
        one = U.Staged(L, [ARRAYS[i]]); fill_slots(one)
        cfg, _ = S.configs_of_spec(specs[j], ARRAYS[i].dtype, strict_histogram=True)
        r1, c1 = encode_config(L, one, cfg)
        assert r1["status"][0] == 0 and chunks[j] == c1[0], NAMES[i]
    names = launches(L, lambda: encode_specs(L, st, specs, cfg=auto_cfg(strict_histogram=True)))
    assert any("literal" in n for n in names), names


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. pass-cutting (a child process: PCO_GFX_WORKSPACE_GB is read once, when the library is loaded)
# ---------------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import ctypes as C, hashlib, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], ".."))
import numpy as np
import gpu_util as U
import chunk_specs_util as S
import test_gpu_chunk_specs as X
from pcodec_amd import _lib as G
L = G.lib()
rng = np.random.default_rng(4)
dist = [U.synth("c2", 20000, seed=1), np.cumsum(rng.integers(-5, 6, 20000)).astype(np.int32), U.synth("c2", 15000, seed=2)]
arrays = U.tile(dist, 200)
spec = S.spec(delta=G.DELTA_TRY_CONSECUTIVE, order=1)
explicit = G.make_config(enable_8_bit=True, max_page_n=6000, mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1)
c = X.SpecCall(L, arrays, X.auto_cfg(max_page_n=6000)); c.fill()
est = L.pco_gfx_wrapped_scratch_estimate(c.k, c.tasks, C.addressof(explicit))
L.pco_gfx_profile_begin()
G.check(c.encode_specs([spec] * c.k))
w_inits = U.profile_launches(L).count("enc_init_kernel")
c.pieces()
st = U.Staged(L, arrays); X.fill_slots(st)
L.pco_gfx_profile_begin()
res, chunks = X.encode_specs(L, st, [spec] * st.k)
s_inits = U.profile_launches(L).count("enc_init_kernel")
assert (res["status"] == 0).all()
print("RESULT " + json.dumps(dict(estimate=est, w_inits=w_inits, s_inits=s_inits, slots=hashlib.sha256(c.slots.cpu().numpy().tobytes()).hexdigest(),
      infos=hashlib.sha256(c.infos.tobytes()).hexdigest(), d_infos=hashlib.sha256(c.device_infos().tobytes()).hexdigest(),
      chunks=hashlib.sha256(b"".join(chunks)).hexdigest(), workspace=L.pco_gfx_workspace_bytes())))
"""


def _child(env_gb):
    env = dict(os.environ); env.pop("PCO_GFX_WORKSPACE_GB", None)
    if env_gb is not None:
        env["PCO_GFX_WORKSPACE_GB"] = env_gb
    r = subprocess.run([sys.executable, "-c", CHILD, HERE], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_a_synchronous_specs_call_beyond_the_budget_runs_in_passes():
    """200 chunks, all Classic / Consecutive(1), under a budget of 0.55 x the library's worst-case estimate for them under the explicit config the specs
    express (the figure a specs call's passes are planned with: the shape of its specs, not Auto's worst case): two balanced passes of 100 in the
    wrapped call, at least two in the standalone call, and the bytes of the uncut calls."""
    whole = _child(None)
    assert whole["w_inits"] == 1 and whole["s_inits"] == 1 and whole["estimate"] > 0
    cut = _child(repr(whole["estimate"] * 0.55 / 1e9))
    print(f"[passes] estimate {whole['estimate']} B; enc_init_kernel x {cut['w_inits']} (wrapped), x {cut['s_inits']} (standalone); workspace {cut['workspace']} B vs {whole['workspace']} B")
    assert cut["w_inits"] == 2 and cut["s_inits"] >= 2
    assert (cut["slots"], cut["infos"], cut["d_infos"], cut["chunks"]) == (whole["slots"], whole["infos"], whole["d_infos"], whole["chunks"])
    assert cut["workspace"] <= whole["workspace"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the Auto debug records
# ---------------------------------------------------------------------------------------------------------------------------------------
def debug_records(L):
    m = (G.AutoModeRecord * G.AUTO_DEBUG_MAX)(); d = (G.AutoDeltaRecord * G.AUTO_DEBUG_MAX)()
    C.memset(m, 0x5A, C.sizeof(m)); C.memset(d, 0x5A, C.sizeof(d))
    nm = L.pco_gfx_debug_auto_mode(m, G.AUTO_DEBUG_MAX); nd = L.pco_gfx_debug_auto_delta(d, G.AUTO_DEBUG_MAX)
    return nm, bytes(m)[: max(nm, 0) * C.sizeof(G.AutoModeRecord)], nd, bytes(d)[: max(nd, 0) * C.sizeof(G.AutoDeltaRecord)]


def test_the_auto_debug_records_read_all_zero_after_a_specs_call_and_as_before_after_an_auto_call(L, R):
    st = U.Staged(L, ARRAYS); fill_slots(st)
    encode_config(L, st, auto_cfg())
    before = debug_records(L)
    assert before[0] == before[2] == st.k and any(before[1]) and any(before[3])
    encode_specs(L, st, R.specs)
    nm, m, nd, d = debug_records(L)
    assert nm == nd == st.k and not any(m) and not any(d), "a specs call resolved nothing: its records are all-zero"
    c = SpecCall(L, ARRAYS, auto_cfg(max_page_n=5000))
    G.check(c.encode()); assert any(debug_records(L)[1])
    G.check(c.encode_specs(R.specs))
    nm, m, nd, d = debug_records(L)
    assert nm == nd == st.k and not any(m) and not any(d)
    encode_config(L, st, auto_cfg())
    assert debug_records(L) == before
