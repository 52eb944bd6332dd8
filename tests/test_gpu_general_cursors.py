"""-m gpu: PCO_GFX_CURSOR_GENERAL (include/pco_gfx.h section 4h) -- full-state cursors for the pages the general kernel decodes: Conv1, Dict under
None / Consecutive / Conv1, tables beyond the walkers' LDS slices with one, two and three variables.  pco_gfx_decompress_page_reads_ex and
pco_gfx_index_pages_ex with the flag against the input arrays, against each other, against the stepped tANS model and the latents; with flags == 0
against the entry points without a flags argument.  Two Lookback pages are the position-only control.  The helpers are the existing modules';
the library handle they take is wrapped so that their calls go through the _ex forms."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import oracle_lib as O  # noqa: E402
import gpu_util as U  # noqa: E402
import tans_model as TM  # noqa: E402
import test_gpu_page_ranges as R  # noqa: E402  (Stream, write_pages, Pool, meta_info, profiled_ms)
import test_page_reads_abi as A  # noqa: E402  (the cursor's layout restated, the stepped tANS model)
import test_general_cursors_abi as GA  # noqa: E402  (the kind-3 layout restated)
import test_gpu_page_reads as PR  # noqa: E402  (Cursors, Call, walk_chains: the chain shapes)
import test_gpu_page_index as PI  # noqa: E402  (IndexCall, check_index)
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig, DeltaSpec, ModeSpec  # noqa: E402

pytestmark = pytest.mark.gpu
N_LONG, N_EVEN = PR.N_LONG, PR.N_EVEN
GENERAL, POSITION = GA.GENERAL, A.POSITION
UNWRITTEN = PR.UNWRITTEN


class Flagged:
    """The library with pco_gfx_decompress_page_reads / pco_gfx_index_pages routed through their _ex forms under `flags`: what the existing
    helpers (PR.Call, PR.walk_chains, PI.IndexCall) call."""

    def __init__(self, lib, flags=G.CURSOR_GENERAL):
        self._lib, self._flags = lib, flags

    def pco_gfx_decompress_page_reads(self, n, tasks, res, d_res, stream):
        return self._lib.pco_gfx_decompress_page_reads_ex(n, tasks, self._flags, res, d_res, stream)

    def pco_gfx_index_pages(self, n, tasks, res, d_res, stream):
        return self._lib.pco_gfx_index_pages_ex(n, tasks, self._flags, res, d_res, stream)

    def __getattr__(self, name):
        return getattr(self._lib, name)


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


@pytest.fixture(scope="module")
def LF(L):
    return Flagged(L)


# ---------------------------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------------------------
CONV1 = {1: dict(quantization=3, bias=0, weights=[8]), 2: dict(quantization=4, bias=5, weights=[-16, 32]),
         32: dict(quantization=5, bias=-3, weights=[(1 + i % 3) * (-1) ** i for i in range(32)])}   # (sum |w| = 64: inside i16 for an 8-bit latent)


def gen(label, x, kind, its_order=0, **kw):
    s = PR.from_generator(label, x, **kw)
    s.kind, s.order = kind, its_order
    return s


def smooth(dt, n, seed):
    return R.numbers(dt, n, seed)


@pytest.fixture(scope="module")
def streams(L):
    """[Stream] with .kind and .order: every general page of the issue's list, then the two Lookback pages."""
    import torch
    out = []
    for order, dt, n, seed in ((1, np.uint8, N_LONG, 1), (2, np.uint16, N_EVEN, 2), (32, np.uint32, N_LONG, 3), (32, np.uint8, N_EVEN, 4), (1, np.uint32, N_EVEN, 5), (2, np.uint16, N_LONG, 6)):
        out.append(gen(f"conv1 order {order} {np.dtype(dt).name} n={n}", smooth(dt, n, seed), "conv1", order, mode=O.MODE_CLASSIC, delta=O.TE_DELTA_CONV1, **CONV1[order]))
    rng = np.random.default_rng(7)
    d32 = rng.integers(0, 1 << 30, 50).astype(np.uint32)[rng.integers(0, 50, N_LONG)]
    d16 = np.sort(rng.integers(0, 1 << 15, 40).astype(np.uint16))[np.clip(np.cumsum(rng.integers(-2, 3, N_EVEN)), 0, 39)]
    dc = rng.integers(0, 1 << 30, 30).astype(np.uint32)[np.clip(np.cumsum(rng.integers(-2, 3, N_LONG)) + 15, 0, 29)]
    out.append(gen("dict uint32 none", d32, "dict", 0, mode=O.MODE_TRY_DICT))
    out.append(gen("dict uint16 consecutive 2", d16, "dict+consecutive", 2, mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_CONSECUTIVE, order=2))
    out.append(gen("dict uint32 conv1", dc, "dict+conv1", 2, mode=O.MODE_TRY_DICT, delta=O.TE_DELTA_CONV1, **CONV1[2]))
    # the level-12 recipe of test_gpu_page_reads.py's route2 fixture: six pages of 8000 over one table of far more than 256 bins
    x = (np.arange(N_LONG, dtype=np.uint16) * 21 + 7)[np.random.default_rng(12).integers(0, N_LONG, 48000)]
    cc = paged.compress_chunks([torch.from_numpy(x.view(np.int16)).cuda()], ChunkConfig(compression_level=12, mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.no_op()),
                               page_sizes=[[8000] * 6])
    pieces = cc.directory; blob = cc.blob.cpu().numpy()
    meta = blob[pieces[0].offset: pieces[0].offset + pieces[0].length].tobytes()
    for p in pieces[1:]:
        s = R.Stream(f"level12 page {p.piece}", x.view(np.int16)[8000 * (p.piece - 1): 8000 * p.piece], meta, blob[p.offset: p.offset + p.length].tobytes())
        s.kind, s.order = "level12", 0
        out.append(s)
    wide = np.random.default_rng(8).integers(0, 60000, N_LONG).astype(np.uint32)
    out.append(gen("wide classic uint32", wide, "wide", 0, mode=O.MODE_CLASSIC, tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_n_bins=300, tbl_seed=1))
    out.append(gen("foreign ans_size_log 14 uint32", wide[::-1].copy(), "asl14", 0, mode=O.MODE_CLASSIC, tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=14, tbl_n_bins=300, tbl_seed=2))
    im = lambda dt, n, seed: (np.random.default_rng(seed).integers(0, 40000, n) * 10 + np.random.default_rng(seed + 1).integers(0, 4, n)).astype(dt)   # noqa: E731
    fm = lambda dt, n, seed: (np.random.default_rng(seed).integers(-20000, 20000, n) / 100.0).astype(dt)   # noqa: E731
    tbl = dict(tbl_vars=O.TBL_PRIMARY, tbl_ans_size_log=O.TBL_ANS_MIN, tbl_n_bins=300, tbl_seed=3)
    out.append(gen("int_mult wide uint32", im(np.uint32, N_LONG, 20), "int_mult", 1, mode=O.MODE_TRY_INT_MULT, mode_u64=10, delta=O.TE_DELTA_CONSECUTIVE, order=1, **tbl))
    out.append(gen("int_mult wide int64 secondary delta", im(np.int64, N_EVEN, 22), "int_mult+sec", 1, mode=O.MODE_TRY_INT_MULT, mode_u64=10, delta=O.TE_DELTA_CONSECUTIVE, order=1,
                   secondary_uses_delta=True, **tbl))
    out.append(gen("float_mult wide float64", fm(np.float64, N_LONG, 24), "float_mult", 1, mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=O.TE_DELTA_CONSECUTIVE, order=1, **tbl))
    out.append(gen("float_mult wide float32 secondary delta", fm(np.float32, N_EVEN, 26), "float_mult+sec", 1, mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01, delta=O.TE_DELTA_CONSECUTIVE,
                   order=1, secondary_uses_delta=True, **tbl))
    for s in R.write_pages(L, [("lookback uint32", R.numbers(np.uint32, N_LONG, 7, period=365)), ("lookback int64", R.numbers(np.int64, N_EVEN, 8, period=365))],
                           PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_LOOKBACK)):
        s.kind, s.order = "lookback", 0
        out.append(s)
    return out


def dict_delta(s):
    """(delta variant, consecutive order) behind a Dict ChunkMeta's dictionary: 4 + 25 bits of mode and length, byte alignment, the latents, 4 bits of variant"""
    k = len(G.chunk_meta_dict(s.meta, G.DTYPE_BYTE[s.nums.dtype.name]))
    rest = int.from_bytes(s.meta[4 + k * s.nums.dtype.itemsize:][:8], "little")
    return rest & 0xF, ((rest >> 4) & 0x7) if rest & 0xF == 1 else 0


def is_general(s):
    return s.kind != "lookback"


def test_the_streams_are_what_they_are_called(L, streams):
    seen = set()
    for s in streams:
        i = R.meta_info(L, s); seen.add(s.kind)
        if s.kind == "conv1":
            assert (i.mode_kind, i.delta_kind, i.present[2]) == (0, 3, 0) and G.chunk_meta_conv1(s.meta, G.DTYPE_BYTE[s.nums.dtype.name])[2] == CONV1[s.order]["weights"]
        elif s.kind.startswith("dict"):
            assert i.mode_kind == 4 and dict_delta(s) == {"dict": (0, 0), "dict+consecutive": (1, 2), "dict+conv1": (3, 0)}[s.kind]
        elif s.kind in ("level12", "wide"):
            assert (i.mode_kind, i.delta_kind) == (0, 0) and i.n_bins[1] > 256
        elif s.kind == "asl14":
            assert (i.mode_kind, i.delta_kind) == (0, 0) and i.ans_size_log[1] == 14
        elif s.kind in ("int_mult", "int_mult+sec", "float_mult", "float_mult+sec"):
            assert i.mode_kind == (1 if s.kind.startswith("int") else 2) and (i.delta_kind, i.delta_order) == (1, 1) and i.present[2] == 1 and i.n_bins[1] > 256
            assert i.secondary_uses_delta == (1 if s.kind.endswith("+sec") else 0)
        else:
            assert s.kind == "lookback" and i.delta_kind == 2
    assert seen == {"conv1", "dict", "dict+consecutive", "dict+conv1", "level12", "wide", "asl14", "int_mult", "int_mult+sec", "float_mult", "float_mult+sec", "lookback"}
    assert {(s.order, s.nums.dtype.name) for s in streams if s.kind == "conv1"} >= {(1, "uint8"), (2, "uint16"), (32, "uint32")}
    assert sum(1 for s in streams if s.kind == "level12") == 6 and sum(1 for s in streams if s.kind == "lookback") == 2
    assert {s.n for s in streams} == {N_LONG, N_EVEN, 8000}


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. chains
# ---------------------------------------------------------------------------------------------------------------------------------------
def walk_all(LF, streams, form):
    """{(stream index, row): 256 bytes}: the general streams want kind 3, the Lookback ones kind 2"""
    gen_ix = [i for i, s in enumerate(streams) if is_general(s)]; lb_ix = [i for i, s in enumerate(streams) if not is_general(s)]
    seen = {}
    for ix, kind in ((gen_ix, GENERAL), (lb_ix, POSITION)):
        got = PR.walk_chains(LF, [streams[i] for i in ix], form, want_kind=kind)   # (bit-exact rows, byte-identical cursors across chains, zero tails)
        seen.update({(ix[k], row): raw for (k, row), raw in got.items()})
    return seen


@pytest.fixture(scope="module")
def walked(LF, streams):
    return walk_all(LF, streams, "sync")


def test_chains_reach_every_batch_boundary_with_kind_3_cursors(streams, walked):
    for si, s in enumerate(streams):
        assert sorted(r for i, r in walked if i == si) == [min(r + 256, s.n) for r in range(0, s.n, 256)], s.label
    for (si, row), raw in walked.items():
        c = A.unpack_cursor(PR.words_of(raw))
        if is_general(streams[si]):
            assert c["kind"] == GENERAL and c["tail"] == [0] * 6
        else:
            assert c["kind"] == POSITION and sum(1 for w in PR.words_of(raw) if w) == 3


@pytest.mark.parametrize("form", ["async", "sync in passes"])
def test_the_other_forms_reach_the_same_cursors(LF, streams, walked, form):
    if form == "sync in passes":
        with PR.small_passes():
            again = walk_all(LF, streams, "sync")
    else:
        again = walk_all(LF, streams, form)
    assert again.keys() == walked.keys() and all(again[k] == walked[k] for k in walked)


def test_general_pages_run_the_new_kernels_and_not_the_prefix_kernel(L, LF, streams, walked):
    gs = [(i, s) for i, s in enumerate(streams) if is_general(s)]
    cur = PR.Cursors(2 * len(gs))
    for k, (i, s) in enumerate(gs):
        cur.put(2 * k, PR.words_of(walked[(i, 512)]))
    jobs = [(s, None, 600, 700, 2 * k, 2 * k + 1) for k, (i, s) in enumerate(gs)]
    L.pco_gfx_profile_begin()
    code, rec, got = PR.run_reads(LF, jobs, cur)
    names = U.profile_names(L)
    assert code == G.PcoSuccess
    PR.check_ok(jobs, rec, got)
    assert any(n.startswith("pco_decode_general_resume_kernel") for n in names) and "reads_shadow_kernel" in names, names
    assert not any(n.startswith("pco_decode_prefix_kernel") for n in names), names
    L.pco_gfx_profile_begin()
    code, rec, got = PI.run_index(LF, [(s, None, 256) for _, s in gs])
    names = U.profile_names(L)
    assert code == G.PcoSuccess and any(n.startswith("pco_decode_general_index_kernel") for n in names), names
    assert not any(n.startswith("pco_decode_prefix_kernel") for n in names), names


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. fields
# ---------------------------------------------------------------------------------------------------------------------------------------
def cursor_at(walked, si, row):
    w = PR.words_of(walked[(si, row)])
    return w, A.unpack_cursor(w)


def test_bit_position_and_states_are_the_stepped_model_s(streams, walked):
    si, s = next((i, s) for i, s in enumerate(streams) if s.kind == "wide")
    body, marks, latents, size_log = A.model_cursors(s.meta, s.page, s.n, 32)
    assert [int(v) for v in TM.to_latent(s.nums)] == latents
    for row, bit, states in marks:
        w, c = cursor_at(walked, si, row)
        assert w == GA.pack_general(row, bit, s.n, G.DTYPE_BYTE["uint32"], [[0] * 4, list(states), [0] * 4]), (row, c)   # everything else is zero
    assert len(marks) == 12


def forward_differences(lat, row, order, bits):
    d = lat[row: row + order]; want = []
    for _ in range(order):
        want.append(d[0]); d = [(b - a) % (1 << bits) for a, b in zip(d, d[1:])]
    return want


def dict_indices(s):
    d = G.chunk_meta_dict(s.meta, G.DTYPE_BYTE[s.nums.dtype.name])
    pos = {int(v): i for i, v in enumerate(d)}
    return [pos[int(v)] for v in TM.to_latent(s.nums)]


def test_moments_are_the_differences_at_the_row(streams, walked):
    n_checked = 0
    for si, s in enumerate(streams):
        if s.kind in ("int_mult", "int_mult+sec"):
            bits = s.nums.dtype.itemsize * 8
            lat = [int(v) for v in TM.to_latent(s.nums)]
            prim = [v // 10 for v in lat]; sec = [v % 10 for v in lat]
            for row in range(256, s.n, 256):
                w, c = cursor_at(walked, si, row)
                want_sec = [sec[row]] if s.kind == "int_mult+sec" else [0]
                assert c["moments"] == [[prim[row]] + [0] * 7, want_sec + [0] * 7] and c["states"][0] == [0] * 4 and c["tail"] == [0] * 6, (s.label, row)
                n_checked += 1
        elif s.kind == "dict+consecutive":
            idx = dict_indices(s)
            for row in range(256, s.n - 2, 256):
                w, c = cursor_at(walked, si, row)
                assert c["moments"] == [forward_differences(idx, row, 2, 32) + [0] * 6, [0] * 8] and c["states"][0] == [0] * 4 and c["states"][2] == [0] * 4, (s.label, row)
                n_checked += 1
        elif s.kind in ("dict", "level12", "asl14"):
            for row in range(256, s.n, 256):
                assert cursor_at(walked, si, row)[0][10:] == [0] * 22, (s.label, row)
    assert n_checked >= 11 + 10 + 10


def test_conv1_residuals_are_the_latents_the_decoder_carries_at_the_row(streams, walked):
    """Conv1's state in front of row r is what delta/conv1.rs carries between two batches: the last `order` residuals of the batch before, which are
    the latents (in Dict mode the dictionary indices) of rows [r, r + order) -- the output lags the deltas by `order`, as the page's own header
    holds the first `order` latents.  (The issue that asked for this test named rows [r - order, r); no decoder carries those, and rows
    [r, r + order) cannot be had from them: their deltas lie in front of the cursor's bit position.)  Rows whose state reaches beyond the page
    are left to the chain comparison."""
    n_checked = 0
    for si, s in enumerate(streams):
        if s.kind not in ("conv1", "dict+conv1"):
            continue
        lat = dict_indices(s) if s.kind == "dict+conv1" else [int(v) for v in TM.to_latent(s.nums)]
        for row in range(256, s.n - s.order + 1, 256):
            w, c = cursor_at(walked, si, row)
            assert GA.unpack_residuals(w, s.order) == lat[row: row + s.order], (s.label, row)
            assert w[10:26] == GA.pack_residuals(lat[row: row + s.order]) and w[26:] == [0] * 6 and c["states"][0] == [0] * 4 and c["states"][2] == [0] * 4, (s.label, row)
            n_checked += 1
    assert n_checked >= 7 * 10


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the index
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_the_flagged_index_is_the_chain_of_reads(LF, streams, walked, form):
    jobs = [(s, None, every) for s in streams for every in (256, 1024)]
    owner = [si for si in range(len(streams)) for _ in (256, 1024)]
    code, rec, got = PI.run_index(LF, jobs, form)
    assert code == G.PcoSuccess, LF.pco_gfx_last_error()
    for j, (s, _, every) in enumerate(jobs):
        PI.check_index([jobs[j]], rec[j: j + 1], got[j: j + 1], lambda _, row, j=j: walked[(owner[j], row)], 0 if is_general(s) else 1, form)
    assert sum(len(g) for g in got) > 300


@pytest.mark.parametrize("form", ["sync", "async"])
def test_one_mixed_index_call(L, LF, streams, walked, form):
    """route-1 pages, general pages, Lookback pages, a general page cut inside the walked prefix and one cut behind its last cursor"""
    r1 = R.write_pages(L, [("classic uint32", R.numbers(np.uint32, N_LONG, 3)), ("consecutive int64", R.numbers(np.int64, N_EVEN, 12))],
                       PR.per(mode=G.MODE_CLASSIC, delta=G.DELTA_TRY_CONSECUTIVE, delta_order=1))
    for s in r1:
        s.kind = "route1"
    r1_truth = PR.walk_chains(L, r1, "sync")   # (kind 1: the unflagged entry point's cursors are what the flag leaves alone)
    vi, victim = next((i, s) for i, s in enumerate(streams) if s.kind == "conv1" and s.n == N_LONG)
    bit_2304 = A.unpack_cursor(PR.words_of(walked[(vi, 2304)]))["bit"]; bit_2816 = A.unpack_cursor(PR.words_of(walked[(vi, 2816)]))["bit"]
    cut_inside = victim.page[: bit_2304 // 8 - 8]          # ends in front of the batch that ends at row 2304: inside [0, 2816)
    cut_behind = victim.page[: bit_2816 // 8 + 1]          # holds every batch in front of row 2816, not the page's last one
    jobs = [(r1[0], None, 256), (streams[0], None, 256), (streams[-1], None, 512), (victim, cut_inside, 256), (r1[1], None, 1024), (victim, cut_behind, 256),
            (streams[-2], None, 256), (streams[6], None, 1024)]
    code, rec, got = PI.run_index(LF, jobs, form)
    if form == "sync":
        assert code == G.PcoDecompressionError and LF.pco_gfx_last_status() == G.ST_INSUFFICIENT_DATA
    assert (rec["status"][3], rec["n_out"][3]) == (G.ST_INSUFFICIENT_DATA, 0)
    truth = {0: lambda row: r1_truth[(0, row)], 1: lambda row: walked[(0, row)], 2: lambda row: walked[(len(streams) - 1, row)], 4: lambda row: r1_truth[(1, row)],
             5: lambda row: walked[(vi, row)], 6: lambda row: walked[(len(streams) - 2, row)], 7: lambda row: walked[(6, row)]}
    for j, t in truth.items():
        PI.check_index([jobs[j]], rec[j: j + 1], got[j: j + 1], lambda _, row, t=t: t(row), 1 if jobs[j][0].kind == "lookback" else 0, (form, j))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. segments side by side
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_segments_from_the_index_in_one_reads_call_equal_the_input(LF, streams):
    jobs = [(s, None, every) for s in streams for every in (256, 1024)]
    call = PI.IndexCall(LF, jobs, "async")
    code, rec, got = call.finish()
    assert code == G.PcoSuccess and (rec["status"] == 0).all()
    cur = PR.Cursors(1)
    reads = []
    for j, (s, _, every) in enumerate(jobs):
        for i, row in enumerate(range(0, s.n, every) if call.ks[j] else [0]):
            reads.append((j, s, row, min(every, s.n - row) if call.ks[j] else s.n, call.ptr(j, i - 1) if i else None))
    # PR.Call lays every dst between canaries; on the way to the library its tasks get their `from` pointers, which lie in the index's own arrays
    rjobs = [(s, None, row, count, None, None) for _, s, row, count, _ in reads]

    class FromTheIndex(Flagged):
        def pco_gfx_decompress_page_reads(self, n, tasks, res, d_res, stream):
            for t, r in zip(tasks, reads):
                t.from_ = r[4]
            return Flagged.pco_gfx_decompress_page_reads(self, n, tasks, res, d_res, stream)

    code, rec, got = PR.Call(FromTheIndex(LF._lib), rjobs, cur).finish()
    assert code == G.PcoSuccess, LF.pco_gfx_last_error()
    PR.check_ok(rjobs, rec, got)
    call.finish()   # (the reads left the index's cursors and their guards alone)


def test_the_paged_functions_under_the_flag(L):
    import torch
    d = np.random.default_rng(1).integers(0, 1 << 15, 50).astype(np.uint32)[np.random.default_rng(2).integers(0, 50, 7000)]
    x = (np.arange(3000, dtype=np.uint16) * 21 + 7)[np.random.default_rng(12).integers(0, 3000, 24000)].view(np.int16)
    lb = R.numbers(np.int64, 5000, 8, period=365)
    cases = [(d.view(np.int32), "int32", ChunkConfig(mode_spec=ModeSpec.try_dict(), delta_spec=DeltaSpec.no_op(), enable_dict=True), [3000, 4000]),
             (x, "int16", ChunkConfig(compression_level=12, mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.no_op()), [8000] * 3),
             (lb, "int64", ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_lookback()), [5000])]
    for a, name, cfg, sizes in cases:
        cc = paged.compress_chunks([torch.from_numpy(a).cuda()], cfg, page_sizes=[sizes])
        dr = cc.directory
        for every in (256, 1024):
            idx = paged.index_pages(cc.blob, dr, [name], every, general=True)
            torch.cuda.synchronize()
            res = idx.results.cpu().numpy().view(paged.RESULT_DT)
            assert (res["status"] == 0).all() and list(res["n_out"]) == [(n - 1) // every for n in sizes]
            saved = paged.save_cursors(cc.blob, dr, [name], every, general=True)
            assert all(bytes(p.cursors.cpu().numpy().tobytes()) == bytes(q.cursors.cpu().numpy().tobytes()) for p, q in zip(idx, saved)), (name, every)
            got = paged.decompress_chunks_from(cc.blob, dr, [name], idx, general=True)
            assert len(got) == 1 and U.bits_equal(got[0].cpu().numpy(), a), (name, every)
            got = paged.decompress_rows_from(cc.blob, dr, [name], idx, [(1100, a.size - 3)], general=True)
            assert U.bits_equal(got[0].cpu().numpy(), a[1100: a.size - 3]), (name, every)
        r = paged.ChunkReader(cc.blob, dr, [name], 0, general=True)
        parts = [r.read(n).cpu().numpy() for n in (256, 1024, 512)]
        parts.append(r.read(a.size - r.pos).cpu().numpy())
        assert U.bits_equal(np.concatenate(parts), a), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. flags == 0 is the old entry point
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_flags_0_is_the_entry_point_without_flags(L, streams):
    L0 = Flagged(L, 0)
    rng = np.random.default_rng(3)
    cur_a, cur_b = PR.Cursors(2 * len(streams)), PR.Cursors(2 * len(streams))
    jobs = []
    for k, s in enumerate(streams):
        row = int(rng.integers(1, s.n // 256)) * 256
        for cur in (cur_a, cur_b):
            cur.put(2 * k, A.pack_cursor(POSITION, row, 0, s.n, G.DTYPE_BYTE[s.nums.dtype.name]))
        first = min(row + int(rng.integers(0, 300)), s.n - 1)
        jobs.append((s, None, first, int(rng.integers(1, s.n - first + 1)), 2 * k, 2 * k + 1))
    jobs.append((streams[0], streams[0].page[:40], 0, 600, None, None))   # ... and a task that fails
    for form in ("sync", "async"):
        a = PR.run_reads(L, jobs, cur_a, form); b = PR.run_reads(L0, jobs, cur_b, form)
        assert a[0] == b[0] and (a[1] == b[1]).all(), form
        assert all((x is None and y is None) or U.bits_equal(x, y) for x, y in zip(a[2], b[2]))
        PR.check_ok(jobs[:-1], a[1][:-1], a[2][:-1], form)
        sa, sb = cur_a.snapshot(), cur_b.snapshot()
        assert sa == sb
        for k, s in enumerate(streams):
            c = A.unpack_cursor(PR.words_of(sa[2 * k + 1]))
            assert c["kind"] == POSITION and sum(1 for w in PR.words_of(sa[2 * k + 1]) if w) == 3, s.label   # kind 2 on route 2, three non-zero words
        ijobs = [(s, None, every) for s in streams for every in (256, 1024)]
        ia = PI.run_index(L, ijobs, form); ib = PI.run_index(L0, ijobs, form)
        assert ia[0] == ib[0] and (ia[1] == ib[1]).all() and ia[2] == ib[2], form
        assert (ia[1]["aux"] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
def test_a_refused_cursor_refuses_its_task_alone(L, LF, streams, walked, form):
    si, s = next((i, s) for i, s in enumerate(streams) if s.kind == "int_mult+sec")      # a primary and a secondary variable, both with moments
    info = R.meta_info(L, s)
    w512 = PR.words_of(walked[(si, 512)]); base = A.unpack_cursor(w512)
    wi, ws = next((i, x) for i, x in enumerate(streams) if x.kind == "wide")
    body = A.model_cursors(ws.meta, ws.page, ws.n, 32)[0]
    wbase = A.unpack_cursor(PR.words_of(walked[(wi, 512)]))
    assert body > 0
    li, lb = next((i, x) for i, x in enumerate(streams) if x.kind == "lookback")
    ci, cs = next((i, x) for i, x in enumerate(streams) if x.kind == "conv1" and x.order == 32)

    def edit(b=base, **kw):
        d = {k: b[k] for k in ("kind", "row", "bit", "page_n", "dtype", "states", "moments", "version")}
        d.update(kw)
        return A.pack_cursor(**d)

    def state(v, j, x):
        st = [list(r) for r in base["states"]]; st[v][j] = x
        return edit(states=st)

    lb_dtype = G.DTYPE_BYTE[lb.nums.dtype.name]
    rows = [("version", s, edit(version=2)), ("kind 1", s, edit(kind=A.FULL)), ("kind 0", s, edit(kind=0)), ("page_n", s, edit(page_n=s.n - 1)),
            ("dtype", s, edit(dtype=base["dtype"] ^ 3)), ("at unaligned", s, edit(row=300)), ("at > first", s, edit(row=768)),
            ("bit before the body", ws, edit(wbase, bit=body - 1)), ("bit beyond the page", s, edit(bit=8 * len(s.page) + 1)),
            ("primary state 2^asl", s, state(1, 2, 1 << info.ans_size_log[1])), ("secondary state 2^asl", s, state(2, 0, 1 << info.ans_size_log[2])),
            ("a state for a variable the page does not have", s, state(0, 3, 1)),
            ("kind 2 on a general page under the flag", s, A.pack_cursor(POSITION, 512, 0, s.n, base["dtype"])),
            ("kind 2 on a Conv1 page under the flag", cs, A.pack_cursor(POSITION, 512, 0, cs.n, G.DTYPE_BYTE[cs.nums.dtype.name])),
            ("kind 3 on a Lookback page", lb, edit(page_n=lb.n, dtype=lb_dtype, states=[[0] * 4] * 3, moments=None, bit=8 * 40)),
            ("kind 1 on a Lookback page", lb, A.pack_cursor(A.FULL, 512, 8 * 40, lb.n, lb_dtype))]
    assert edit() == w512
    cur = PR.Cursors(2 * len(rows) + 4)
    jobs = []
    for k, (_, st, words) in enumerate(rows):
        cur.put(2 * k, words); jobs.append((st, None, 600, 300, 2 * k, 2 * k + 1))
    g0 = 2 * len(rows)
    cur.put(g0, w512); cur.put(g0 + 2, A.pack_cursor(POSITION, 512, 0, lb.n, lb_dtype))
    good = [(s, None, 600, 300, g0, g0 + 1), (lb, None, 600, 300, g0 + 2, g0 + 3), (cs, None, 0, cs.n, None, None)]
    before = cur.snapshot()
    all_jobs = jobs[:5] + good[:1] + jobs[5:] + good[1:]
    order = list(range(5)) + [len(rows)] + list(range(5, len(rows))) + [len(rows) + 1, len(rows) + 2]
    code, rec, got = PR.run_reads(LF, all_jobs, cur, form)
    if form == "sync":
        assert code == G.PcoDecompressionError and L.pco_gfx_last_status() == G.ST_INVALID_ARGUMENT
    after = cur.snapshot()
    for at, k in enumerate(order):
        if k < len(rows):
            assert (rec["status"][at], rec["n_out"][at], rec["consumed"][at], rec["aux"][at]) == (G.ST_INVALID_ARGUMENT, 0, 0, 0), rows[k][0]
            assert got[at] is None, ("dst was written", rows[k][0])
            assert after[2 * k] == before[2 * k] and after[2 * k + 1] == UNWRITTEN, rows[k][0]
    gj = [order.index(len(rows) + i) for i in range(3)]
    PR.check_ok(good, rec[gj], [got[j] for j in gj], form)
    assert after[g0 + 1] == walked[(si, 1024)] and after[g0 + 3] == walked[(li, 1024)]
    # kind 3 into a flags == 0 call: on a general page (route 2 wants kind 2 there) and, for what it is worth, on a two-kernel page
    cur = PR.Cursors(2); cur.put(0, w512)
    for lib in (L, Flagged(L, 0)):
        code, rec, got = PR.run_reads(lib, [(s, None, 600, 300, 0, 1)], cur, form)
        assert rec["status"][0] == G.ST_INVALID_ARGUMENT and got[0] is None and cur.snapshot()[1] == UNWRITTEN


def test_a_cursor_of_another_page_of_the_same_chunk_stays_inside(LF, streams, walked):
    """Same tables, another page's bit position, states and nothing else wrong: wrong numbers or an error status, every canary intact."""
    pages = [(i, s) for i, s in enumerate(streams) if s.kind == "level12"]
    cur = PR.Cursors(2 * len(pages)); jobs = []
    for k, (i, s) in enumerate(pages):
        oi, other = pages[(k + 1) % len(pages)]
        c = A.unpack_cursor(PR.words_of(walked[(oi, 4096)]))
        cur.put(2 * k, GA.pack_general(4096, min(c["bit"], 8 * len(s.page)), s.n, c["dtype"], c["states"]))
        jobs.append((s, None, 4096, 3904, 2 * k, 2 * k + 1))
    code, rec, got = PR.run_reads(LF, jobs, cur)   # (finish() checks the canaries around every dst)
    cur.snapshot()
    assert all(st in (G.ST_OK, G.ST_INSUFFICIENT_DATA, G.ST_CORRUPTION) for st in rec["status"]), rec["status"]


def test_a_page_damaged_behind_the_read_and_inside_it(LF, streams, walked):
    for kind in ("conv1", "dict+consecutive", "wide", "int_mult+sec"):
        si, s = next((i, x) for i, x in enumerate(streams) if x.kind == kind)
        bit = lambda row: A.unpack_cursor(PR.words_of(walked[(si, row)]))["bit"]   # noqa: E731
        page = s.page[: bit(1536) // 8 + 1]     # every batch in front of row 1536 is whole; what follows is gone
        cur = PR.Cursors(4)
        cur.put(0, PR.words_of(walked[(si, 512)])); cur.put(2, PR.words_of(walked[(si, 512)]))
        jobs = [(s, page, 600, 900, 0, 1), (s, page, 600, 1200, 2, 3)]   # rows [600, 1500) end in front of the damage; [600, 1800) run into it
        for form in ("sync", "async"):
            code, rec, got = PR.run_reads(LF, jobs, cur, form)
            assert list(rec["status"]) == [G.ST_OK, G.ST_INSUFFICIENT_DATA] and list(rec["n_out"]) == [900, 0], (kind, form, rec)
            assert U.bits_equal(got[0], s.nums[600:1500]) and got[1] is None
            slots = cur.snapshot()
            assert slots[1] == walked[(si, 1536)] and slots[3] == UNWRITTEN, (kind, form)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the work follows the slice
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_work_of_a_general_read_follows_its_slice(L):
    """One wide-table page of 2^18 u16 numbers at level 12 (2^20 when the whole page decodes in under 2 ms).  Kernel time from pco_gfx_profile_*:
    (a) rows [15 n / 16, n) from a saved cursor against the same rows through pco_gfx_decompress_page_ranges: 1/16 of the batches by construction,
    at most 1/4; (b) the page as sixteen segments in one call against pco_gfx_decompress_pages: at most 1/4; (c) one flagged index call against
    pco_gfx_decompress_pages: the same walk minus join and store, at most 1.5 x."""
    import torch

    def setup(n):   # the level-12 recipe of the `streams` fixture in one page: 3000 distinct 16-bit values, each many times
        x = (np.arange(3000, dtype=np.uint16) * 21 + 7)[np.random.default_rng(12).integers(0, 3000, n)].view(np.int16)
        cc = paged.compress_chunks([torch.from_numpy(x).cuda()], ChunkConfig(compression_level=12, mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.no_op()), page_sizes=[[n]])
        pieces = cc.directory; blob = cc.blob.cpu().numpy()
        s = R.Stream(f"level 12 i16 2^{n.bit_length() - 1}", x, blob[pieces[0].offset: pieces[0].offset + pieces[0].length].tobytes(),
                     blob[pieces[1].offset: pieces[1].offset + pieces[1].length].tobytes())
        assert len(pieces) == 2 and R.meta_info(L, s).n_bins[1] > 256
        return s

    def measure(s):
        n = s.n; seg = n // 16; w = 2; dt = G.DTYPE_BYTE["int16"]
        pool = R.Pool([s.meta, s.page])
        whole = torch.zeros(n * w + 64, dtype=torch.uint8, device="cuda")
        part = torch.zeros(seg * w + 64, dtype=torch.uint8, device="cuda")
        curs = torch.zeros((15, 256), dtype=torch.uint8, device="cuda")

        def reads(tasks):
            t = (G.PageReadTask * len(tasks))(*tasks); res = (G.TaskResult * len(tasks))()
            G.check(L.pco_gfx_decompress_page_reads_ex(len(tasks), t, G.CURSOR_GENERAL, res, None, None))

        def task(dst, first, count, fr):
            return G.PageReadTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), dst, n, first, count, dt, 4, fr, None)

        def index():
            t = (G.PageIndexTask * 1)(G.PageIndexTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), curs.data_ptr(), n, seg, dt, 4)); res = (G.TaskResult * 1)()
            G.check(L.pco_gfx_index_pages_ex(1, t, G.CURSOR_GENERAL, res, None, None))
            assert (res[0].n_out, res[0].aux) == (15, 0)

        def last_as_range():
            t = (G.PageRangeTask * 1)(G.PageRangeTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), part.data_ptr(), n, 15 * seg, seg, dt, 4)); res = (G.TaskResult * 1)()
            G.check(L.pco_gfx_decompress_page_ranges(1, t, res, None, None))

        def one_page():
            t = (G.PageTask * 1)(G.PageTask(pool.ptr(0), len(s.meta), pool.ptr(1), len(s.page), whole.data_ptr(), n, dt, 4)); res = (G.TaskResult * 1)()
            G.check(L.pco_gfx_decompress_pages(1, t, res, None, None))

        ms_page = R.profiled_ms(L, one_page)
        assert U.bits_equal(whole[: n * w].cpu().numpy().view(np.int16), s.nums)
        ms_index = R.profiled_ms(L, index)
        cptr = lambda k: curs.data_ptr() + 256 * (k - 1)   # noqa: E731  (the cursor in front of row k * seg)
        ms_range = R.profiled_ms(L, last_as_range)
        part.zero_()
        ms_read = R.profiled_ms(L, lambda: reads([task(part.data_ptr(), 15 * seg, seg, cptr(15))]))
        assert U.bits_equal(part[: seg * w].cpu().numpy().view(np.int16), s.nums[15 * seg:])
        whole.zero_()
        ms_sixteen = R.profiled_ms(L, lambda: reads([task(whole.data_ptr() + w * k * seg, k * seg, seg, cptr(k) if k else None) for k in range(16)]))
        assert U.bits_equal(whole[: n * w].cpu().numpy().view(np.int16), s.nums)
        return ms_page, ms_index, ms_range, ms_read, ms_sixteen

    s = setup(1 << 18)
    ms = measure(s)
    if ms[0] < 2.0:
        s = setup(1 << 20); ms = measure(s)
    ms_page, ms_index, ms_range, ms_read, ms_sixteen = ms
    print(f"{s.label}: pco_gfx_decompress_pages {ms_page:.3f} ms, flagged index {ms_index:.3f} ms; rows [15 n / 16, n): as a range {ms_range:.3f} ms, from a saved cursor "
          f"{ms_read:.3f} ms; sixteen segments in one call {ms_sixteen:.3f} ms")
    assert ms_read <= ms_range / 4, (ms_read, ms_range)
    assert ms_sixteen <= ms_page / 4, (ms_sixteen, ms_page)
    assert ms_index <= 1.5 * ms_page, (ms_index, ms_page)
