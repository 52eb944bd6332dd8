"""-m gpu: the quantile histogram's bin walk (K2 of encode_kernels.hip: hist_walk, hist_walk_rec, enc_hist_walk_kernel, the one-thread-per-bin
shortcut of hist_emit and of the 256-bin windows at levels 9-12, and encode_hist_literal.hip's builder) at its run and count edges.

The rows and the plain model that certifies them are in tests/hist_edges_util.py and tests/hist_model.py; tests/test_hist_model.py pins both on
the CPU (model == both rules of the oracle, no heapsort branch, every row on its branch and changed by its variants) before anything here runs.
Rows that share a config share ONE synchronous call.  Per row and present variable, pco_gfx_debug_histogram -- a read of what the histogram
kernels left in the chunk's plan region -- must give the model's bins, bin for bin (count, lower, upper, n_hist), the variable's number of
latents and n_bins_log, and the hist_path the model predicts (0 counted compact, 1 rank queries at full width, 2 the radix-sort fallback); the
chunk's bytes equal the oracle's and it decodes bit for bit.  A boundary that moved by one rank shows in the bins even where optimize_bins
would have merged it away in the bytes.  Strict rows are held to O.histogram(rule=0) on the latents in stored order.  Per call, the histogram
kernels in the profile are exactly the union of latent_window_util.TIER_KERNELS over the rows' tiers, and enc_hist_walk_kernel is there iff
some variable is outside the direct tier.  Nothing is skipped."""
import collections
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import gpu_util as U
import hist_edges_util as E
import latent_window_util as W
import oracle_lib as O
from pcodec_amd import _lib as G
from test_gpu_width_paths import decode_call, encode_call
from test_gpu_wrapped_writer import Call

pytestmark = pytest.mark.gpu
CAP = 4096 + 8


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def device_histogram(L, task, var, cap=CAP):
    """(n_hist or -status, [(count, lower, upper)] of the bins written, info) with a sentinel behind what `cap` allows."""
    lo = np.full(cap + 2, 0xA5A5A5A5A5A5A5A5, np.uint64); hi = lo.copy(); cnt = np.full(cap + 2, 0xA5A5A5A5, np.uint32); info = np.zeros(4, np.uint32)
    n = L.pco_gfx_debug_histogram(task, var, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), cap, info.ctypes.data_as(C.c_void_p))
    k = max(min(n, cap), 0)
    assert (lo[k:] == 0xA5A5A5A5A5A5A5A5).all() and (hi[k:] == 0xA5A5A5A5A5A5A5A5).all() and (cnt[k:] == 0xA5A5A5A5).all(), "written past min(n_hist, cap)"
    return n, list(zip(cnt[:k].tolist(), lo[:k].tolist(), hi[:k].tolist())), info.tolist()


def cfg_of(rows):
    return G.make_config(enable_8_bit=True, strict_histogram=rows[0].strict, **rows[0].kw)


@functools.lru_cache(maxsize=None)
def want(name, pages=None):
    """The oracle's bytes of a row, once: a standalone chunk, or (ChunkMeta, [pages]) of a wrapped one (`pages`: in these exact pages instead)."""
    r = E.BY_NAME()[name]
    ocfg = O.make_config(enable_8_bit=True, **r.kw)
    if r.paging is None and pages is None:
        return U.oracle_chunk(r.arr, ocfg)
    exact = list(pages) if pages is not None else (r.pages if r.paging == "exact" else None)
    meta, pgs, ns = O.wrapped_compress(r.arr, ocfg, max_pages=len(exact or r.pages) + 1, exact_pages=exact)
    assert ns == (exact or r.pages)
    return meta, pgs


def by_config(rows):
    groups = collections.OrderedDict()
    for r in rows:
        groups.setdefault(E.config_key(r), []).append(r)
    return list(groups.values())


def check_histograms(L, rows):
    """The hook against the model for every variable of every chunk of the call just made: [(row, variable, what differs)]."""
    bad = []
    for t, r in enumerate(rows):
        vs, _ = E.variables(r.name)
        for var in (0, 1, 2):
            v = next((x for x in vs if x.var == var), None)
            n, bins, info = device_histogram(L, t, var)
            if v is None:
                if n != 0: bad.append((r.name, var, "absent variable", n))
                continue
            model = E.model_of(r.name, var)[0]
            if r.strict:
                lit, fb = O.histogram(v.latents, v.bins_log, rule=0)
                assert not fb and lit == model
            if n != len(model) or bins != model:
                first = next((i for i, (a, b) in enumerate(zip(bins, model)) if a != b), min(len(bins), len(model)))
                bad.append((r.name, var, "bins", n, len(model), first, bins[first:first + 2], model[first:first + 2]))
            if info != [v.latents.size, v.bins_log, v.hist_path, 0]:
                bad.append((r.name, var, "info", info, [v.latents.size, v.bins_log, v.hist_path, 0]))
    return bad


def check_kernels(rows, names):
    tiers = [v.tier for r in rows for v in E.variables(r.name)[0]]
    hist = {k for t in tiers for k in W.TIER_KERNELS[t]}
    got = set(names) & set(W.HIST_KERNELS)
    print(f"{len(rows)} chunks, tiers {sorted(set(tiers))}: {sorted(got)}")
    assert got == hist, (rows[0].name, sorted(got), sorted(hist))
    assert "enc_hist_kernel" in names
    assert ("enc_hist_walk_kernel" in names) == any(t != "direct" for t in tiers), (rows[0].name, names)
    assert ("enc_hist_literal_kernel" in names) == rows[0].strict


def run_group(L, rows):
    """One synchronous call over rows of ONE config: the device's histograms against the model, bytes against the oracle, kernels, round trip."""
    assert len(by_config(rows)) == 1
    arrays = [r.arr for r in rows]
    if rows[0].paging is None:
        chunks, names = encode_call(arrays, cfg_of(rows))
        bad = check_histograms(L, rows)
        wrong = [r.name for r, c in zip(rows, chunks) if c != want(r.name)]
        assert not bad and not wrong, (len(bad), bad[:4], len(wrong), wrong[:6])
        check_kernels(rows, names)
        decode_call(chunks, arrays)
        return
    c = Call(L, arrays, cfg_of(rows), [r.pages if r.paging == "exact" else None for r in rows])
    L.pco_gfx_profile_begin()
    G.check(c.encode())
    names = U.profile_names(L)
    bad = check_histograms(L, rows)
    pieces = c.pieces()
    wrong = [r.name for r, (meta, pages, ns) in zip(rows, pieces) if (meta, pages) != want(r.name) or ns != r.pages]
    assert not bad and not wrong, (len(bad), bad[:4], len(wrong), wrong[:6])
    check_kernels(rows, names)
    c.decode_and_compare()


@pytest.mark.parametrize("section", list("abcdef"))
def test_the_devices_bins_equal_the_models_for_every_row(L, section):
    rows = [r for r in E.all_rows() if r.section == section]
    assert rows
    failed = []                       # (every config's call runs, so that one report names every row that is wrong)
    for group in by_config(rows):
        try:
            run_group(L, group)
        except AssertionError as e:
            failed.append((group[0].name, str(e)[:1500]))
    assert not failed, failed


def mixed_rows():
    """Every standalone Classic level-8 row of (a), (b) and (c), shuffled: all five tiers, the fallback, shortcut and walked side by side."""
    rows = [r for r in E.rows_a() + E.rows_b() + E.rows_c() if r.kw == E.cfg_kw(8)]
    rng = np.random.default_rng(9)
    return [rows[i] for i in rng.permutation(len(rows))]


def test_every_tier_in_one_call_synchronous_and_asynchronous(L):
    import torch
    rows = mixed_rows()
    tiers = {v.tier for r in rows for v in E.variables(r.name)[0]}
    flags = {E.model_of(r.name, 1)[1].shortcut for r in rows}
    assert tiers == set(W.TIERS) and flags == {True, False} and any(r.gives_up for r in rows)
    run_group(L, rows)
    arrays = [r.arr for r in rows]; cfg = cfg_of(rows)
    s = U.Staged(L, arrays)
    tasks = s.enc_tasks()
    G.check(L.pco_gfx_compress_chunks(s.k, U.ptr(tasks), C.byref(cfg), None, s.d_res.data_ptr(), None))
    torch.cuda.synchronize()
    res = s.results()
    assert (res["status"] == 0).all(), res["status"]
    got = s.slot_bytes(res["n_out"])
    assert [r.name for r, c in zip(rows, got) if c != want(r.name)] == []


def test_the_same_rows_through_the_wrapped_writer_in_several_pages(L):
    """No delta: every position is stored whatever the paging, so the histogram is the one-page row's; the bytes are the oracle's pages."""
    rows = [r for r in mixed_rows() if r.arr.size >= 1000]
    assert len(rows) >= 60 and {v.tier for r in rows for v in E.variables(r.name)[0]} == set(W.TIERS)
    pages = [[r.arr.size // 3 + 1, 257, r.arr.size - r.arr.size // 3 - 258] for r in rows]
    c = Call(L, [r.arr for r in rows], cfg_of(rows), pages)
    L.pco_gfx_profile_begin()
    G.check(c.encode())
    names = U.profile_names(L)
    bad = check_histograms(L, rows)
    wrong = [r.name for r, pg, (meta, pgs, ns) in zip(rows, pages, c.pieces()) if (meta, pgs) != want(r.name, tuple(pg)) or ns != pg]
    assert not bad and not wrong, (len(bad), bad[:4], len(wrong), wrong[:6])
    check_kernels(rows, names)
    c.decode_and_compare()


def test_the_hooks_contract(L):
    """0 before any encode on a fresh thread, 0 for an absent variable and for a chunk beyond the pass, min(n_hist, cap) bins written for a
    small cap with n_hist returned, INVALID_ARGUMENT for a variable that does not exist, 0 after pco_gfx_release_workspace."""
    row = E.BY_NAME()["a-uint32-n4096-after-skip-run-ends@c"]
    model = E.model_of(row.name, 1)[0]
    out = {}

    def work():
        try:
            out["fresh"] = device_histogram(L, 0, 1)[0]
            chunks, _ = encode_call([row.arr, row.arr[:300]], cfg_of([row]))
            out["chunk"] = chunks[0]
            out["full"] = device_histogram(L, 0, 1)
            out["small"] = device_histogram(L, 0, 1, cap=7)
            out["none"] = device_histogram(L, 0, 1, cap=0)
            out["absent"] = [device_histogram(L, 0, 0)[0], device_histogram(L, 0, 2)[0]]
            out["beyond"] = device_histogram(L, 2, 1)[0]
            out["second"] = device_histogram(L, 1, 1)[2]
            out["invalid"] = device_histogram(L, 0, 3)[0]
            L.pco_gfx_release_workspace()
            out["released"] = device_histogram(L, 0, 1)[0]
        except BaseException as e:   # (reported by the asserting thread)
            out["error"] = repr(e)

    t = threading.Thread(target=work); t.start(); t.join()
    assert "error" not in out, out["error"]
    assert out["fresh"] == 0 and out["released"] == 0 and out["absent"] == [0, 0] and out["beyond"] == 0
    assert out["chunk"] == want(row.name)
    assert out["full"][0] == len(model) and out["full"][1] == model and out["full"][2] == [4096, 8, 0, 0]
    assert out["small"][0] == len(model) and out["small"][1] == model[:7] and out["none"][0] == len(model) and out["none"][1] == []
    assert out["second"][:2] == [300, W.unopt_bins_log(8, 300)]
    assert out["invalid"] == -G.ST_INVALID_ARGUMENT
