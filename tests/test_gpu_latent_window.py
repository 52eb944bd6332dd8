"""-m gpu: the speculative 16-bit latent window of the encoder and the histogram tiers behind it, at their edges.

The rows and the model that predicts their way through the encoder are in tests/latent_window_util.py; tests/test_latent_window.py pins both
on the CPU (routes, tiers, no heapsort branch, oracle round trip) before anything here runs.  Every row has one latent -- or one range -- exactly
at, or one step beyond, a decision of enc_presample_kernel, enc_split_kernel<c16> or hist_var:

  (a) ref - 2^14, ref + 2^14 - 1 and one step beyond each, at a presampled position, next to one, at 2047 / 2048, at the last element of
      a partial tile, and at 300 numbers (no presample); nine number types and u8;
  (b) the clamp of the reference 2^14 from both ends of the latent type, and 16-bit types covered in halves;
  (c) consecutive orders 1, 2 and 7 around the toggle, with huge raw values at the unstored positions of every page, as one page and as
      wrapped chunks of three pages (PagingSpec::Exact and EqualPagesUpTo, pages starting at odd indices);
  (d) int-mult, float-quant and float-mult secondaries, and the primary beside a fitting secondary;
  (e) numeric ranges on both sides of kDirectHistRange, kMidHistRange and kWideHistRange at kSmallHistCap, one more, and 20 000 latents, as
      16-bit keys (compact, every residue of the smallest key modulo 4096 the window leaves room for) and at full width after a redo or a
      sample, as a classic u64, as order-1 differences of a u32 and as the secondary of an int-mult i64, at levels 8 and 0.

Every chunk's bytes equal the oracle's and decode bit for bit to the input.  Rows that share a route (or a tier) and a config share one
SYNCHRONOUS call, and the kernels that call launched certify the prediction: a synchronous call launches the split and histogram kernels
the device flagged and no others, so the launched set must EQUAL the predicted one -- a row that does not reach its route fails, it does not
quietly test something else.  (f) then mixes all routes in one call per config, synchronous and asynchronous, with copies of one row spread
through it.  Nothing is skipped."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_util as U
import latent_window_util as W
import oracle_lib as O
from pcodec_amd import _lib as G
from test_gpu_width_paths import decode_call, encode_call
from test_gpu_wrapped_batched import decode_pages, wrapped_batch
from test_gpu_wrapped_writer import Call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


@functools.lru_cache(maxsize=None)
def want(name):
    """The oracle's bytes of a row, once: a standalone chunk, or (ChunkMeta, [pages]) of a wrapped one."""
    r = W.BY_NAME()[name]
    if r.paging is None:
        return U.oracle_chunk(r.arr, O.make_config(enable_8_bit=True, **r.kw))
    meta, pages, ns = O.wrapped_compress(r.arr, O.make_config(enable_8_bit=True, **r.kw), max_pages=len(r.pages) + 1, exact_pages=r.pages if r.paging == "exact" else None)
    assert ns == r.pages
    return meta, pages


def by_config(rows):
    groups = collections.OrderedDict()
    for r in rows:
        groups.setdefault(W.config_key(r), []).append(r)
    return list(groups.values())


def expected_kernels(rows):
    """(split kernels, histogram kernels or None) a synchronous call over `rows` launches, by the model."""
    split = W.split_kernels_for(r.route for r in rows)
    tiers = [t for r in rows for t, present in zip(W.analysis_of(r.name).tiers, (True, r.kw["mode"] != 1)) if present]
    hist = None if any(t is None for t in tiers) else {k for t in tiers for k in W.TIER_KERNELS[t]}
    return split, hist


def check_kernels(rows, names):
    split, hist = expected_kernels(rows)
    got_split = set(names) & set(W.SPLIT_KERNELS); got_hist = set(names) & set(W.HIST_KERNELS)
    print(f"{len(rows)} chunks, routes {sorted({r.route for r in rows})}: {sorted(got_split)} {sorted(got_hist)}")
    assert got_split == split, (rows[0].name, sorted(got_split), sorted(split))
    if hist is not None:
        assert got_hist == hist, (rows[0].name, sorted(got_hist), sorted(hist))


def wrapped_cfg(rows):
    return G.make_config(enable_8_bit=True, **rows[0].kw)


def run_group(L, rows):
    """One synchronous call over rows of ONE config: bytes against the oracle, the launched kernels against the model, and the round trip."""
    assert len(by_config(rows)) == 1
    if rows[0].paging is None:
        chunks, names = encode_call([r.arr for r in rows], G.make_config(enable_8_bit=True, **rows[0].kw))
        bad = [r.name for r, c in zip(rows, chunks) if c != want(r.name)]
        assert not bad, (len(bad), bad[:6])
        check_kernels(rows, names)
        decode_call(chunks, [r.arr for r in rows])
        return chunks
    c = Call(L, [r.arr for r in rows], wrapped_cfg(rows), [r.pages if r.paging == "exact" else None for r in rows])
    L.pco_gfx_profile_begin()
    G.check(c.encode())
    names = U.profile_names(L)
    pieces = c.pieces()
    bad = [r.name for r, (meta, pages, ns) in zip(rows, pieces) if (meta, pages) != want(r.name) or ns != r.pages]
    assert not bad, (len(bad), bad[:6])
    check_kernels(rows, names)
    c.decode_and_compare()
    return [(m, p) for m, p, _ in pieces]


ROUTE_CASES = sorted({(r.section, r.route) for r in W.all_rows()})


@pytest.mark.parametrize("section,route", ROUTE_CASES, ids=[f"{s}-{r}" for s, r in ROUTE_CASES])
def test_rows_of_one_route_take_that_route_and_encode_like_the_oracle(L, section, route):
    """all "c16": enc_split_kernel<c16> alone; all "redo": it and enc_split_kernel(redo), not enc_split_kernel; all "sample" (and "never"):
    enc_split_kernel alone.  The histogram kernels are the union of the rows' tiers, exactly."""
    rows = [r for r in W.all_rows() if (r.section, r.route) == (section, route)]
    assert rows
    for group in by_config(rows):
        assert W.split_kernels_for(r.route for r in group) == {"c16": {"enc_split_kernel<c16>"}, "redo": {"enc_split_kernel<c16>", "enc_split_kernel(redo)"},
                                                             "sample": {"enc_split_kernel"}, "never": {"enc_split_kernel"}}[route]
        run_group(L, group)


def tier_row_tier(r):
    return r.tiers[1] if r.tiers[1] is not None else r.tiers[0]


@pytest.mark.parametrize("tier", W.TIERS)
def test_rows_of_one_tier_launch_that_tier_and_none_above(L, tier):
    """Calls whose rows all predict one tier (the int-mult rows' primary is `direct`, which launches nothing of its own): that tier's kernel
    and no other histogram kernel -- the compact rows with 16-bit keys, the full rows at full width after a redo or a sample."""
    rows = [r for r in W.rows_e() if tier_row_tier(r) == tier]
    assert rows
    for group in by_config(rows):
        _, hist = expected_kernels(group)
        assert hist == set(W.TIER_KERNELS[tier]), (tier, hist)
        run_group(L, group)


def mixed_call(rows, seed):
    """The rows of one config shuffled, with a copy of its first "c16" row after every fourth: (rows of the call, indices of the copies)."""
    rng = np.random.default_rng(seed)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    copy = next(r for r in rows if r.route == "c16")
    out, copies = [], []
    for i, r in enumerate(rows):
        out.append(r)
        if i % 4 == 3:
            copies.append(len(out)); out.append(copy)
    return out, copies


def mixed_groups(paged):
    rows = [r for r in W.all_rows() if r.section in "abcd" and (r.paging is not None) == paged]
    return [g for g in by_config(rows) if any(r.route == "c16" for r in g)]


def test_every_route_in_one_call_synchronous_and_asynchronous(L):
    """(f) all rows of (a)-(d) that share a config in ONE shuffled call, routes mixed: the synchronous form (a full-width slot for exactly the
    chunks that left) and the asynchronous form (results == NULL: a slot per chunk up front, every kernel launched) both give the oracle's
    bytes -- those the per-route calls gave -- and the copies of one row are byte-identical wherever they sit."""
    import torch
    groups = mixed_groups(paged=False)
    assert sum(len(g) for g in groups) == sum(r.section in "abcd" and r.paging is None for r in W.all_rows())   # no config is left out
    assert all({r.route for r in g} == {"c16", "redo", "sample"} for g in groups)
    for gi, group in enumerate(groups):
        rows, copies = mixed_call(group, gi)
        cfg = G.make_config(enable_8_bit=True, **rows[0].kw)
        wants = [want(r.name) for r in rows]
        chunks, names = encode_call([r.arr for r in rows], cfg)
        assert [r.name for r, c, w_ in zip(rows, chunks, wants) if c != w_] == []
        check_kernels(rows, names)
        s = U.Staged(L, [r.arr for r in rows])
        tasks = s.enc_tasks()
        G.check(L.pco_gfx_compress_chunks(s.k, U.ptr(tasks), C.byref(cfg), None, s.d_res.data_ptr(), None))
        torch.cuda.synchronize()
        res = s.results()
        assert (res["status"] == 0).all(), res["status"]
        got = s.slot_bytes(res["n_out"])
        assert [r.name for r, c, w_ in zip(rows, got, wants) if c != w_] == []
        assert len({got[i] for i in copies}) == 1 and len({chunks[i] for i in copies}) == 1 and len(copies) >= len(group) // 4


def test_every_route_in_one_wrapped_call_synchronous_and_asynchronous(L):
    """The same for the chunks of several pages: pco_gfx_compress_wrapped_chunks_ex with host infos, then with the piece directory on the device."""
    import torch
    groups = mixed_groups(paged=True)
    assert len(groups) == 2 * len(W.ORDERS)
    for gi, group in enumerate(groups):
        rows, copies = mixed_call(group, 100 + gi)
        assert {r.route for r in rows} == {"c16", "redo"}
        wants = [want(r.name) for r in rows]
        for sync in (True, False):
            c = Call(L, [r.arr for r in rows], wrapped_cfg(rows), [r.pages if r.paging == "exact" else None for r in rows])
            L.pco_gfx_profile_begin()
            G.check(c.encode(sync=sync))
            names = U.profile_names(L)
            torch.cuda.synchronize()
            pieces = c.pieces(None if sync else c.device_infos())
            assert [r.name for r, (m, p, ns), w_ in zip(rows, pieces, wants) if (m, p) != w_ or ns != r.pages] == [], sync
            if sync: check_kernels(rows, names)
            assert len({(pieces[i][0], tuple(pieces[i][1])) for i in copies}) == 1
            c.decode_and_compare(None if sync else c.device_infos())


@pytest.mark.parametrize("order", W.ORDERS)
def test_pages_cut_by_max_page_n_through_the_older_wrapped_entry_point(L, order):
    """The EqualPagesUpTo rows of (c) through pco_gfx_compress_wrapped_chunks: the same bytes, every page decodes."""
    rows = [r for r in W.rows_c() if r.paging == "equal" and W.order_of(r.kw) == order]
    assert len(rows) == len(W.ORDER_TYPES) * 7 and {r.route for r in rows} == {"c16", "redo"}
    out, state = wrapped_batch(L, [r.arr for r in rows], wrapped_cfg(rows))
    assert [r.name for r, (m, p, ns) in zip(rows, out) if (m, p) != want(r.name) or ns != r.pages] == []
    code, res, back, _ = decode_pages(L, [r.arr for r in rows], state)
    assert code == 0 and all(x.status == 0 for x in res)
    assert all(U.bits_equal(b, r.arr) for b, r in zip(back, rows))
