"""-m "not gpu": the model of the encoder's front (tests/latent_window_util.py) and its rows, pinned before the device is judged by them.

  * the constants read from the .hip sources have the values and the relations the model assumes;
  * the model's ordered latents equal the oracle's split on every row;
  * every row's route (and, for the tier rows, tier) computed by the model is the one the row's name claims -- the claims are made by the
    builders from how they placed the latents, the model computes from the finished array;
  * the rows cover what they promise: every edge offset, position, clamp point, order, residue, size and level;
  * no row makes the reference's histogram take its order-dependent heapsort branch (the device follows the multiset rule: such a row could
    not be compared byte for byte, and the GPU module skips nothing), and the oracle round-trips every row."""
import collections

import numpy as np
import pytest

import format_limits_util as F
import gpu_util as U
import latent_window_util as W
import oracle_lib as O

SECTIONS = {"a": W.rows_a, "b": W.rows_b, "c": W.rows_c, "d": W.rows_d, "e": W.rows_e, "n": W.rows_never}


def test_the_constants_the_model_is_built_on():
    assert (W.kC16KeyRange, W.kBias, W.kDirectHistRange, W.kMidHistRange, W.kWideHistRange, W.kSmallHistCap) == (32768, 16384, 4096, 16384, 32768, 8192)
    assert (W.kSplitE, W.kSplitTile, W.kPresampleMinN, W.kPresampleTail, W.kPresampleLanes, W.kMaxUnoptBinsLog) == (8, 2048, 4096, 8, 64, 8)
    assert W.kC16KeyRange == 2 * W.kBias                       # the window is [ref - bias, ref + bias - 1]
    assert W.kC16KeyRange <= 1 << 15                           # keys travel in 16 bits with room for key + 1 (the strict replay)
    assert W.kWideHistRange <= W.kC16KeyRange                  # a chunk that holds its window never needs the select / sort kernels
    assert W.kDirectHistRange < W.kMidHistRange < W.kWideHistRange and W.kDirectHistRange & (W.kDirectHistRange - 1) == 0
    assert W.kPresampleMinN > W.kPresampleTail + W.kPresampleLanes and 7 <= W.kPresampleTail   # pos + order stays inside the chunk for orders up to 7
    # the sizes of the rows: two full tiles and a partial one, under the presample's floor, and the cap from both sides
    assert W.N_BIG == 2 * W.kSplitTile + 512 and W.N_BIG >= W.kPresampleMinN > W.N_SMALL
    assert W.TIER_N_LAT[:2] == (W.kSmallHistCap, W.kSmallHistCap + 1)
    # the presample reads 64 distinct positions, the first latent's among them
    for order in (0, 1, 7):
        idx = W.sample_indices(W.N_BIG, order)
        assert len(set(idx)) == 64 and idx[0] == order and max(idx) < W.N_BIG
    assert [W.tier_of(r, n) for r, n in ((4095, 20000), (4096, 8192), (4096, 8193), (16383, 8193), (16384, 8193), (32767, 20000), (32768, 8192), (32768, 8193))] == \
        ["direct", "small", "mid", "mid", "wide", "wide", "small", "select"]
    assert [W.unopt_bins_log(l, n) for l, n in ((8, 300), (8, 4096), (0, 20000), (12, 20000), (12, 1 << 20))] == [6, 8, 0, 11, 12]


def test_row_names_are_unique_and_say_their_route():
    rows = W.all_rows()
    assert len(W.BY_NAME()) == len(rows)
    for r in rows:
        assert r.route in W.ROUTES and (r.name.endswith("-" + r.route) or r.section == "e" and f"-{r.route}-" in r.name), r.name
        assert sum(r.pages) == r.arr.size and (len(r.pages) == 1) == (r.paging is None), r.name
    # an offset inside the window never leaves, one outside always does
    for r in rows:
        if r.section in "ac" and ("-ref" in r.name or "-diff+" in r.name or "-diff-" in r.name):
            inside = any(f"{o:+d}@" in r.name for o in W.INSIDE) and "junk-diff" not in r.name
            assert (r.route == "c16") == inside, r.name


@pytest.mark.parametrize("section", sorted(SECTIONS))
def test_every_row_takes_the_route_and_tier_it_claims(section):
    bad = []
    for r in SECTIONS[section]():
        a = W.analysis_of(r.name)
        if a.route != r.route or (r.tiers is not None and a.tiers != r.tiers):
            bad.append((r.name, a.route, a.tiers, a.bad1[:4], a.bad2[:4]))
        # a row that leaves through ONE placed latent leaves through nothing else
        if r.section in "acd" and r.route in ("redo", "sample") and "junk" not in r.name and "first@max" not in r.name:
            assert len(a.bad1) + len(a.bad2) == 1, (r.name, a.bad1[:4], a.bad2[:4])
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("section", sorted(SECTIONS))
def test_model_latents_equal_the_oracle_split_and_no_row_takes_the_heapsort_branch(section):
    bad = []
    for r in SECTIONS[section]():
        kw = {k: v for k, v in r.kw.items() if k != "max_page_n"}
        cfg = O.make_config(enable_8_bit=True, **kw)
        p, s = W.ordered_latents(r.arr, r.kw)
        op, os_, mk, _ = O.split_latents(r.arr, cfg)
        assert mk == {1: 0, F.MODE_INT_MULT: 1, F.MODE_FLOAT_MULT: 2, F.MODE_FLOAT_QUANT: 3}[r.kw["mode"]], (r.name, mk)
        assert np.array_equal(op, p) and (s is None or np.array_equal(os_, s)), r.name
        # (the plan is the one-page chunk's; the pages of a wrapped row drop a few more positions from the same multiset)
        info, _, fell_back = O.chunk_plan(r.arr, cfg)
        if fell_back: bad.append(r.name)
        assert info.mode_kind == mk, (r.name, info.mode_kind)     # the encoder keeps the mode: the secondary the model speaks of exists
        f = O.simple_compress(r.arr, O.make_config(enable_8_bit=True, max_page_n=r.arr.size, **kw))
        assert U.bits_equal(O.simple_decompress(f, r.arr.dtype, cap=r.arr.size + 8), r.arr), r.name
        if r.paging is not None:
            meta, pages, ns = O.wrapped_compress(r.arr, O.make_config(enable_8_bit=True, **r.kw), max_pages=len(r.pages) + 1,
                                                 exact_pages=r.pages if r.paging == "exact" else None)
            assert ns == r.pages, (r.name, ns)
    assert not bad, ("rows on the reference's heapsort branch: change their seed", bad)


def test_window_rows_cover_every_edge_and_position():
    names = [r.name for r in W.rows_a()]
    for dt in W.WINDOW_TYPES:
        for off in W.INSIDE + W.OUTSIDE:
            for place in ("sampled", "unsampled", "i2047", "i2048", "last"):
                assert any(n.startswith(f"a-{W.tname(dt)}-n{W.N_BIG}-ref{off:+d}@{place}-") for n in names), (dt, off, place)
            assert any(n.startswith(f"a-{W.tname(dt)}-n{W.N_SMALL}-ref{off:+d}@any-") for n in names)
    # a sampled position leaves through the presample, the one next to it through its tile
    by = W.BY_NAME()
    for dt in W.WINDOW_TYPES:
        for off in W.OUTSIDE:
            assert by[f"a-{W.tname(dt)}-n{W.N_BIG}-ref{off:+d}@sampled-sample"].route == "sample"
            for place in ("unsampled", "i2047", "i2048", "last"):
                assert f"a-{W.tname(dt)}-n{W.N_BIG}-ref{off:+d}@{place}-redo" in by
    assert W.unsampled_index(W.N_BIG, 0) == W.sampled_index(W.N_BIG, 0) + 1
    # the clamp: every first latent with both ends of its window, and each step beyond that exists
    names = [r.name for r in W.rows_b()]
    for dt in W.WINDOW_TYPES:
        for first in ("0", "1", "bias-1", "bias", "max-bias", "max-bias+1", "max"):
            have = {n.split("-")[-2] for n in names if n.startswith(f"b-{W.tname(dt)}-n{W.N_SMALL}-first@{first}-")}
            assert have == ({"base", "lo", "hi", "above"} if first in ("0", "1", "bias-1", "bias") else {"base", "lo", "hi", "below", "above"}), (dt, first, have)
    assert sum("covers[" in n for n in names) == 8
    # the type's maximum as first latent is itself outside the clamped window: with the presample, lane 0 finds it
    assert by[f"b-uint16-n{W.N_BIG}-first@max-base-sample"].route == "sample" and by[f"b-uint16-n{W.N_SMALL}-first@max-base-redo"].route == "redo"


def test_delta_rows_have_junk_that_would_fail_and_stored_differences_that_fit():
    for r in W.rows_c():
        a = W.analysis_of(r.name)
        if "junk" in r.name:
            assert a.junk_pages_outside == len(r.pages), r.name              # every page has unstored positions far outside the window
            assert F.width(r.arr.dtype) == 16 or a.junk_inside == 0, r.name
        if "first-stored" in r.name:
            order = W.order_of(r.kw); start = r.pages[0] if "page2" in r.name else 0
            assert a.bad1 == [start + order], (r.name, a.bad1)
    names = [r.name for r in W.rows_c()]
    for dt in W.ORDER_TYPES:
        for order in W.ORDERS:
            for paging in (f"n{W.N_BIG}", f"exact{W.EXACT_PAGES[0]}", f"equal{W.EQUAL_MAX_PAGE_N}"):
                for off in W.INSIDE + W.OUTSIDE:
                    assert any(n.startswith(f"c-{W.tname(dt)}-o{order}-{paging}-diff{off:+d}@") for n in names), (dt, order, paging, off)
    assert W.EXACT_PAGES[0] % 2 == 1 and W.EQUAL_MAX_PAGE_N % 2 == 1                  # pages that start at odd indices
    assert all(r.route != "sample" for r in W.rows_c() if r.paging is not None)      # no presample for chunks of several pages


def test_tier_rows_cover_ranges_residues_sizes_kinds_and_levels():
    rows = W.rows_e()
    seen = collections.defaultdict(set)
    for r in rows:
        _, kind, form, res, lat, level, _, tier = r.name.replace("d1-u32", "d1u32").replace("imult-i64", "imulti64").split("-")
        a = W.analysis_of(r.name)
        var = 1 if kind == "imulti64" else 0
        rng = int(form.lstrip("compactful"))
        assert a.ranges[var] == rng and a.n_lat[var] == int(lat[3:]) and a.tiers[var] == tier, (r.name, a.ranges, a.n_lat, a.tiers)
        if form.startswith("compact"):
            assert a.route == "c16" and a.min_keys[var] % W.kDirectHistRange == int(res[3:]), (r.name, a.min_keys)
        seen[form].add((kind, int(res[3:]), int(lat[3:]), level, tier))
    assert set(seen) == {f"compact{r}" for r in W.COMPACT_RANGES} | {f"full{r}" for r in W.FULL_RANGES}
    for form, s in seen.items():
        assert {x[0] for x in s} == {"u64", "d1u32", "imulti64"} and {x[2] for x in s} == set(W.TIER_N_LAT) and {x[3] for x in s} == {"L0", "L8"}, form
        rng = int(form.lstrip("compactful"))
        # every residue the window leaves room for: all four up to a range of 2^14, fewer as the range fills the window
        want = {W.compact_split(rng, q)[2] for q in W.RESIDUES} if form.startswith("compact") else set(W.RESIDUES)
        assert {x[1] for x in s} == want, (form, {x[1] for x in s}, want)
        if rng < W.kMidHistRange: assert want == set(W.RESIDUES)
    tiers = collections.Counter(W.analysis_of(r.name).tiers[1 if "imult" in r.name else 0] for r in rows)
    assert set(tiers) == set(W.TIERS), tiers
    # a secondary reaches every tier above `direct`
    assert {W.analysis_of(r.name).tiers[1] for r in rows if "imult" in r.name} == set(W.TIERS)


def test_secondary_rows_end_the_speculation_through_either_variable():
    through = collections.Counter()
    for r in W.rows_d():
        a = W.analysis_of(r.name)
        if r.route != "c16":
            through[("primary" if a.bad1 else "secondary", r.kw["mode"], r.route)] += 1
            assert bool(a.bad1) == ("primary" in r.name), r.name
    for mode in (F.MODE_INT_MULT, F.MODE_FLOAT_QUANT, F.MODE_FLOAT_MULT):
        for var in ("primary", "secondary"):
            for rt in ("redo", "sample"):
                assert through[(var, mode, rt)] >= 2, (var, mode, rt, through)
