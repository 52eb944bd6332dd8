"""-m "not gpu": the plain model of the lookback search (tests/lookback_model.py) and its rows, pinned before the device is judged by them.

  * the constants read from the sources have the values and the relations the rows rely on;
  * on every row the model's lookbacks equal the oracle's choose_lookbacks page for page, the delta inverts, and the oracle's bytes decode back
    to the input; no row takes the reference's heapsort histogram branch (the GPU module compares bytes and skips nothing);
  * every row's event log contains what its name claims -- the edge lookback at every lane, the rounds of the noisy tile, the crossing at the
    named lane, the lookback at the planted position -- and the model's route is the one the name claims;
  * every body occurs on every route that can carry it (the ones no data reaches are listed with the reason), and every call the GPU module
    makes has the shape its rows were built for;
  * the u16 table with its sweep says exactly what the exact table says on the 2^17 rows, and without the sweep it does not."""
import collections

import numpy as np
import pytest

import gpu_util as U
import latent_window_util as W
import lookback_model as M
import oracle_lib as O

BODIES = ("threshold", "handback", "window", "sweep", "bucket", "hazard", "crossing", "tie", "screen")


def test_the_constants_the_rows_are_built_on():
    assert (M.kRing, M.kCounts, M.kWaves) == ({"small": 1024, "large": 2048}, {"small": 8192, "large": 4096}, 4)
    assert M.kNear == {"small": 768, "large": 1792} and all(M.kNear[k] == M.kRing[k] - 64 * M.kWaves for k in M.kRing)
    assert (M.kLbNear, M.kLbCountsLds) == ({"LbFull": 960, "LbSmall": 192}, {"LbFull": 1024, "LbSmall": 256})
    assert (M.kLbPipeSmallMaxPage, M.kLbSmallMaxPage, M.kLbSeqMaxPage, M.kSmallWmax, M.kScreenSpan) == (8192, 8192, 8192, 13, 4)
    assert (M.kLbSeqTiles, M.kLbAbortWindow, M.kLbAbortRounds, M.kLhWorkers, M.kLhChunk) == (8, 8, 24, 15, 5)
    # a u16 age never aliases: the oldest entry a lookup can meet is window_n + 1 (the sweep's marker) plus the positions up to the next sweep
    assert M.WINDOW15 + 1 + M.kLbSweepPeriod + 64 * M.kLhWorkers + 64 < 1 << 16 and M.WINDOW15 + 1 + M.kLbSweepPeriod + 64 < 1 << 16
    assert M.kCounts["small"] >= M.kLbPipeSmallMaxPage            # far counts cannot occur on the small pipeline
    assert (1 << M.kSmallWmax) <= M.kLbPipeSmallMaxPage           # ... whose chunks have at most 8192 numbers
    assert M.BODY_START == 1 + 64 * M.T0 and M.T0 > M.kLbSeqTiles + M.kLbAbortWindow   # a body never decides the route
    assert [M.window_log(n) for n in (2, 16, 17, 8192, 8193, 16384, 16385, 1 << 17)] == [4, 4, 5, 13, 14, 14, 15, 15]
    assert M.equal_pages(32770, 4098) == [4097, 4097] + [4096] * 6
    # rounds: one more than the changes, or as many when the last change is at the tile's last lane
    assert M.tile_rounds([1] * 64 + [2] * 64 + [2] * 63 + [3]) == [1, 2, 1]


def test_the_search_on_known_answers():
    # u64: Lmax at 100 and 0 at 1000 choose lookback 900 (bucket - 1 wraps in 64 bits); the same on u32 does not
    for bits, linked in ((64, True), (32, False)):
        rng = np.random.default_rng(bits)
        lat = M.wide(rng, 1200, bits); lat[100] = (1 << bits) - 1; lat[1000] = 0
        lbs = M.choose_lookbacks(lat, bits, M.window_log(1200))
        assert (lbs[999] == 900) == linked, (bits, lbs[999])
        assert lbs == O.choose_lookbacks(np.array(lat, M.UINT[bits]), M.window_log(1200)).tolist()
    # the delta and its inverse
    lat = [5, 9, 5, 200, 9, 7]; lbs = [1, 2, 1, 3, 5]
    state, d = M.apply_lookbacks(lat, lbs, 8)
    assert state == [5] and d == [(9 - 5 + 128) % 256, 128, (200 - 5 + 128) % 256, (9 - 9 + 128) % 256, (7 - 5 + 128) % 256]
    assert M.undo_lookbacks(state, d, lbs, 8) == lat


def test_the_oracle_hook_takes_all_four_widths():
    for bits in (8, 16, 32, 64):
        rng = np.random.default_rng(bits)
        lat = rng.integers(0, 1 << min(bits, 20), 3000).astype(M.UINT[bits])
        assert O.choose_lookbacks(lat, M.window_log(3000)).tolist() == M.choose_lookbacks(lat.tolist(), bits, M.window_log(3000)), bits


def test_row_names_are_unique_and_say_their_route():
    rows = M.all_rows()
    assert len(M.BY_NAME()) == len(rows) and {r.body for r in rows} == set(BODIES)
    for r in rows:
        assert sum(r.pages) == r.arr.size and (len(r.pages) == 1) == (r.paging is None) and len(r.routes) == len(r.pages), r.name
        assert set(r.routes) == {r.name.rsplit("-", 1)[1]} or r.name.startswith(("t-", "y-")) and f"-{r.routes[0]}-" in r.name, r.name


@pytest.mark.parametrize("body", BODIES)
def test_model_equals_oracle_and_every_row_shows_what_it_claims(body):
    """The model's lookbacks against the oracle's page for page; the route; the claims; the delta's inverse."""
    for r in (r for r in M.all_rows() if r.body == body):
        res = M.analysis_of(r.name)
        p, _ = W.ordered_latents(r.arr, r.kw)
        op, _, _, _ = O.split_latents(r.arr, O.make_config(enable_8_bit=True, **{k: v for k, v in r.kw.items() if k != "max_page_n"}))
        assert np.array_equal(op, p), r.name
        bits = p.dtype.itemsize * 8; wlog = M.window_log(r.arr.size); start = 0
        for pn, pr in zip(r.pages, res):
            page = p[start:start + pn]; start += pn
            assert O.choose_lookbacks(page, wlog).tolist() == pr.lbs, r.name
            if pn <= 5000:
                state, d = M.apply_lookbacks(page.tolist(), pr.lbs, bits)
                assert M.undo_lookbacks(state, d, pr.lbs, bits) == page.tolist(), r.name
        assert [pr.route for pr in res] == r.routes, (r.name, [pr.route for pr in res])
        for c in r.claims:
            pr = res[c[1]]
            if c[0] == "lb":      # the edge lookback at least 64 times, at every lane
                assert pr.log.chosen[c[2]] >= 64 and len(pr.log.lanes[c[2]]) == 64, (r.name, c, pr.log.chosen[c[2]])
                tail = pr.lbs[-64:]
                assert tail == [c[2]] * 64, (r.name, "the edge lookback holds to the end of the page")
            elif c[0] == "at": assert pr.lbs[c[2] - 1] == c[3], (r.name, c, pr.lbs[c[2] - 1])
            elif c[0] == "not": assert pr.lbs[c[2] - 1] != c[3], (r.name, c)
            elif c[0] == "rounds":   # that tile alone: no other tile of the abort window (or the one behind it) is near the threshold
                assert pr.rounds[c[2]] == c[3], (r.name, c, pr.rounds[c[2]])
                assert all(x <= 2 for t, x in enumerate(pr.rounds[M.kLbSeqTiles:M.kLbSeqTiles + M.kLbAbortWindow + 1], M.kLbSeqTiles) if t != c[2]), (r.name, pr.rounds[8:17])
            elif c[0] == "cross":    # the count of P reaches each of these powers of two at that lane, in the body
                _, _, P, lane, counts = c
                got = {cnt: ln for i, ln, lb, cnt, _ in pr.log.crossings if lb == P and i >= M.BODY_START}
                assert all(got.get(cnt) == lane for cnt in counts), (r.name, got)
            elif c[0] == "tie":      # at that position two groups tied on goodness and proposal order decided
                assert tuple(c[2:]) in pr.log.ties, (r.name, c)
            elif c[0] == "same":     # the deltas both lookbacks give at that position are identical
                i, a, b = c[2:]; lat = p.tolist()
                assert (lat[i] - lat[i - a]) % (1 << bits) == (lat[i] - lat[i - b]) % (1 << bits), (r.name, c)
            elif c[0] == "big":      # a tile in which P is chosen at least 33 times and its count crosses a power of two (the one-wave kernel's big[] list)
                tiles = collections.Counter((i - 1) // 64 for i, lb in enumerate(pr.lbs, 1) if lb == c[2])
                assert any(tiles[(i - 1) // 64] >= 33 for i, _, lb, cnt, _ in pr.log.crossings if lb == c[2] and cnt >= 64), (r.name, c)
            else: raise AssertionError(c)


@pytest.mark.parametrize("body", BODIES)
def test_oracle_bytes_round_trip_and_no_row_takes_the_heapsort_branch(body):
    bad = []
    for r in (r for r in M.all_rows() if r.body == body):
        kw = {k: v for k, v in r.kw.items() if k != "max_page_n"}
        cfg = O.make_config(enable_8_bit=True, **kw)
        info, _, fell_back = O.chunk_plan(r.arr, cfg)
        if fell_back: bad.append(r.name)
        assert info.delta_kind == 2 and info.window_n_log == M.window_log(r.arr.size), (r.name, info.delta_kind, info.window_n_log)   # (DeltaEncoding::Lookback)
        if r.paging is None:
            f = O.simple_compress(r.arr, O.make_config(enable_8_bit=True, max_page_n=r.arr.size, **kw))
            assert U.bits_equal(O.simple_decompress(f, r.arr.dtype, cap=r.arr.size + 8), r.arr), r.name
        else:
            meta, pages, ns = O.wrapped_compress(r.arr, O.make_config(enable_8_bit=True, **r.kw), max_pages=len(r.pages) + 1, exact_pages=r.pages if r.paging == "exact" else None)
            assert ns == r.pages, (r.name, ns)
            f = O.simple_compress_exact(r.arr, cfg, r.pages)      # (the same pages as standalone chunks: what the oracle can decode)
            assert U.bits_equal(O.simple_decompress(f, r.arr.dtype, cap=r.arr.size + 8), r.arr), r.name
    assert not bad, ("rows on the reference's heapsort branch: change their seed", bad)


# body -> the (route, pipeline, one-wave layout) triples it must occur on.  What no data reaches:
#   * threshold: a period is an edge of ONE kernel -- the ring and count thresholds of the pipeline on pipeline pages, the one-wave kernel's on
#     handed-back pages; the seq kernel has no threshold (everything a decision reads is in LDS);
#   * far counts (a lookback above kCounts) on the small pipeline: its counts cover every page it takes;
#   * window_n and window_n + 1 below window_n_log 15: a page longer than window_n belongs to a chunk with the next window;
#   * sweep: only pages beyond 2^16 are ever swept for a reason, and those are the large pipeline's; the one-wave kernel keeps u32 positions;
#   * screen: the seq kernel takes pages of at most 8192 numbers, so its rows are the small shape's; 8-bit pages are always screened;
#   * a far count exists on the large pipeline only;
# NOT BUILT (reachable, and open):
#   * a flip in which the HASHED group takes part.  With identical deltas a[i] - a[i - p] = a[i] - a[i - q], p < q, the table names the latest
#     occurrence, p, so q is proposed by a brute-force or a repeating slot only, and a lookback that has won sits in a repeating slot (evaluated
#     before the hashed ones).  Two alternating lookbacks therefore flip as brute force against repeating, which is what rows_tie() builds.  Three
#     OTHER changes between a win of p and a win of q would push p out of the repeating slots while q stays in one: p is then proposed by a hashed
#     slot only, q keeps the identical-delta positions by order until p's count has the longer bit length.  No row does that yet; ties of
#     goodness with the hashed group occur in the rows' logs and are counted below;
#   * ties and crossings on the seq and the one-wave kernel: both decide element by element with the counts as they are -- there is no ready-made
#     maximum that could be stale;
#   * hand-back at 4097 numbers: 64 tiles are not more than 4 * (kLbSeqTiles + kLbAbortWindow).
AXES = {
    "threshold": {("pipe", "small", "LbSmall"), ("pipe", "large", "LbFull"), ("back", "small", "LbSmall"), ("back", "large", "LbFull")},
    "handback": {("pipe", "small", "LbSmall"), ("back", "small", "LbSmall")},
    "window": {("pipe", "small", "LbSmall"), ("pipe", "large", "LbFull"), ("back", "large", "LbFull"), ("pipe", "large", "LbSmall")},
    "sweep": {("pipe", "large", "LbFull")},
    "bucket": {("pipe", "small", "LbSmall"), ("back", "small", "LbSmall"), ("seq", "small", "LbSmall")},
    "hazard": {("pipe", "small", "LbSmall")},
    "crossing": {("pipe", "small", "LbSmall"), ("pipe", "large", "LbFull")},
    "tie": {("pipe", "small", "LbSmall"), ("pipe", "large", "LbFull")},
    "screen": {("seq", "small", "LbSmall"), ("back", "small", "LbSmall"), ("back", "large", "LbFull"), ("pipe", "small", "LbSmall"), ("pipe", "large", "LbFull")},
}


def test_every_body_occurs_on_every_route_that_can_carry_it():
    seen = collections.defaultdict(set); widths = collections.defaultdict(set)
    for r in M.all_rows():
        for rt in r.routes: seen[r.body].add((rt,) + r.shape)
        widths[r.body].add(r.arr.dtype.itemsize * 8)
    assert dict(seen) == AXES
    assert all({32, 64} <= w for w in widths.values()), widths                       # every body on u64 and u32
    assert widths["bucket"] == {8, 16, 32, 64} and widths["screen"] == {8, 16, 32, 64}
    kinds = {r.arr.dtype.kind for r in M.all_rows()}
    assert kinds == {"u", "i", "f"} and any(r.kw["mode"] == 4 for r in M.all_rows())
    # every threshold period, one step either side, on u64 and u32
    names = {r.name for r in M.rows_thresholds()}
    for (route, kind), periods in M.threshold_periods().items():
        assert len(periods) in (3, 6)
        for P in periods:
            assert {f"t-u64-{route}-{kind}-P{P}", f"t-u32-{route}-{kind}-P{P}"} <= names
    # the hand-back edge: 23, 24, 25 rounds x tiles 8, 15, 16 x 4097 and 4098 numbers; handed back exactly where all three conditions hold
    for r in M.rows_handback():
        _, _, n, tile, rounds, _, route = r.name.split("-")
        assert (route == "back") == (int(rounds[6:]) > M.kLbAbortRounds and int(tile[4:]) < M.kLbSeqTiles + M.kLbAbortWindow and int(n[1:]) > 4097), r.name
    assert len(M.rows_handback()) == 2 * 2 * 3 * 3
    # crossings: brute, hashed near and far lookbacks at the first lane, in the middle, at the last lane, for every power of two up to 4096; the flip of a tie at the same three lanes on both pipelines; and ties between all group pairs in the logs
    crossed = set(); ties = collections.Counter()
    kind_of = lambda P: "brute" if P <= M.BRUTE else "far" if P > M.kCounts["large"] else "near"
    for r in M.all_rows():
        for pr in M.analysis_of(r.name):
            ties.update((a, b) for _, a, b in pr.log.ties)
        for c in r.claims:
            if c[0] == "cross": crossed |= {(kind_of(c[2]), c[3], cnt) for cnt in c[4]}
    powers = [1 << k for k in range(1, 13)]
    assert crossed == {(k, ln, cnt) for k in ("brute", "near", "far") for ln in M.CROSS_LANES for cnt in powers}, crossed
    assert M.CROSS_TOP == 4096 and all(M.CROSS_FIRST[k][1] == (2, 4, 8, 16, 32) for k in ("brute", "near", "far"))
    flips = {(r.arr.dtype.itemsize * 8, r.shape[0], (c[2] - 1) % 64) for r in M.rows_tie() for c in r.claims if c[0] == "tie"}
    assert flips == {(w, sh, ln) for w in (64, 32) for sh in ("small", "large") for ln in M.CROSS_LANES}, flips
    for r in M.rows_tie():
        kinds = [c[0] for c in r.claims]
        assert kinds == ["at", "at", "tie", "same", "same"] and r.claims[1][2] == r.claims[2][2] > 1 + 64 * (M.kLbSeqTiles + 1), r.name
    print(dict(ties))
    for pair in (("brute", "repeating"), ("brute", "hashed"), ("repeating", "hashed")):
        assert ties[pair] >= 64, (pair, ties)


def test_every_call_has_the_shape_its_rows_were_built_for():
    groups = {M.group_key(g[0]): g for g in M.groups()}
    classic = tuple(sorted(M.LOOKBACK.items()))
    small, large = (classic, None, ("small", "LbSmall")), (classic, None, ("large", "LbFull"))
    assert set(groups) == {small, large, (classic, "exact", ("large", "LbFull")), (tuple(sorted(dict(M.LOOKBACK, max_page_n=4098).items())), "equal", ("large", "LbSmall")),
                           (tuple(sorted(dict(mode=4, mode_u64=M.INT_MULT_BASE, delta=3).items())), None, ("small", "LbSmall"))}
    for g in groups.values():
        shape = M.call_shape([r.arr.size for r in g], [p for r in g for p in r.pages])
        assert all(r.shape == shape for r in g), (g[0].name, shape)
    routes = {k: collections.Counter(rt for r in g for rt in r.routes) for k, g in groups.items()}
    assert set(routes[small]) == {"pipe", "seq", "back"} and set(routes[large]) == {"pipe", "back"}     # one call per config mixes the routes
    # pages of at most 8192 numbers beside larger ones: every page goes to the large pipeline
    assert min(r.arr.size for r in groups[large]) <= 8192 < max(r.arr.size for r in groups[large])


def test_the_swept_u16_table_is_exact_and_an_unswept_one_is_not():
    """On the 2^17 rows the six proposal streams of a u16 table swept as the pre-pass sweeps it equal the exact table's at every position; a
    table that is never swept differs at the planted returns (it says 65536 + d is d), which is what these rows are for."""
    for r in M.rows_sweep():
        p, _ = W.ordered_latents(r.arr, r.kw); lat = p.tolist()
        exact = []; M.choose_lookbacks(lat, p.dtype.itemsize * 8, 15, 0, None, exact)
        exact = [[1] + [e[s] for e in exact] for s in range(6)]
        swept = M.u16_table_proposals(lat, 15)
        assert swept == exact, r.name
        unswept = M.u16_table_proposals(lat, 15, sweep=False)
        differ = {i for s in range(6) for i in range(len(lat)) if unswept[s][i] != exact[s][i]}
        planted = [c[2] for c in r.claims if c[0] == "not" and c[3] in M.ALIAS_D]
        assert len(planted) == len(M.ALIAS_D) - 1 and set(planted) <= differ, (r.name, sorted(differ)[:10])
        print(r.name, len(differ), "positions tell a table without the sweep apart")
