"""-m "not gpu": the plain model of the quantile histogram (tests/hist_model.py) pinned to the oracle, and every row of
tests/hist_edges_util.py certified to stand on the comparison it is named for, before tests/test_gpu_hist_edges.py runs any of them.

  * the model reproduces the reference's known answers (histograms.rs: test_bin_idx_and_c_count, test_histogram_quicksort);
  * for every row and every present variable, at the variable's own n_bins_log: model == O.histogram(rule=1) == O.histogram(rule=0), neither
    call reports the heapsort branch, and O.chunk_plan does not either.  No row is skipped or excused: the share allowed to take the heapsort
    branch is zero;
  * the model reports, at the rank the row was built around, the branches the row is named for; every row's bins change under each variant it
    names; every variant is named by a row -- except `window_clean_ignores_pending`, which cannot change a bin (hist_model's docstring has the
    argument) and is shown equal to the rule on every small input tried here, with a window of four bins so that windows abound;
  * coverage, asserted: every entry of the branch report, a run that skips 99 bins, both values of the shortcut flag in every producer's rows,
    every window kind and both values of both crossing flags in the rows of (e), a tier and a hist_path for every variable of (c).

Not built: an input, sorted beforehand, that forces the reference's quickselect onto its heapsort branch at the top of the recursion, on which
`sorted_rule` would have to equal the literal oracle.  The branch needs 1 + log2(n + 1) bad pivots in a row from choose_pivot's median of
medians on data that is already in order, and behind a partial quickselect the two rules are mixed; tests/test_gpu_strict_hist.py and
tests/golden/hist_fallback.npz cover that branch on recorded inputs.  `sorted_rule` is tied to apply_sorted by the reference's own known
answers for it instead (test_histogram_sorted_simple, below)."""
import collections

import numpy as np
import pytest

import hist_edges_util as E
import hist_model as M
import latent_window_util as W
import oracle_lib as O

SECTIONS = "abcdef"


def test_bin_idx_and_c_count_known_answers():
    n, bl = 41, 2
    assert [M.bin_idx(c, n, bl) for c in (0, 10, 11, 30, 31, 40)] == [0, 0, 1, 2, 3, 3]
    assert M.c_count(0, n, bl) == 11 and M.c_count(3, n, bl) == 41


def test_histogram_quicksort_known_answers():
    for lat, bl, bins in M.known_answers():
        for seed in range(16):
            x = np.random.default_rng(seed).permutation(np.array(lat, np.uint32))
            assert M.histogram(x, bl)[0] == bins, (lat[:4], bl, seed)
            assert O.histogram(x, bl, rule=0) == (bins, False) and O.histogram(x, bl, rule=1) == (bins, False)


def test_sorted_rule_is_apply_sorted_on_the_references_known_answers():
    """histograms.rs test_histogram_sorted_simple: apply_sorted on whole inputs."""
    kats = [([8], 0, [(1, 8, 8)]), (list(range(1, 10)), 2, [(3, 1, 3), (2, 4, 5), (2, 6, 7), (2, 8, 9)]), ([8] * 11, 2, [(11, 8, 8)]),
            ([0, 0, 0, 1, 2, 2, 2, 2], 3, [(3, 0, 0), (1, 1, 1), (4, 2, 2)]), ([0, 0, 1, 2, 2, 2, 2, 2], 3, [(2, 0, 0), (1, 1, 1), (5, 2, 2)])]
    for lat, bl, bins in kats:
        assert M.histogram(lat, bl, ("sorted_rule",))[0] == bins, (lat, bl)
    # the slip the rule guards against: 60 % one value at 16 bins of 255 -- apply_sorted splits a bin the quickselect keeps whole
    x = np.random.default_rng(1).permutation(np.concatenate([np.full(153, 7), np.arange(1000, 1102)])).astype(np.uint32)
    assert M.histogram(x, 4)[0] == O.histogram(x, 4, rule=0)[0] != M.histogram(x, 4, ("sorted_rule",))[0]


def test_row_names_are_unique_and_every_row_says_what_it_stands_on():
    rows = E.all_rows()
    assert len(E.BY_NAME()) == len(rows) and all(r.about and r.name.startswith(r.section + "-") for r in rows)
    assert all(r.arr.size <= 1 << 16 for r in rows)
    assert {r.section for r in rows} == set(SECTIONS)


@pytest.mark.parametrize("section", list(SECTIONS))
def test_model_equals_both_oracle_rules_and_no_row_takes_the_heapsort_branch(section):
    rows = [r for r in E.all_rows() if r.section == section]
    assert rows
    bad = []
    for r in rows:
        vs, _ = E.variables(r.name)
        assert {v.var for v in vs} == ({1} | ({0} if r.kw.get("delta") == 3 else set()) | ({2} if r.kw["mode"] != 1 else set()))
        for v in vs:
            bins, rep = E.model_of(r.name, v.var)
            for rule in (1, 0):
                got, fb = O.histogram(v.latents, v.bins_log, rule=rule)
                if fb or got != bins:
                    bad.append((r.name, v.var, rule, fb))
            assert sum(b[0] for b in bins) == v.latents.size and len(bins) <= 1 << v.bins_log
        if r.paging != "exact":      # (the oracle's plan of the chunk as the config pages it; an Exact row's latents went through O.histogram above)
            _, _, fb = O.chunk_plan(r.arr, O.make_config(enable_8_bit=True, **r.kw))
            if fb:
                bad.append((r.name, "chunk_plan"))
    assert not bad, bad[:8]


def test_every_row_shows_the_branches_it_is_named_for():
    bad = []
    for r in E.all_rows():
        _, rep = E.model_of(r.name, r.var)
        for st, names in r.needs.items():
            step = rep.step_of(st)
            if step is None or not set(names) <= set(step[0]):
                bad.append((r.name, st, names, step))
    assert not bad, bad[:6]


def test_every_row_changes_under_each_variant_it_names_and_every_variant_is_named():
    named = collections.Counter(); bad = []
    for r in E.all_rows():
        v = next(x for x in E.variables(r.name)[0] if x.var == r.var)
        bins, _ = E.model_of(r.name, r.var)
        for variant in r.variants:
            named[variant] += 1
            if M.histogram(v.latents, v.bins_log, (variant,))[0] == bins:
                bad.append((r.name, variant))
    assert not bad, bad[:8]
    assert set(named) == set(M.VARIANTS) - set(M.EQUIVALENT_VARIANTS), sorted(set(M.VARIANTS) - set(named))
    print(dict(named))


def test_dropping_pending_from_the_windows_clean_changes_no_bin():
    """`window_clean_ignores_pending` against the rule on 2000 small inputs with windows of four bins, and on every row of (e): a bin is never
    pending where the walk stands on a window's first rank, so the position check alone refuses those windows.  Its other half does matter."""
    rng = np.random.default_rng(5); crossed = 0; differs = 0
    for it in range(2000):
        n = int(rng.integers(1, 400)); bl = int(rng.integers(3, 8))
        x = rng.integers(0, max(2, n // (1 + it % 6)), n)
        bins, rep = M.histogram(x, bl, window=4)
        assert bins == M.histogram(x, bl)[0] == M.histogram(x, bl, ("window_clean_ignores_pending",), window=4)[0]
        crossed += sum(w.pending_crossed for w in rep.windows)
        differs += bins != M.histogram(x, bl, ("window_clean_ignores_pos",), window=4)[0]
    assert crossed > 100 and differs > 100, (crossed, differs)
    for r in E.rows_e():
        v = E.variables(r.name)[0][0]
        assert M.histogram(v.latents, v.bins_log, ("window_clean_ignores_pending",))[0] == E.model_of(r.name, 1)[0]


def test_coverage_of_branches_shortcut_windows_and_producers():
    hits = collections.Counter(); skipped = 0
    shortcut = collections.defaultdict(set)
    for r in E.all_rows():
        for v in E.variables(r.name)[0]:
            _, rep = E.model_of(r.name, v.var)
            hits.update(rep.counts); skipped = max(skipped, rep.max_skipped)
            shortcut[E.producer_of(r, v)].add(rep.shortcut)
    assert all(hits[name] > 0 for name in M.REPORT), {name: hits[name] for name in M.REPORT}
    assert skipped >= 99, skipped
    assert set(shortcut) == set(W.TIERS) | {"big", "literal", "sort-fallback"}, sorted(shortcut)
    assert all(shortcut[p] == {True, False} for p in W.TIERS + ("big", "literal")), dict(shortcut)
    kinds = collections.Counter(); flags = set()
    for r in E.rows_e():
        _, rep = E.model_of(r.name, 1)
        assert len(rep.windows) == (1 << E.variables(r.name)[0][0].bins_log) // M.WINDOW
        kinds.update(w.kind for w in rep.windows)
        flags |= {("pending", w.pending_crossed) for w in rep.windows} | {("run", w.run_crossed) for w in rep.windows}
        seq = "".join(w.kind[0] for w in rep.windows)
        flags |= {s for s in ("sw", "ws") if s in seq}
    assert all(kinds[k] > 0 for k in M.WINDOW_KINDS), kinds
    assert flags == {("pending", True), ("pending", False), ("run", True), ("run", False), "sw", "ws"}, flags
    print(dict(hits), skipped, dict(kinds))


def test_every_row_of_c_has_its_tier_and_hist_path():
    seen = set()
    for r in E.rows_c():
        vs, route = E.variables(r.name)
        for v in vs:
            assert v.tier in W.TIERS and v.hist_path in (0, 1, 2) and v.latents.size == (r.arr.size - (1 if r.kw.get("delta") == 3 else 0) if v.var != 2 else r.arr.size)
        designed = next(v for v in vs if v.var == r.var)
        tier = r.name.split("-")[1]
        if tier in W.TIERS:
            assert designed.tier == tier, (r.name, designed.tier)
            assert (route == "c16") == (tier != "select" and "full-width" not in r.name), (r.name, route)
        seen.add((designed.tier, designed.hist_path, route == "c16"))
        assert (designed.hist_path == 2) == r.gives_up
    assert {t for t, _, _ in seen} == set(W.TIERS)
    assert ("wide", 0, True) in seen and ("wide", 0, False) in seen and ("select", 2, False) in seen and ("small", 0, True) in seen
    lb = E.variables("c-lookback-int64-n4608-period365")[0]
    assert [v.var for v in lb] == [0, 1] and not E.model_of("c-lookback-int64-n4608-period365", 0)[1].shortcut
    im = [r for r in E.rows_c() if "imult" in r.name]
    assert im and all(E.variables(r.name)[0][1].bins_log == 6 and E.variables(r.name)[0][1].var == 2 for r in im)
