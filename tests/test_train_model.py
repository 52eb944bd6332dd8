"""-m "not gpu": the plain model of the training step (tests/train_model.py) against the oracle, and the cases of
tests/train_edges_util.py pinned before the device is judged by them.

  * the model equals the oracle -- log2_approx exhaustively over 1 .. 2^16 and around every power of two, optimize_bins and
    quantize_weights on every case's histogram and on a seeded sweep of random bin lists of 1 .. 4096 bins, the whole plan through
    chunk_plan on every case;
  * every case reaches its edge: the model's report shows the tied candidates at the stated steps (or the shortcut, the repair-loop
    counts, the reduction, worst - baseline), and the case's VARIANT of the model gives other bins or weights -- a case that does not
    discriminate fails here, it is not kept;
  * the tie cases, built from powers of two, give the same partition and the same tied candidates in exact integer arithmetic;
  * every case's array realises its bin list under the reference's literal histogram and under the multiset rule, without the
    order-dependent heapsort branch (the device follows the multiset rule; the GPU module skips nothing);
  * known answers through the chunk path: unoptimized_bins_log at the sizes where the kernel changes, and the fallback decision."""
import numpy as np
import pytest

import gpu_util as U
import oracle_lib as O
import train_edges_util as E
import train_model as M

f32 = np.float32


def test_log2_approx_equals_the_oracle_bit_for_bit():
    xs = [f32(i) for i in range(1, (1 << 16) + 1)]
    for e in range(32):
        p = f32(2.0 ** e)
        xs += [np.nextafter(p, f32(0)), p, np.nextafter(p, f32(np.inf))]
    xs = np.array(xs, f32)
    want = np.array([O.lib().pco_oracle_log2_approx(float(x)) for x in xs], f32)
    assert np.array_equal(M.log2_approx(xs).view(np.uint32), want.view(np.uint32))
    for e in range(32):                      # what makes the ties exact
        assert M.log2_approx(f32(2.0 ** e)) == f32(e)
    assert all(float(v) * (1 << M.SCALE_LOG) % 1 == 0 for v in M.log2_approx(xs[1:1 << 16]))


def random_bins(rng, nb, bits, kind):
    top = 1 << min(bits, 48)
    pts = np.sort(rng.choice(top, 2 * nb, replace=False)) if top > 4 * nb else None
    if pts is None:
        return None
    if kind == "flat": counts = rng.integers(1, 60, nb)
    elif kind == "geometric": counts = np.maximum(1, (4000 * 0.97 ** np.arange(nb)).astype(np.int64))[rng.permutation(nb)]
    else: counts = np.where(np.arange(nb) == nb // 2, 200000, rng.integers(1, 30, nb))
    trivial = rng.random(nb) < 0.3
    return [(int(c), int(pts[2 * i]), int(pts[2 * i] if trivial[i] else pts[2 * i + 1])) for i, c in enumerate(counts)]


@pytest.mark.parametrize("kind", ["flat", "geometric", "one-dominant"])
def test_model_equals_the_oracle_on_random_bin_lists(kind):
    rng = np.random.default_rng(len(kind))
    seen = 0
    for nb in (1, 2, 3, 7, 63, 64, 65, 255, 256, 257, 700, 1024, 2500, 4095, 4096):
        for bits in E.WIDTHS:
            bins = random_bins(rng, nb, bits, kind)
            if bins is None: continue
            for asl in (0, 10, 12):
                if nb > 256 and asl != 12: continue
                got, rep = M.optimize_bins(bins, bits, asl)
                assert got == [tuple(b) for b in O.optimize_bins(bins, bits, asl)], (kind, nb, bits, asl, rep.shortcut)
            counts = [b[0] for b in got]
            for size_log in (4, 10, 12):
                sl, w, _ = M.quantize_weights(counts, sum(counts), size_log)
                assert (sl, w) == O.quantize_weights(counts, sum(counts), size_log), (kind, nb, bits, size_log)
            sl = max(size_log, (len(counts) - 1).bit_length())
            assert M.quantize_weights_to(counts, sum(counts), sl)[0] == O.quantize_weights_to(counts, sum(counts), sl)
            seen += 1
    assert seen >= 50


def test_the_reference_known_answers_and_the_dominant_bin_beside_255_singletons():
    assert M.quantize_weights_to([777], 777, 0)[0] == [1]
    assert M.quantize_weights_to([777, 1], 778, 2)[0] == [3, 1]
    assert M.quantize_weights_to([2, 3, 6, 5, 1], 17, 3)[0] == [1, 1, 3, 2, 1]
    assert M.quantize_weights([77, 100], 177, 4)[:2] == (4, [7, 9])
    assert M.quantize_weights([77, 77], 154, 4)[:2] == (1, [1, 1])
    # 255 bins that want less than one weight each beside one that wants the rest: 1 ... 1, 769 at size 10 (no chunk reaches this:
    # train_edges_util.cases_f).  Without the cut at zero the small bins' surplus is negative.
    counts = [1] * 255 + [100000]
    got = M.quantize_weights(counts, sum(counts), 10)
    assert got[:2] == (10, [1] * 255 + [769]) == O.quantize_weights(counts, sum(counts), 10)
    assert M.quantize_weights(counts, sum(counts), 10, {"no_surplus_floor"})[:2] != got[:2]


@pytest.mark.parametrize("section", list(E.SECTIONS))
def test_every_case_reaches_its_edge_and_discriminates(section):
    cases = [c for c in E.section(section)]
    assert cases and all(c is not None for c in cases) or section == "b", "a case no count per value realises"
    for c in cases:
        if c is None: continue
        plans, fb, worst, baseline, ubl = E.model_plans(c)
        bad = E.check_edge(c, plans[c.var], worst, baseline)
        assert bad is None, (c.name, c.edge, bad)
        assert E.predicted_chunk(c, E.variant_set(c)) != E.predicted_chunk(c), (c.name, c.variant, "the case does not discriminate")
        assert fb == (c.section == "h" and c.edge["fallback"] > 0), (c.name, worst, baseline)
        assert (ubl > 8) == (c.section in "cd" or c.kw["level"] == 12 and E.numbers(c.name).size >= 1024), (c.name, ubl)


def test_the_cases_that_do_not_fit_are_the_ones_known_not_to():
    """At 16 bits a bin's metadata (31 bits) costs less than isolating one value of the sparse prefix saves (32): the prefix falls apart
    and the 192-run's tie in slots 0/1 does not exist.  At 8 bits the type has room for the 21-triple case and the runs only."""
    missing = [i for i, c in enumerate(E.section("b")) if c is None]
    assert len(missing) == 1 and sum(c is None for s in E.SECTIONS for c in E.section(s)) == 1
    names = set(E.BY_NAME())
    assert {f"b-w{b}-run192-sparse-slots01" for b in (32, 64)} <= names and "b-w16-run192-sparse-slots01" not in names
    assert len(names) == len(E.all_cases())
    # every slot boundary of the one-wave kernel, every wave pairing of the block kernel
    steps = {(c.section, i, tuple(js)) for c in E.all_cases() if "ties" in c.edge for i, js in c.edge["ties"].items()}
    for sec, pair in (("a", (63, 64)), ("a", (127, 128)), ("a", (191, 192)), ("a", (254, 255)), ("b", (32, 96)), ("b", (64, 128)), ("b", (128, 192)),
                      ("b", (1, 128)), ("b", (63, 190)), ("c", (1, 128)), ("c", (64, 128)), ("c", (1, 1024)), ("c", (1001, 2024)), ("c", (1024, 1025))):
        assert any(s == sec and js == pair for s, _, js in steps), (sec, pair)
    assert {len(c.bins) for c in E.section("c")} >= {257, 1023, 1024, 1025, 4095, 4096}
    assert {c.bits for c in E.section("e")} == {c.bits for c in E.section("f")} == {16, 32, 64}
    used = set().union(*(E.variant_set(c) for c in E.all_cases())) | {"no_surplus_floor"}
    assert used == set(M.VARIANTS), set(M.VARIANTS) - used            # no variant is listed that no case must change under
    assert {c.bits for c in E.section("a")} == set(E.WIDTHS) and max(E.numbers(c.name).size for c in E.all_cases()) == 1 << 18


@pytest.mark.parametrize("section", ["a", "b", "c", "d", "g"])
def test_tie_cases_agree_with_exact_integer_arithmetic(section):
    for c in E.section(section):
        if c is None or "ties" not in c.edge: continue      # (the lookback cases hold strays of other counts: their tie is f32's, checked above)
        if len(c.bins) > 1100 and c.bits != 32: continue
        ubl = M.choose_unoptimized_bins_log(c.kw["level"], E.numbers(c.name).size)
        n_lat = sum(b[0] for b in c.bins)
        a, b = M.train(c.bins, c.bits, ubl, n_lat), M.train(c.bins, c.bits, ubl, n_lat, exact=True)
        assert a[:6] == b[:6] and a.dp.partitioning == b.dp.partitioning and a.dp.shortcut == b.dp.shortcut, c.name
        assert all(a.dp.ties[i] == b.dp.ties[i] == js for i, js in c.edge["ties"].items()), c.name
        assert float(a.dp.best_cost) == b.dp.best_cost / (1 << M.SCALE_LOG), c.name   # an integer: nothing was rounded on the winning path


@pytest.mark.parametrize("section", list(E.SECTIONS))
def test_arrays_realise_their_bin_lists_and_the_model_equals_the_oracle_through_the_chunk(section):
    for c in E.section(section):
        if c is None: continue
        x = E.numbers(c.name)
        plans, fb, worst, baseline, ubl = E.model_plans(c)
        for key, lat in E.case_latents(c).items():
            bl = M.var_bins_log(ubl, key)
            h0, fb0 = O.histogram(lat, bl, rule=0)
            h1, fb1 = O.histogram(lat, bl, rule=1)
            assert h0 == h1 and not fb0 and not fb1, (c.name, key, "the heapsort branch: change the seed")
            if key == c.var and c.bins is not None:
                assert h1 == c.bins, (c.name, len(h1), len(c.bins))
            # the oracle's own stages on the case's histogram
            est = M.estimated_ans_size_log(bl, lat.size)
            got, _ = M.optimize_bins(h1, c.bits, est)
            assert got == [tuple(b) for b in O.optimize_bins(h1, c.bits, est)], (c.name, key)
        cfg = O.make_config(**c.kw)
        info, bins, hist_fell_back = O.chunk_plan(x, cfg)
        assert not hist_fell_back and E.shown_chunk(info, bins) == E.predicted_chunk(c), c.name
        f = O.simple_compress(x, cfg)
        assert U.bits_equal(O.simple_decompress(f, x.dtype, cap=x.size + 8), x), c.name
        info2, bins2 = O.inspect_first_chunk(f)
        assert E.shown_chunk(info2, bins2) == E.predicted_chunk(c), c.name


def test_lookback_cases_have_a_delta_variable_of_32_bits_with_the_triples_in_it():
    """The lookbacks steered by the plain model of the search are the oracle's; the chunk keeps its lookback delta, with the window and the
    one-latent state the model of should_fallback assumes; every triple's values hold exactly 64 lookbacks."""
    import lookback_model as LM
    cases = [c for c in E.section("g") if c.var == "delta"]
    assert {(c.bits, c.kw["level"]) for c in cases} == {(b, l) for b in (16, 32, 64) for l in (8, 12)}
    for c in cases:
        x = E.numbers(c.name)
        lbs = E.case_latents(c)["delta"]
        assert lbs.dtype == np.uint32 and np.array_equal(lbs, O.choose_lookbacks(x, LM.window_log(x.size))), c.name
        assert all(int((lbs == v + d).sum()) == E.LOOKBACK_COUNT for v in E.LOOKBACK_TRIPLES for d in range(3)) and lbs.size == 2048
        info, bins, _ = O.chunk_plan(x, O.make_config(**c.kw))
        assert info.var_present[0] and info.delta_kind == E.DELTA_SHOWN[E.DELTA_LOOKBACK], c.name
        assert (info.window_n_log, info.state_n_log) == (LM.window_log(x.size), 0), c.name


def test_fallback_sweep_finds_all_three_differences_next_to_each_other():
    s = E.fallback_sweep()
    assert s[-1] and s[0] and s[1], {k: len(v) for k, v in s.items()}        # none of -1, 0, +1 is missing
    assert s[-1][-1] + 1 == s[0][0] and s[0][-1] + 1 == s[1][0]
    for c in E.section("h"):
        info, bins, _ = O.chunk_plan(E.numbers(c.name), O.make_config(**c.kw))
        fell_back = info.delta_kind == 0 and info.n_bins[1] == 1 and int(bins[1][0][2]) == 16
        assert fell_back == (c.edge["fallback"] > 0), c.name


@pytest.mark.parametrize("level,n,want", [(9, (1 << 12) - 1, 8), (9, 1 << 12, 8), (9, (1 << 13) - 1, 8), (9, 1 << 13, 9), (12, (1 << 16) - 1, 11), (12, 1 << 16, 12),
                                          (8, (1 << 12) - 1, 7), (8, 1 << 12, 8), (10, 1 << 12, 9), (12, 511, 8), (12, 1023, 8), (12, 1024, 9)])
def test_unoptimized_bins_log_where_the_kernel_changes(level, n, want):
    """The value by the reference's arithmetic, and through the chunk path: the bins of `n` normally distributed numbers follow the
    histogram's resolution -- the model, fed the oracle's histogram at 2^want bins, must predict chunk_plan, and fed the one at half as many
    must not."""
    assert M.choose_unoptimized_bins_log(level, n) == want
    rng = np.random.default_rng(n)
    x = (np.int64(1 << 31) + np.round(rng.normal(0.0, 1.0, n) * (1 << 24)).astype(np.int64)).astype(np.uint32)
    lat_hist, _ = O.histogram(x, want, rule=1)
    other, _ = O.histogram(x, want - 1, rule=1)
    p = M.train(lat_hist, 32, want, n)
    info, bins, _ = O.chunk_plan(x, O.make_config(level=level, mode=1, delta=1))
    shown = E.shown_chunk(info, bins)[2][1]
    assert shown == (p.ans_size_log, list(zip(p.weights, p.lowers, p.offset_bits)))
    q = M.train(other, 32, want - 1, n)
    assert shown != (q.ans_size_log, list(zip(q.weights, q.lowers, q.offset_bits))), "the sizes do not tell the two bins_log apart"
