"""-m "not gpu": the model of enc_walkseg_kernel's schedule (walkseg_model.py) against the oracle, and the rows of walkseg_edges_util.py against
what they claim.

  * the constants the model reads from the sources, and their relations;
  * every row: the oracle trains the table the row assumes, does not take its heapsort branch and round-trips; the model's true walk arrives at
    the page's four final states with the batches' tANS bit totals of the oracle's chunk; the kernel's schedule gives the true walk;
  * every two-valued row: the model's event record equals what the rule of the two-valued tables says (walkseg_edges_util.expected_events);
  * every row reveals the mutants it names; every mutant that changes a value the page shows is revealed by at least five rows;
  * every axis is covered: segments in use, chains, fix_n classes, symbol sources, levels;
  * the model's arc beside all T trajectories on the rows with tables of up to 2^6 states (the brute force of test_walk_segments_model.py,
    on the rows' own symbols).

Mutant (g), `nbs` not made odd, is the one the page cannot show: the schedule is exact for ANY cut into segments (the odd share spreads the
walkers' LDS traffic, it decides no value), so its words, totals and final states equal the true ones on every row.  That is asserted as
such; what changes is the event record (other segments), and at least five rows show that."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import walkseg_edges_util as E
import walkseg_model as M

ROWS = E.ROWS()
VALUE_MUTANTS = tuple(m for m in M.MUTANTS if m != "g")


def test_constants_and_their_relations():
    assert (M.kWsSegs, M.kWsMinBatches, M.kWsMaxItems, M.kWsSkew, M.kWsSymBase, M.kBatchN, M.kDirectHistRange, M.kFastEncMaxAsl) == (16, 64, 4096, 1, 4096, 256, 4096, 10)
    assert M.kWsSegs * 4 == 64                                     # one quad of the walker wave per segment
    assert M.info_off(M.kFastEncMaxAsl) + 8 * 256 == M.kWsSymBase  # the largest table and 256 info words end where the symbol buffers begin
    assert M.vt_off(10, 2) + 2027 + 1 == M.kWsSymBase
    for n_lat in list(range(M.kWsMinBatches * M.kBatchN, 120 * M.kBatchN, 97)) + [1 << 18, (1 << 18) + 1, 1 << 24]:
        g = M.geometry(n_lat)
        assert g.nbs % 2 == 1 and 1 <= g.n_seg <= M.kWsSegs and (g.n_seg - 1) * g.nbs < g.nb <= g.n_seg * g.nbs
    assert [M.geometry(nb * 256)[1:3] for nb in (64, 65, 79, 80, 81, 112, 113, 1024)] == [(5, 13), (5, 13), (5, 16), (5, 16), (7, 12), (7, 16), (9, 13), (65, 16)]
    assert M.source(True, 2027, 10, 2) == "all_lds" and M.source(True, 2028, 10, 2) == "finds" and M.source(True, 4096, 10, 2) == "stages" and M.source(False, 72, 10, 2) == "stages"


def test_the_row_set():
    by_cls = {c: sum(r.cls == c for r in ROWS) for c in "GTMRASOVB"}
    assert by_cls == {"G": 10, "T": 7, "M": 37, "R": 10, "A": 12, "S": 16, "O": 3, "V": 4, "B": 2}, by_cls
    assert all(M.kWsMinBatches * M.kBatchN <= r.n_lat <= (1 << 18) + 1 for r in ROWS)
    assert sum(r.n_lat > 1 << 17 for r in ROWS) <= 8              # a few rows of 2^18 latents, the rest 64 .. 113 batches (the reset rows: 257)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_row_against_the_oracle_and_its_claim(name):
    r = E.BY_NAME()[name]
    assert not E.took_heapsort(name), "the reference's heapsort branch: the device would not be compared on this row"
    a = E.numbers(name)
    f = O.simple_compress(a, O.make_config(**r.kw))                # (refused by the oracle: an exception here)
    back = O.simple_decompress(f, a.dtype, a.size)
    assert back.tobytes() == a.tobytes(), "the oracle does not round-trip the row"
    W, d = E.walks(name)
    want_vars = dict(r.claims).get("vars", (1,))
    assert tuple(sorted(W)) == tuple(want_vars), (sorted(W), d.layout.asl, [len(b) for b in d.layout.bins])
    if r.weights is not None:
        assert tuple(sorted(b[0] for b in d.layout.bins[1])) == r.weights, "the oracle trained another table than the row assumes"
    assert d.layout.asl[1] == r.kw["level"] + 2
    revealed = set()
    for v, w in W.items():
        assert not M.pinned_to_oracle(w, d, v), M.pinned_to_oracle(w, d, v)
        o = w.run(None); tw, tf, tb = w.true()
        assert np.array_equal(o.words, tw) and o.finals == tf and np.array_equal(o.bat, tb) and not o.error, f"variable {v}: the schedule does not give the true walk"
        assert all(s.resets_after == 0 for s in o.segs)            # (a met chain stays met: no reset behind a meeting)
        g = w.run("g")
        assert np.array_equal(g.words, tw) and g.finals == tf and np.array_equal(g.bat, tb) and not g.error, "an even share of batches changed a value"
        revealed |= {m for m in VALUE_MUTANTS if w.reveals(m)}
    assert set(r.reveals) <= revealed, f"claims {sorted(set(r.reveals) - revealed)}, reveals {sorted(revealed)}"
    o = W[1].run(None)
    if r.positions is not None and len(r.weights) == 2:
        ex = E.expected_events(r.n_lat, r.positions)
        assert (o.geom.nb, o.geom.nbs, o.geom.n_seg) == ex.geom
        assert [s.fix_n for s in o.segs] == ex.fix and [s.whole_open for s in o.segs] == ex.whole and [s.met_in_last for s in o.segs] == ex.met_in_last
        assert [s.last_chain for s in o.segs] == ex.last_chain and [s.round for s in o.segs] == ex.round and o.rounds == ex.rounds
        assert [s.met for s in o.segs] == ex.met
    for key, val in r.claims:
        if key == "geom": assert (o.geom.nb, o.geom.nbs, o.geom.n_seg) == val
        elif key == "fix": assert o.segs[val[0]].fix_n == val[1], (val, o.segs[val[0]])
        elif key == "last": assert o.segs[val[0]].last_chain == val[1], (val, o.segs[val[0]])
        elif key == "unmet": assert not o.segs[val].met and o.segs[val].whole_open
        elif key == "rounds": assert o.rounds == val, o.rounds
        elif key == "top_latents": assert o.geom.segs[-1][1] == val and o.segs[-1].fix_n == 0
        elif key == "resets":
            assert any(s.resets_before >= val and s.met and 1 < s.fix_n < s.my_nb for s in o.segs), "no segment with that many resets before a meeting in mid-segment"
            assert any(not s.met for s in o.segs), "no segment that never meets"
        elif key == "bins": assert len(d.layout.bins[1]) == val
        elif key != "vars": raise KeyError(key)
    if r.source is not None:
        assert E.source_of(name) == r.source


def test_every_value_mutant_is_revealed_by_five_rows_or_more():
    counts = {m: [r.name for r in ROWS if any(w.reveals(m) for w in E.walks(r.name)[0].values())] for m in VALUE_MUTANTS}
    print({m: len(v) for m, v in counts.items()})
    assert all(len(v) >= 5 for v in counts.values()), {m: len(v) for m, v in counts.items()}
    claimed = {m: sum(m in r.reveals for r in ROWS) for m in VALUE_MUTANTS}
    assert all(v >= 5 for v in claimed.values()), claimed
    # (g) moves the segments and nothing else
    moved = [r.name for r in ROWS if E.walks(r.name)[0][1].run("g").geom != E.walks(r.name)[0][1].run(None).geom]
    assert len(moved) >= 5, moved


def test_the_model_says_what_the_device_did_under_every_mutant():
    """tests/golden/walkseg_mutants_on_device.json: per mutant (each applied once to encode_walkseg.hip in a build that was never committed) the
    rows whose chunk an MI355X did not write as the oracle does.  The model must name exactly those rows, mutant by mutant."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walkseg_mutants_on_device.json")) as f:
        rec = json.load(f)
    known = [n for n in rec["rows"] if n in E.BY_NAME()]
    assert len(known) >= 90
    for m in M.MUTANTS:
        model = sorted(n for n in known if any(w.reveals(m) for w in E.walks(n)[0].values()))
        assert model == sorted(n for n in rec["failed"][m] if n in E.BY_NAME()), m


def test_every_axis_is_covered():
    seen_seg, last_chains, fix_cls, sources, levels = set(), set(), set(), set(), set()
    for r in ROWS:
        o = E.walks(r.name)[0][1].run(None)
        seen_seg.add(o.geom.n_seg); levels.add(r.kw["level"])
        for s in o.segs[:-1]:
            if s.last_chain is not None and s.fix_n > 1: last_chains.add(s.last_chain)
            fix_cls.add("1" if s.fix_n == 1 else "all-unmet" if s.whole_open and not s.met else "all-met" if s.met_in_last else "all-1" if s.fix_n == s.my_nb - 1 else "mid")
        if r.source and r.cls == "S": sources.add(E.source_of(r.name))
    assert seen_seg >= {12, 13, 14, 15, 16}, seen_seg
    assert last_chains == {0, 1, 2, 3}
    assert fix_cls == {"1", "mid", "all-1", "all-met", "all-unmet"}, fix_cls
    assert sources == {"finds", "all_lds", "stages"}
    assert levels == {8, 6, 4, 2}


@pytest.mark.parametrize("name", [r.name for r in ROWS if r.kw["level"] <= 4])
def test_the_arc_beside_every_trajectory(name):
    """On the rows' own symbols and tables of 2^4 and 2^6 states: the model's first pass of a lane against brute force over all T starts -- the
    same meeting step (or none) and the same number of resets -- for three segments of the row (one, for the rows of 2^18 latents)."""
    w = E.walks(name)[0][1]; g = M.geometry(w.n)
    qs = [3] if w.n > 1 << 17 else sorted({0, min(7, g.n_seg - 2), g.n_seg - 2})
    for q in qs:
        lo, nl, nbq = g.segs[q]
        for j in range(4):
            A, Bs, res, _, meet, _ = w._pass1(lo, nl, j, 0, w.tab.T - 1, True)
            last = nl - 1 - ((nl - 1 - j) % 4)
            syms = [w.S[i] for i in range(lo + last, lo + j - 1, -4)]
            k, resets = M.brute_arc_check(w.tab, syms)
            assert (None if k is None else lo + last - 4 * k) == meet, (q, j, k, meet)
            assert resets == sum(res) and (A[-1] == Bs[-1]) == (k is not None)
