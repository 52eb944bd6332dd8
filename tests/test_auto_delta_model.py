"""-m "not gpu": the plain model of DeltaSpec::Auto (auto_delta_model.py) and the row table (auto_delta_edges_util.py) that
test_gpu_auto_delta_edges.py runs on the device, pinned on the CPU.

For every row: the oracle's nine estimates and decision (oracle_lib.auto_delta_costs: every candidate evaluated, choose_auto_delta_encoding
untouched) satisfy the row's claim, so the row sits on the edge it is named after; the model's sample length and its replay of the decision
from those estimates equal the oracle's.  The model's sample positions are held against the oracle's by probing: a number changed at a
position changes the oracle's estimates exactly when the model says the position is sampled, on both sides of every group boundary.  A few
hundred random chunks pin the replay beyond the table.  The batch replay over wave sub-lists (what the device does) equals the sequential
decision chunk by chunk.  And every wrong reading of VARIANTS changes what is predicted for each row that names it, so a row that would
let the misreading through cannot stay in the table unnoticed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import auto_delta_edges_util as E
import auto_delta_model as M
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [r.name for r in E.rows()]


@pytest.mark.parametrize("name", NAMES)
def test_row_sits_on_its_edge_and_the_model_decides_as_the_oracle(name):
    r = E.by_name()[name]
    sn, costs, dec = E.oracle(name)
    assert sn == M.sample_n(r.arr.size), name
    assert r.claim(sn, costs, dec), (name, r.edge, sn, None if costs is None else costs.tolist(), dec)
    if sn == 0:
        assert dec == (M.NONE, 0, 0) and M.decide(None, r.arr.size) == dec and M.schedule(None, r.arr.size) == 0
        return
    assert costs.dtype == np.float32 and (costs == np.floor(costs)).all() and (costs > 0).all()       # whole bytes
    assert M.decide(costs, r.arr.size) == dec, (name, costs.tolist())
    # the decision in the oracle's own chunk: what the encoder writes (the fallback to a plain chunk aside, which keeps no delta)
    info, _, _ = O.chunk_plan(r.arr, O.make_config(max_page_n=1 << 20, **r.kw))
    assert (info.delta_kind, info.delta_order, info.window_n_log) in (dec, (M.NONE, 0, 0)), name


def probe(arr, kw, pos):
    """whether the oracle's estimates change when the number at `pos` does"""
    b = arr.copy(); b[pos] = b[pos] ^ np.array(0x5A5A5A5A, dtype=np.uint32).astype(b.dtype)
    return not np.array_equal(O.auto_delta_costs(arr, O.make_config(**kw))[1], O.auto_delta_costs(b, O.make_config(**kw))[1])


@pytest.mark.parametrize("n", [10, 11, 199, 200, 201, 7649, 7650, 7651, 15649, 15650, 15651, 1 << 20])
def test_sample_positions_are_the_oracles_by_probing(n):
    """a smooth chunk; one number replaced by something far away just outside and just inside each end of each group (of the first two and the
    last group for the 132 groups of 2^20)"""
    pos = M.sample_positions(n)
    sampled = set(pos.tolist())
    assert len(pos) == M.sample_n(n) == len(sampled)
    arr = (1000 + 7 * np.arange(n, dtype=np.uint64)).astype(np.uint32)
    g = pos.reshape(-1, min(n, 200)); k = len(g)
    assert k == {10: 1, 11: 1, 199: 1, 200: 1, 201: 1, 7649: 1, 7650: 2, 7651: 2, 15649: 2, 15650: 3, 15651: 3, 1 << 20: 132}[n]
    if n in (7650, 15650): assert pos[-1] == n - 1                             # the last group ends exactly at the last number
    if n == 15651: assert pos[-1] == n - 2 and g[1][0] == 7725                 # the stride's division truncates: one number stays behind the third group
    for grp in [g[i] for i in sorted({0, min(1, k - 1), k - 1})]:
        for p in (int(grp[0]) - 1, int(grp[0]), int(grp[-1]), int(grp[-1]) + 1):
            if 0 <= p < n: assert probe(arr, E.DEFAULT, p) == (p in sampled), (n, p)


def random_chunk(seed):
    rng = np.random.default_rng(seed)
    dt = [np.uint8, np.uint16, np.uint32, np.uint64, np.int32, np.int64][seed % 6]
    n = int(rng.choice([rng.integers(1, 30), rng.integers(30, 600), rng.integers(600, 9000)]))
    kind = seed % 4
    if kind == 0: a = E.cums(rng.integers(0, int(rng.choice([2, 3, 16, 256])), n), int(rng.integers(0, 9)), np.uint64)
    elif kind == 1: period = int(rng.integers(2, 40)); a = rng.integers(0, 1 << 16, period)[np.arange(n) % period] + rng.integers(0, 4, n)
    elif kind == 2: a = rng.integers(0, 1 << 62, n)
    else: a = E.cums(E.quad_ramp(n, 0x9E3779B1, 1 << int(rng.integers(8, 32))), int(rng.integers(0, 6)), np.uint64)
    return np.asarray(a).astype(np.uint64).astype(dt), int(rng.choice([0, 4, 8, 12]))


def test_the_replay_equals_the_oracle_on_random_chunks():
    stops = set()
    for seed in range(400):
        a, level = random_chunk(seed)
        sn, costs, dec = O.auto_delta_costs(a, O.make_config(level=level))
        assert sn == M.sample_n(a.size) and M.decide(costs, a.size) == dec, (seed, a.dtype, a.size, level)
        stops.add(dec[:2])
    assert stops >= {(M.NONE, 0), (M.LOOKBACK, 0)} | {(M.CONSECUTIVE, k) for k in range(1, 8)}, stops


def test_the_table_covers_the_edges():
    decs = {n: E.oracle(n)[2] for n in NAMES}
    assert {d[:2] for d in decs.values()} >= {(M.NONE, 0), (M.LOOKBACK, 0)} | {(M.CONSECUTIVE, k) for k in range(1, 8)}
    assert {M.schedule(E.oracle(n)[1], E.by_name()[n].arr.size) for n in NAMES} == {0, 0x0f, 0x3f, 0xff, 0x1ff}
    assert {E.oracle(n)[0] for n in NAMES} >= {0, 10, 11, 17, 199, 200, 400, 600, 800, 26400}
    assert {d[2] for d in decs.values() if d[0] == M.LOOKBACK} == {12, 15}
    named = {v for r in E.rows() for v in r.variants}
    assert named == set(M.VARIANTS) - {"first_wave_stride"}                     # (the batch names that one)


def batch_inputs():
    chunks = E.batch_call(); out = []
    for name, a in chunks:
        sn, costs, dec = O.auto_delta_costs(a, O.make_config(**E.DEFAULT))
        out.append((costs, a.size, dec))
    return chunks, out


def test_the_batch_replay_over_wave_sub_lists_equals_the_sequential_decision():
    chunks, inp = batch_inputs()
    assert 22 <= len(chunks) <= 30
    got = M.batch([(c, n) for c, n, _ in inp])
    for (name, a), (c, n, dec), (d, mask) in zip(chunks, inp, got):
        assert d == dec == M.decide(c, n) and mask == M.schedule(c, n), name
    masks = [m for _, m in got]
    # every deeper wave runs, each over fewer chunks than the one before, and the chunks that go on are scattered among those that do not
    live = [[i for i, m in enumerate(masks) if m >> b & 1] for b in (0, 4, 6, 8)]
    assert len(live[0]) > len(live[1]) > len(live[2]) > len(live[3]) >= 2
    for deeper in live[1:]: assert any(j - i > 1 for i, j in zip(deeper, deeper[1:])), deeper
    assert sum(1 for m in masks if m == 0) >= 2
    names = [n for n, _ in chunks]; k = names.index("narrow_u8_n10_sums")
    assert chunks[k + 1][1].dtype == np.uint64 and chunks[k + 1][1].size == 10 and chunks[k][1].dtype == np.uint8
    assert names.count("monotone_stop5_u64") == 3
    by_n = {}
    for _, a in chunks: by_n.setdefault(a.size, set()).add(a.dtype.itemsize)
    assert by_n[10] >= {1, 8} and by_n[1000] == {1, 8}


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_a_wrong_reading_changes_every_row_that_names_it(variant):
    if variant == "first_wave_stride":
        _, inp = batch_inputs()
        right = M.batch([(c, n) for c, n, _ in inp]); wrong = M.batch([(c, n) for c, n, _ in inp], variant)
        assert [d for d, _ in wrong] != [d for d, _ in right]
        return
    named = [r for r in E.rows() if variant in r.variants]
    assert named, variant
    for r in named:
        sn, costs, dec = E.oracle(r.name); n = r.arr.size
        if variant == "stride_without_max":
            assert M.sample_positions(n, variant) is M.UNDEFINED and M.sample_positions(n) is not M.UNDEFINED, r.name
        elif variant == "raw_bits":                                            # the sample taken from the numbers' bits: the oracle on the unsigned view, no mode
            raw = r.arr.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[r.arr.dtype.itemsize])
            _, c2, _ = O.auto_delta_costs(raw, O.make_config(**dict(r.kw, mode=O.MODE_CLASSIC, mode_u64=0, mode_f64=0.0)))
            assert M.decide(c2, n) != dec, r.name
        else:
            assert M.decide(costs, n, variant) != dec, (r.name, variant, costs.tolist())


def test_hook_record_layout_is_the_headers(tmp_path):
    """pcodec_amd._lib.AutoDeltaRecord mirrors PcoGfxAutoDeltaRecord of include/pco_gfx.h field for field"""
    from pcodec_amd import _lib as G
    fields = [f[0] for f in G.AutoDeltaRecord._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "%s/include/pco_gfx.h"\nint main() { printf("%%zu", sizeof(PcoGfxAutoDeltaRecord)); %s return 0; }\n'
                   % (ROOT, " ".join('printf(" %%zu", offsetof(PcoGfxAutoDeltaRecord, %s));' % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-std=c++17", "-w", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(G.AutoDeltaRecord)] + [getattr(G.AutoDeltaRecord, f).offset for f in fields]
