"""The page layout model (pack_layout_model.py) and the rows of the bit packers' edge suite (pack_edges_util.py), on the CPU.

What the device suite (test_gpu_pack_edges.py) takes on trust is checked here: that the model finds the end of every row's chunk and its
padding from the bytes alone, that its bins are the oracle's, that its positions are those of the older one-variable model (tans_model), that
every row is routed to the packer it was built for and shows every condition it claims, that the families leave no required condition
unclaimed (but for the few no input can meet), and that three wrong restatements of the packers' arithmetic would have been noticed."""
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import pack_edges_util as E
import pack_layout_model as P
import tans_model as T

NAMES = [r.name for r in E.ROWS()]


@pytest.mark.parametrize("name", NAMES)
def test_the_model_finds_the_chunks_end_and_the_oracles_bins(name):
    """parse_chunk itself fails unless the last batch ends where the zero padding of the chunk's last byte begins; its bins are the oracle's."""
    chunk = E.oracle_chunk(name); L = E.layout(name); a = E.numbers(name)
    assert L.end_bits == 8 * len(chunk) and L.end_bits - L.body_last < 8 and L.n == a.size and L.latent_bits == a.dtype.itemsize * 8
    assert L.body_first == L.head_bits and L.meta_end <= L.head_bits <= L.body_last
    info, bins = O.inspect_first_chunk(E.oracle_file(name))
    for v in range(3):
        assert bool(info.var_present[v]) == L.present[v]
        if not L.present[v]: continue
        assert info.ans_size_log[v] == L.asl[v] and info.n_bins[v] == len(L.bins[v])
        assert [tuple(int(x) for x in b) for b in bins[v]] == [tuple(b) for b in L.bins[v]], (name, v)
    # sections follow one another without gaps, from the head to the body's last bit
    pos = L.body_first
    for v, b, kind, at, bits in P.sections(L):
        assert at == pos, (name, v, b, kind); pos += bits
    assert pos == L.body_last
    assert P.what_lies_at(L, 0) == "chunk meta" and P.what_lies_at(L, L.end_bits) == "beyond the chunk"
    if L.body_last > L.body_first: assert "section" in P.what_lies_at(L, L.body_last - 1)


def _other_chunks():
    """Chunks of the kinds the rows do not hold: float-mult and float-quant on f16 / f32 / f64, consecutive deltas of orders 1 .. 7 with both
    variables, signed types, 8-bit int-mult, lookback on a float-mult chunk, and levels 10 and 12 (up to 4096 bins)."""
    rng = np.random.default_rng(77)
    n = 3000
    with np.errstate(all="ignore"):
        quant = (rng.normal(0, 100, n).astype(np.float32).view(np.uint32) & np.uint32(0xFFF00000)).view(np.float32)
        yield "fmult-f64", rng.integers(1000, 900000, n) / 100.0, dict(mode=2, mode_f64=0.01, delta=1)
        yield "fmult-f32-o1", ((np.cumsum(rng.integers(-55, 56, n)) + 5000) * 0.1).astype(np.float32), dict(mode=2, mode_f64=0.1, delta=2, delta_order=1)
        yield "fmult-f16", (rng.integers(0, 2000, n) * np.float16(0.5)).astype(np.float16), dict(mode=2, mode_f64=0.5, delta=1)
        yield "fquant-f32", np.where(rng.random(n) < 0.2, (quant.view(np.uint32) | rng.integers(0, 4, n).astype(np.uint32)).view(np.float32), quant), dict(mode=3, mode_u64=20, delta=1)
        yield "fmult-f64-lookback", (rng.integers(0, 9000, 365)[np.arange(n) % 365] + 1000 + rng.integers(0, 3, n)) / 100.0, dict(mode=2, mode_f64=0.01, delta=3)
    yield "imult-i8", (rng.integers(-8, 8, n) * 7 + rng.integers(0, 3, n)).astype(np.int8), dict(mode=4, mode_u64=7, delta=1)
    yield "imult-i64-o7", ((np.cumsum(rng.integers(-3, 4, n)) + 500) * 1000 + rng.integers(0, 3, n)).astype(np.int64), dict(mode=4, mode_u64=1000, delta=2, delta_order=7)
    yield "classic-i16-o2", (np.cumsum(np.cumsum(rng.integers(-2, 3, n))) // 64).astype(np.int16), dict(mode=1, delta=2, delta_order=2)
    yield "classic-u32-level12", E.many_spikes(32, 65536, 6, k=3500, shift=10), dict(level=12, mode=1, delta=1)
    yield "classic-u64-level10", E.many_spikes(64, 20000, 5, k=900), dict(level=10, mode=1, delta=1)


@pytest.mark.parametrize("case", list(_other_chunks()), ids=[c[0] for c in _other_chunks()])
def test_the_model_reads_every_mode_delta_and_width(case):
    name, a, kw = case
    a = np.ascontiguousarray(a)
    f = O.simple_compress(a, O.make_config(**kw))
    header = 4 + 1 + 1 + (6 + max(int(a.size).bit_length(), 1) + 7) // 8 + 2
    L = P.parse_chunk(f[header:-1])
    info, bins = O.inspect_first_chunk(f)
    assert L.n == a.size and L.latent_bits == a.dtype.itemsize * 8 and L.end_bits == 8 * (len(f) - header - 1)
    assert L.mode == {1: 0, 4: 1, 2: 2, 3: 3}[kw["mode"]] and L.delta == kw["delta"] - 1 and L.order == kw.get("delta_order", 0), (name, L.mode, L.delta, L.order)
    for v in range(3):
        assert bool(info.var_present[v]) == L.present[v]
        if L.present[v]: assert [tuple(int(x) for x in b) for b in bins[v]] == [tuple(b) for b in L.bins[v]]
    assert sum(len(s.widths) for row in L.batches for v, s in row.items() if v == 1) in (0, L.n_lat[1])
    assert P.head_sections(L) and P.route(L, E.NONE) in P.ROUTE_BYTE
    if name.endswith("level12"): assert len(L.bins[1]) > 2048 and P.route(L, E.NONE) == "page"


def tans_positions(data, latent_bits):
    """tans_model's reading of a one-variable Classic / no-delta file, batch by batch: [(first bit of the batch, its tANS bits, its offset
    bits)], counted from the chunk's first byte.  tans_model.decode_one_chunk_file keeps no positions, so its loop is stepped here with its
    own reader (Bits, on the whole file, header included) and its own tables; that the stepping is right shows in the same test, where
    decode_one_chunk_file itself returns the row's latents from the same bytes."""
    r = T.Bits(data)
    r.read(32); r.read(8); r.read(8); r.read(1 + r.read(6)); r.align(); r.read(16)
    chunk_at = r.pos
    r.read(8); n = r.read(24) + 1
    assert r.read(4) == 0 and r.read(4) == 0
    size_log = r.read(4); n_bins = r.read(15)
    bins = [(r.read(size_log) + 1, r.read(latent_bits), r.read(P.OB_BITS[latent_bits])) for _ in range(n_bins)]
    r.align()
    nodes = T.decoder_nodes(size_log, [b[0] for b in bins])
    state = [r.read(size_log) for _ in range(T.INTERLEAVING)]
    r.align()
    out = []
    for start in range(0, n, T.BATCH_N):
        at = r.pos; syms = []
        for i in range(min(T.BATCH_N, n - start)):
            if n_bins == 1: syms.append(0); continue
            s, bits, base = nodes[state[i % 4]]
            syms.append(s); state[i % 4] = base + r.read(bits)
        mid = r.pos
        for s in syms: r.read(bins[s][2])
        out.append((at - chunk_at, mid - at, r.pos - mid))
    return out


# (tans_model reads its stream as one Python integer: a read costs the chunk's length, so the chunks of the longest copies -- 40 KB and more -- are
# left out; the J rows, 98 304 numbers in little over 100 bytes, are in)
ONE_VARIABLE = [r.name for r in E.ROWS() if r.kw["mode"] == 1 and r.kw["delta"] == 1 and r.kw["level"] == 8 and len(E.oracle_chunk(r.name)) <= 40000]


@pytest.mark.parametrize("name", ONE_VARIABLE)
def test_one_variable_rows_lie_where_tans_model_reads_them(name):
    L = E.layout(name); a = E.numbers(name)
    latents, _ = T.decode_one_chunk_file(E.oracle_file(name), L.latent_bits)
    assert latents == [int(x) for x in T.to_latent(a)]
    want = tans_positions(E.oracle_file(name), L.latent_bits)
    got = [(s.pos, s.ans_bits, s.off_bits) for row in L.batches for s in row.values()]
    if P.trivial(L, 1): want = []          # (a variable that writes nothing has no sections in the model)
    assert got == want


def test_enough_rows_are_compared_with_tans_model():
    assert len(ONE_VARIABLE) >= 100 and {E.BY_NAME()[n].family for n in ONE_VARIABLE} >= {"W", "S", "J", "T", "C", "P", "H"}
    assert {E.BY_NAME()[n].route for n in ONE_VARIABLE if E.BY_NAME()[n].family == "J"} == {"lean<2>", "lean<2, wide>", "general"}


def compact_is_plausible(row):
    """The row's word on which variables hold 16-bit latents, against what the chunk shows: a variable whose bins span fewer than 4096 values
    is counted in value space at any length, one longer than 8192 latents up to 32 768 values; lowers 32 768 or more apart (or one bin of 16
    or more offset bits) rule 16-bit latents out, and so do more than 256 histogram bins."""
    L = E.layout(row.name)
    for v in range(3):
        if not L.present[v] or P.trivial(L, v): continue
        lows = [lo for _, lo, _ in L.bins[v]]
        tops = [min(lo + (1 << ob) - 1, nxt - 1) for (_, lo, ob), nxt in zip(L.bins[v], lows[1:] + [1 << 64])]   # (a bin ends below the next one)
        span = max(tops) - min(lows)
        big = row.kw["level"] > 8 and L.n >= 8192
        if row.compact[v]:
            if big or not (span < 4096 or (L.n_lat[v] > 8192 and span < 32768)): return False
        elif not (big or max(lows) - min(lows) >= 32768 or max(ob for _, _, ob in L.bins[v]) >= 16): return False
    return True


@pytest.mark.parametrize("call", E.CALLS(), ids=[c.name for c in E.CALLS()])
def test_every_row_takes_its_route_and_meets_its_conditions(call):
    """A row that misses its route or one of its conditions is an error, never a skip.  (On the CPU the 16-bit latents of a variable are the
    row's word, checked for plausibility; the device suite reads them back.)"""
    routes = E.predicted_routes(call)
    for name in call.rows:
        row = E.BY_NAME()[name]
        assert row.claims, name
        assert routes[name] == row.route, (name, routes[name], row.route)
        assert row.route in P.ROUTE_BYTE
        missed = [c for c in row.claims if not E.holds(row, c)]
        assert not missed, (name, missed)
        assert compact_is_plausible(row), name
        assert E.numbers(name).size <= 100000


def test_no_required_condition_is_left_unclaimed():
    """Every condition of REQUIRED is claimed by a row, or marked unreachable (three at most), or asks for an offset wider than the route's
    variables can be (WIDTH_LIMITED, each with its reason: eight, all of them full-width-offset conditions) -- exactly one of the three."""
    assert len(E.UNREACHABLE) <= 3 and all(len(why) > 20 for why in list(E.UNREACHABLE.values()) + list(E.WIDTH_LIMITED.values()))
    assert len(E.WIDTH_LIMITED) == 8 and not set(E.WIDTH_LIMITED) & set(E.UNREACHABLE)
    assert {k[3] for k in E.WIDTH_LIMITED} == {"sec:bmax_in=64..64", "sec:bmax=32", "sec:outliers_at_lanes_0_63", "full64_after_pending"}
    for key, conds in E.REQUIRED.items():
        have = E.coverage(*key)
        assert any(r.family == key[0] and r.route in key[1] for r in E.ROWS()), key
        for c in conds:
            assert [c in have, key + (c,) in E.UNREACHABLE, key + (c,) in E.WIDTH_LIMITED].count(True) == 1, (key, c)
    for key in list(E.UNREACHABLE) + list(E.WIDTH_LIMITED):
        assert key[3] in E.REQUIRED[key[:3]]
    # the staging conditions on every route that packs through PackSink
    for rt in ("general", "lean<2>", "lean<2, wide>", "lean<6>", "lean<3>"):
        assert set(E.S_ALL) <= set(E.REQUIRED[("S", (rt,), None)])


def test_the_walk_and_pack_call_is_arranged_as_described():
    """40 pages: two whole blocks of sixteen and a last one of eight; items 2 k and 2 k + 1 share a packing wave -- a long page beside a short
    one in both orders, and a constant page among them."""
    call = next(c for c in E.CALLS() if c.name == "P")
    nb = [len(E.layout(n).batches) for n in call.rows]
    assert len(call.rows) == 40 and call.shifts == (8,)
    pairs = [(nb[i], nb[i + 1]) for i in range(0, 40, 2)]
    assert any(a >= 5 and b <= 2 for a, b in pairs) and any(a <= 2 and b >= 5 for a, b in pairs)
    assert any(E.holds(E.BY_NAME()[n], "writes_nothing") for n in call.rows[:32])
    assert {1, 2, 3, 5} <= set(nb) and any(E.numbers(n).size % 256 for n in call.rows)
    # the second walk-and-pack call: more than 4096 items, so no segmented walk, and two pieces per page for enc_place_kernel
    assert all(E.numbers(f"P-u8-long-{i}").size == 32768 and E.predicted_routes(E.Call("x", E.CLASSIC, (f"P-u8-long-{i}",) * 4112, (0,)))[f"P-u8-long-{i}"] == "walkp" for i in range(3))


def answer(row, variants):
    """What the model says of a row: its claims, its runs, every flush of every stage and where its offset fields lie."""
    L = E.layout(row.name)
    fields = hashlib.sha256(repr(P.fields(L, variants)[:4096]).encode()).hexdigest()
    return (tuple(E.holds(row, c, variants) for c in row.claims), tuple(P.runs(L, variants)),
            tuple(tuple(s[1]) for s in P.run_schedules(L, row.route, variants)), fields)


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_a_wrong_restatement_changes_a_rows_answer(variant):
    """Offsets before tANS bits, runs of 32 batches, a reserve without the reach of a put: each changes what the model says of some row
    and turns a claim of some row false (the fields that end 32, 33, 64 and 65 bits into their dword; six runs; a flush the reach decides)."""
    changed = [r.name for r in E.ROWS() if r.family in "WSJ" and answer(r, (variant,)) != answer(r, ())]
    assert changed, variant
    assert any(not E.holds(r, c, (variant,)) for r in E.ROWS() if r.family in "SJ" for c in r.claims), variant


def test_sink_schedule_by_hand():
    """The issue's note, by the restated arithmetic: a u64 page of one bin of 43 offset bits passes its second batch's reserve 408 bits below
    the threshold, one of 44 bits flushes 104 beyond it."""
    for k, d in ((43, 408), (44, -104)):
        L = E.layout(f"S-u64-ob{k}")
        assert L.head_bits == 136 and [s.off_bits for row in L.batches for s in row.values()] == [256 * k] * 5
        stage = P.run_schedules(L, "lean<2, wide>")[1]
        assert stage[0] == "run0" and stage[2][:2] == [P.kStgDwords * 32 - (8 + 256 * k + P.kPutReach), d]
    fits = 22528 - 96 - 5 - 103   # what a stage that starts at bit 5 of its dword and holds 103 bits has room for
    flushes, dist, pends = P.sink_schedule(5, [(100, 100), (None, 3), (fits, fits), (1, 1)])
    assert dist == [22528 - 96 - 5 - 100, 0, -1] and flushes == [5 + 103 + fits] and pends == [0, 103, 103 + fits]


def test_routes_by_hand():
    L = E.layout("S-u64-ob43")
    assert P.route(L, E.NONE) == "lean<2, wide>" and P.route(L, E.PRIMARY) == "lean<2>" and P.route(L, E.NONE, walkp=True) == "walkp"
    assert P.route(E.layout("C-u32-16384"), E.NONE) == "copy" and P.route(E.layout("C-u32-16384"), E.PRIMARY) == "lean<2>"
    assert P.route(E.layout("C-u16-16384"), E.NONE) == "copy" and P.route(E.layout("T-general-1"), E.NONE) == "general"
    assert P.route(E.layout("T-page-1"), E.NONE) == "page" and P.route(E.layout("C-u32-1"), E.PRIMARY) == "general"
    assert P.walkp_verdict(E.layout("P-body0"), E.PRIMARY, 1) == "ok" and P.walkp_verdict(E.layout("P-body0"), E.NONE, 1) == "bad"
    assert P.walkp_verdict(E.layout("P-constant"), E.PRIMARY, 1) == "idle" and P.walkp_verdict(E.layout("T-lean6-1"), E.BOTH, 2) == "bad"
    assert P.call_slots([dict(mode=1, delta=1)]) == (1,) and P.call_slots([dict(mode=4, delta=3)]) == (0, 1, 2)
