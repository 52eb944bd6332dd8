"""The rows of the segmented encode walk's edge suites (test_walkseg_model.py on the CPU, test_gpu_walkseg_edges.py on the device).

enc_walkseg_kernel decides where a chain's ends have met, what to walk again and in which round.  A row puts a meeting where one of those
decisions is made.  The tables that make this possible:

  * two values, `heavy` everywhere and `rare` at a few chosen positions, train to two bins of weights (T - 1, 1): under the heavy symbol alone
    the arc never closes, one step of the rare symbol sends every state to one state, so chain j of a segment meets exactly at the highest
    index = j (mod 4) of the segment that holds the rare value (two_valued; expected_events states what follows for fix_n, the rounds and
    the chain that met last, by that rule alone -- the model's arc simulation must agree);
  * three values, two of about equal weight and a rare one, train to (T/2 - 1, T/2, 1): left alone their chains meet after thousands of
    steps and take the `all` reset of ws_step2 tens to hundreds of times on the way (three_valued).

A position is (segment, batch in walk order, group in the batch, chain): the latent 4 * group + chain of the batch; group 63 is the first of a
full batch the walk reaches, group 0 the last.  What a row claims is checked on the CPU against walkseg_model on the oracle's chunk; which
mutants of the kernel a row must reveal is part of the claim."""
import collections
import functools

import numpy as np

import latent_window_util as LW
import oracle_lib as O
import walkseg_model as M

Row = collections.namedtuple("Row", "name cls kw make n_lat positions weights reveals source claims")
# cls: G geometry, T top segment, M meeting, R redo chains, A the `all` reset, S symbol sources, O consecutive orders, V several variables, B many bins
# weights: the sorted weights the oracle must train for the primary; reveals: mutants the row must reveal; claims: extra (key, value) checks

HEAVY, RARE = 5, 77


def standalone_header_len(n_hint):
    """magic, standalone version, uniform type byte, the varint n_hint, the wrapped format's two bytes"""
    return 4 + 1 + 1 + (6 + max(int(n_hint).bit_length(), 1) + 7) // 8 + 2


def kw_of(level=8, order=0, **extra):
    kw = dict(level=level, mode=1, delta=2 if order else 1)
    if order: kw["delta_order"] = order
    kw.update(extra)
    return kw


def latent_index(n_lat, pos):
    q, it, grp, j = pos
    g = M.geometry(n_lat)
    lo, nl, nbq = g.segs[q]
    i = (nbq - 1 - it) * M.kBatchN + 4 * grp + j
    assert 0 <= it < nbq and 0 <= grp < 64 and i < nl, (pos, g.segs[q])
    return lo + i


def START(n_lat, q, chains=(0, 1, 2, 3)):
    """Every chain of segment q meets at the first latent of it that the walk reaches."""
    g = M.geometry(n_lat); lo, nl, nbq = g.segs[q]
    out = []
    for j in chains:
        last = nl - 1 - ((nl - 1 - j) % 4)             # the highest index = j (mod 4) of the segment
        b = last // M.kBatchN
        out.append((q, nbq - 1 - b, (last % M.kBatchN) // 4, j))
    return out


def from_latent_values(lat, dtype, order):
    """Numbers whose stored latents (after `order` rounds of differences; the toggle 2^(w-1) added when order > 0) are `lat`."""
    w = np.dtype(dtype).itemsize * 8
    if order == 0:
        return np.ascontiguousarray(np.asarray(lat, np.int64).astype(dtype))
    dd = [0] * order + [int(x) for x in lat]
    seq = LW.integrate(dd, order, [1000 + 7 * r for r in range(order)], w)
    u = LW.F.UINT[w]
    return np.ascontiguousarray(np.array(seq, dtype=np.uint64).astype(u).view(dtype) if np.dtype(dtype).kind != "u" else np.array(seq, dtype=np.uint64).astype(u))


def two_valued(n, rare_positions, heavy=HEAVY, rare=RARE, dtype=np.uint32, level=8, delta_order=0):
    """n numbers: `heavy` everywhere, `rare` at the positions (segment, batch in walk order, group, chain) of the n - delta_order latents."""
    n_lat = n - delta_order
    lat = np.full(n_lat, heavy, np.int64)
    for p in rare_positions:
        lat[latent_index(n_lat, p)] = rare
    return from_latent_values(lat, dtype, delta_order)


def three_valued(n, seed, rare_positions, values=(5, 6, 77), dtype=np.uint32):
    """Two values at about 50/50 (never exactly: one more of the second) and a rare third at `rare_positions`."""
    rng = np.random.default_rng(seed)
    lat = np.where(rng.random(n) < 0.5, values[0], values[1]).astype(np.int64)
    k = int((lat == values[0]).sum()) - int((lat == values[1]).sum())
    flip = np.flatnonzero(lat == (values[0] if k >= 0 else values[1]))[: (abs(k) + 1) // 2 + 8]
    lat[flip] = values[1] if k >= 0 else values[0]
    for p in rare_positions:
        lat[latent_index(n, p)] = values[2]
    return np.ascontiguousarray(lat.astype(dtype))


# ------------------------------------------------------------------------------------------------ what a two-valued page must do
Expected = collections.namedtuple("Expected", "geom fix whole met_in_last last_chain round rounds met")


def expected_events(n_lat, positions):
    """By the rule of the two-valued tables alone: a chain of a segment below the top is open at every batch start up to the batch of its
    highest rare latent, or throughout; the top segment starts from one state."""
    g = M.geometry(n_lat)
    fix, whole, mil, last, met = [], [], [], [], []
    for q, (lo, nl, nbq) in enumerate(g.segs):
        if q + 1 == g.n_seg:
            fix.append(0); whole.append(nbq == 0); mil.append(False); last.append(None); met.append(True); continue
        top_of = {}
        for p in positions:
            if p[0] != q: continue
            i = latent_index(n_lat, p)
            top_of[p[3]] = max(top_of.get(p[3], -1), i)
        opens = [nbq if j not in top_of else nbq - (top_of[j] - lo) // M.kBatchN for j in range(4)]
        fix.append(max(opens)); whole.append(max(opens) == nbq); met.append(len(top_of) == 4); mil.append(max(opens) == nbq and len(top_of) == 4)
        never = [j for j in range(4) if j not in top_of]
        last.append(None if len(never) > 1 else never[0] if never else min(top_of, key=top_of.get))
    rnd = [None] * g.n_seg
    for q in range(g.n_seg - 2, -1, -1):
        rnd[q] = 0 if met[q + 1] else rnd[q + 1] + 1
    return Expected((g.nb, g.nbs, g.n_seg), fix, whole, mil, last, rnd, max([r for r in rnd if r is not None], default=-1) + 1, met)


# ------------------------------------------------------------------------------------------------ the rows
def _rows():
    rows = []

    def add2(name, cls, n, positions, reveals=(), level=8, dtype=np.uint32, order=0, heavy=HEAVY, rare=RARE, source=None, claims=(), extra_kw=None):
        T = 1 << (level + 2)
        kw = kw_of(level, order, **(extra_kw or {}))
        rows.append(Row(name, cls, kw, functools.partial(two_valued, n, tuple(positions), heavy, rare, dtype, level, order), n - order, tuple(positions),
                        (1, T - 1), tuple(reveals), source, tuple(claims)))

    def all_start(n_lat, skip=()):
        g = M.geometry(n_lat)
        return [p for q in range(g.n_seg - 1) if q not in skip for p in START(n_lat, q)]

    B = M.kBatchN
    # ---- G: geometry.  A rare in every chain at the top of segment 0 and of a middle segment: everything between hands over through rounds
    for nb, lvl in ((64, 8), (65, 8), (75, 2), (79, 6), (80, 8), (81, 6), (112, 4), (113, 8)):
        n = nb * B; g = M.geometry(n)
        pos = START(n, 0) + START(n, g.n_seg // 2)
        add2(f"G-nb{nb}-nbs{g.nbs}-seg{g.n_seg}", "G", n, pos, reveals=("a", "d", "h") + (("e",) if g.n_seg == 16 else ()), level=lvl, claims=(("geom", (nb, g.nbs, g.n_seg)),))
    for nb, n, lvl in ((1024, 1 << 18, 4), (1025, (1 << 18) + 1, 6)):   # (1025 batches: one page only with max_page_n above the default 2^18)
        g = M.geometry(n)
        add2(f"G-nb{nb}-nbs{g.nbs}-seg{g.n_seg}", "G", n, START(n, 0) + START(n, 8) + START(n, 14), reveals=("a", "d", "h", "e"), level=lvl, claims=(("geom", (nb, g.nbs, g.n_seg)),),
             extra_kw=dict(max_page_n=1 << 19) if nb == 1025 else None)
    # ---- T: the top segment: a full segment, one full batch, one partial batch of 255 / 4 / 3 / 1 latents, a full batch and a partial one
    for tag, n in (("full-segment", 80 * B), ("one-batch", 66 * B), ("partial255", 65 * B + 255), ("partial4", 65 * B + 4), ("partial3", 65 * B + 3),
                   ("partial1", 65 * B + 1), ("batch+partial100", 66 * B + 100)):
        g = M.geometry(n); top = g.n_seg - 1
        nl_top = g.segs[top][1]
        rare_top = [(top, 0, 0, j) for j in range(min(4, nl_top - (g.segs[top][2] - 1) * B))] if nl_top < 5 * B else START(n, top)   # a rare in every chain the top's last batch has
        add2(f"T-top-{tag}", "T", n, all_start(n) + rare_top, reveals=("h",), level=(6, 4, 2)[len(rows) % 3], claims=(("top_latents", nl_top),))
    # ---- M: where a chain meets.  nb = 80 (sixteen segments of five batches); segment 7's chain j at the place, its other chains and every other
    # segment at their start; two rares of the other pair of lanes lower in segment 7 (they show a batch total that lost that pair)
    n = 80 * B
    places = {"first-walked": (0, 63), "end-of-first-batch": (0, 0), "end-of-batch1": (1, 0), "start-of-batch2": (2, 63), "end-of-batch2": (2, 0),
              "one-before-last": (3, 10), "last-batch": (4, 32)}
    fixes = {"first-walked": 1, "end-of-first-batch": 1, "end-of-batch1": 2, "start-of-batch2": 3, "end-of-batch2": 3, "one-before-last": 4, "last-batch": 5}
    for pname, (it, grp) in places.items():
        for j in range(4):
            others = [c for c in range(4) if c != j]
            pos = all_start(n, skip=(7,)) + START(n, 7, others) + [(7, it, grp, j)] + [(7, k, 5, j ^ 2) for k in range(1, it + 1)]
            rv = ("h",) + (("a",) if fixes[pname] == 5 else ()) + (("b",) if j < 2 and it >= 1 else ())
            add2(f"M-{pname}-chain{j}", "M", n, pos, reveals=rv, level=(6, 4)[j % 2], claims=(("fix", (7, fixes[pname])),) + ((("last", (7, j)),) if pname != "first-walked" else ()))
    for j in range(4):   # three chains meet, one never does
        pos = all_start(n, skip=(7,)) + START(n, 7, [c for c in range(4) if c != j])
        add2(f"M-chain{j}-never", "M", n, pos, reveals=("a", "f", "h"), level=(4, 2)[j % 2], claims=(("fix", (7, 5)), ("last", (7, j)), ("unmet", 7)))
    for ja, jb in ((0, 1), (2, 3), (0, 2), (1, 3)):   # two chains meet, two never do: the segment below must wait for the whole quad above
        pos = all_start(n, skip=(7,)) + START(n, 7, [c for c in range(4) if c not in (ja, jb)])
        add2(f"M-chains{ja}{jb}-never", "M", n, pos, reveals=("a", "f", "h"), level=(6, 4)[ja % 2], claims=(("fix", (7, 5)), ("unmet", 7)))
    add2("M-met-at-once-beside-open-to-the-end", "M", n, all_start(n, skip=(9,)), level=6, reveals=("a", "h"), claims=(("fix", (9, 5)), ("fix", (8, 1)), ("unmet", 9)))
    # ---- R: redo chains: runs of k segments without a rare, a met segment (or the top) above, a segment with a rare in every chain below
    def run_row(name, runs, nb=80, level=6, reveals=("a", "h"), rounds=None):
        n = nb * B; g = M.geometry(n)
        skip = [q for a, k in runs for q in range(a, a + k)]
        add2(name, "R", n, all_start(n, skip=skip), reveals=reveals, level=level, claims=(("rounds", rounds),) if rounds else ())
    for k in (1, 2, 3, 5, 14):
        run_row(f"R-run{k}", [(1, k)] if k == 14 else [(4, k)], reveals=("a", "h") + (("d",) if k >= 4 else ()), rounds=k + 1, level=(8, 6, 4, 2)[k % 4])
    run_row("R-run11-of-13-segments", [(1, 11)], nb=64, reveals=("a", "d", "h"), rounds=12)
    run_row("R-two-runs", [(2, 3), (9, 4)], level=4, reveals=("a", "d", "h"), rounds=5)
    run_row("R-run-under-the-top", [(12, 3)], reveals=("a", "e", "h"), rounds=4)
    run_row("R-run-at-the-bottom", [(0, 3)], level=2, reveals=("a", "h"), rounds=3)
    n = 80 * B
    add2("R-only-rare-in-the-top", "R", n, START(n, 15), reveals=("a", "d", "h"), claims=(("rounds", 15),))
    # ---- S: symbol sources: the range of the two values decides where the walker's symbols come from
    def src_row(name, rng_, dtype, level=8, want=None):
        n = 64 * B
        add2(name, "S", n, START(n, 0) + START(n, 6) + START(n, 11), reveals=("h",), level=level, dtype=dtype, heavy=HEAVY, rare=HEAVY + rng_, source=want)
    for dt in (np.uint16, np.uint32, np.int64, np.uint8):
        src_row(f"S-range72-{np.dtype(dt).name}", 72, dt, want="all_lds")
    for lvl in (8, 6, 4, 2):
        edge = M.kWsSymBase - M.vt_off(lvl + 2, 2) - 1
        edge = min(edge, 4095)
        src_row(f"S-L{lvl}-range{edge}-last-in-lds", edge, np.uint32, lvl, "all_lds")
        if edge + 1 < M.kDirectHistRange:
            src_row(f"S-L{lvl}-range{edge + 1}-first-beyond", edge + 1, np.uint32, lvl, "finds")
    src_row("S-range4095-finds-ends", 4095, np.uint16, 8, "finds")
    src_row("S-range4096-stages", 4096, np.uint16, 8, "stages")
    src_row("S-range2^20-u32-stages", 1 << 20, np.uint32, 8, "stages")
    src_row("S-range2^20-i64-stages", 1 << 20, np.int64, 6, "stages")
    # ---- O: consecutive orders: n_lat = n - order, the page's first latent is not the page's first number
    for order in (1, 2, 7):
        n = 64 * B + order
        add2(f"O-order{order}-16384-latents", "O", n, all_start(n - order), reveals=("h",), order=order, level=6)
    # ---- A: the `all` reset (three-valued; seeds chosen on the CPU, see A_SEEDS)
    for lvl, n, seed in A_SEEDS:
        T = 1 << (lvl + 2); g = M.geometry(n); mid = g.segs[3][2] // 2
        pos = tuple(START(n, 0) + [(3, mid, 30, j) for j in range(4)] + START(n, 9) + START(n, 13))
        rows.append(Row(f"A-L{lvl}-n{n}-seed{seed}", "A", kw_of(lvl), functools.partial(three_valued, n, seed, pos), n, pos, (1, T // 2 - 1, T // 2),
                        ("c", "h"), None, (("resets", 10),)))
    # ---- V: more than one variable.  Int-mult (base 8): quotient and remainder both two-valued, their rares in different segments; float-mult
    # with a constant secondary (one bin: nothing to walk)
    n = 64 * B
    qpos = tuple(START(n, 0) + START(n, 5) + START(n, 10)); rpos = tuple(START(n, 2) + START(n, 7))
    rows.append(Row("V-int-mult-i64-base8", "V", dict(level=8, mode=4, mode_u64=8, delta=1),
                    lambda: (two_valued(n, qpos, dtype=np.int64) * 8 + two_valued(n, rpos, 1, 6, dtype=np.int64)).astype(np.int64), n, None, (1, 1023), ("a", "d", "h"), None, (("vars", (1, 2)),)))
    rows.append(Row("V-float-mult-f32-constant-secondary", "V", dict(level=8, mode=2, mode_f64=0.25, delta=1),
                    lambda: (two_valued(n, qpos, 40, 112).astype(np.float32) * np.float32(0.25)), n, None, (1, 1023), ("a", "d", "h"), None, (("vars", (1,)),)))
    # lookback on a periodic opening with a long two-valued tail: the lookback variable is item page * n_slots + 0 (two slots; three with int-mult)
    tn = n + 512
    def lb_numbers(mult):
        per = np.random.default_rng(9).integers(0, 1 << 12, 37)[np.arange(2048) % 37].astype(np.int64)
        x = np.concatenate([per, two_valued(tn, START(tn, 0) + START(tn, 6)).astype(np.int64)])
        if mult: x = x * 8 + np.concatenate([np.zeros(2048, np.int64), two_valued(tn, START(tn, 3), 1, 6).astype(np.int64)])
        return x.astype(np.uint32)
    rows.append(Row("V-lookback-two-slots", "V", dict(level=8, mode=1, delta=3), functools.partial(lb_numbers, False), 2048 + tn - 1, None, (1, 2, 1021), ("a", "c", "d", "h"), None, (("vars", (0, 1)),)))
    rows.append(Row("V-lookback-int-mult-three-slots", "V", dict(level=8, mode=4, mode_u64=8, delta=3), functools.partial(lb_numbers, True), 2048 + tn - 1, None, (1, 2, 1021), ("a", "c", "d", "h"), None,
                    (("vars", (0, 1, 2)),)))
    # ---- B: many bins at a table of 2^10 states: with 256 bins the info words end where the symbol buffers begin (no room for the value table),
    # with 200 the value table still fits behind them
    for b, src in ((256, "finds"), (200, "all_lds")):
        rows.append(Row(f"B-{b}-bins", "B", kw_of(8), functools.partial(many_bins, b), sum(384 if i % 2 == 0 else 64 for i in range(b)), None, None, ("h",), src, (("bins", b),)))
    return rows


def many_bins(b):
    """Every value below b of a byte, 384 and 64 of them by turns (bins the partition does not merge), shuffled."""
    a = np.repeat(np.arange(b).astype(np.uint8), np.where(np.arange(b) % 2 == 0, 384, 64))
    np.random.default_rng(b).shuffle(a)
    return a


# (level, n, seed): three-valued pages with a segment that takes at least ten resets before a meeting in mid-segment and a segment that never meets
A_SEEDS = tuple((lvl, n, seed) for lvl in (8, 6, 4) for n in ((1 << 16) + 255, 1 << 18) for seed in (1, 2))

SHORT = {   # pages one latent short of the segmented walk, encoded beside the long ones: they stay with the unsegmented walkers
    "short-16383": (lambda: two_valued(64 * 256 - 1, [(0, 0, 0, 0), (5, 2, 7, 1)]), kw_of(8)),
    "short-16383-order1": (lambda: two_valued(64 * 256, [(0, 0, 0, 0), (5, 2, 7, 1)], delta_order=1), kw_of(6, 1)),
    "short-16383-order2": (lambda: two_valued(64 * 256 + 1, [(0, 0, 0, 0), (5, 2, 7, 1)], delta_order=2), kw_of(6, 2)),
    "short-16383-order7": (lambda: two_valued(64 * 256 + 6, [(0, 0, 0, 0), (5, 2, 7, 1)], delta_order=7), kw_of(6, 7)),
}


@functools.lru_cache(maxsize=None)
def ROWS():
    rows = _rows()
    assert len({r.name for r in rows}) == len(rows)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def BY_NAME():
    return {r.name: r for r in ROWS()}


@functools.lru_cache(maxsize=None)
def numbers(name):
    a = np.ascontiguousarray(SHORT[name][0]() if name in SHORT else BY_NAME()[name].make())
    a.setflags(write=False)
    return a


def kw(name):
    return dict(SHORT[name][1]) if name in SHORT else dict(BY_NAME()[name].kw)


@functools.lru_cache(maxsize=None)
def oracle_file(name):
    return O.simple_compress(numbers(name), O.make_config(**kw(name)))


@functools.lru_cache(maxsize=None)
def oracle_chunk(name):
    """The standalone chunk the oracle writes for the row: its one-chunk file without header and terminator."""
    return oracle_file(name)[standalone_header_len(numbers(name).size):-1]


@functools.lru_cache(maxsize=None)
def walks(name):
    """({variable: PageWalk}, Decoded) of the row's oracle chunk."""
    return M.page_walks(oracle_chunk(name))


def took_heapsort(name):
    """chunk_plan's flag: the reference's histogram took its heapsort branch on this row (the device would not be compared)."""
    return O.chunk_plan(numbers(name), O.make_config(**kw(name)))[2]


def source_of(name, v=1):
    """The model's word on where the walker's symbols of variable v come from."""
    r = BY_NAME()[name]; a = numbers(name)
    an = LW.analyse(a, r.kw, [a.size])
    _, d = walks(name)
    rng_ = an.ranges[v - 1]
    return M.source(an.route == "c16", rng_, d.layout.asl[v], len(d.layout.bins[v]))


# ------------------------------------------------------------------------------------------------ several pages
def paged_numbers(pages, seed=0):
    """A chunk in `pages`: every page two-valued with the rares where its own geometry puts the start of each of its segments (a short page: a
    rare in each chain near its end).  The table is the chunk's; every page's top segment starts from T."""
    parts = []
    for k, pn in enumerate(pages):
        if pn >= M.kWsMinBatches * M.kBatchN:
            g = M.geometry(pn)
            parts.append(two_valued(pn, [p for q in range(0, g.n_seg - 1, 2 + k % 2) for p in START(pn, q)]))
        else:
            a = np.full(pn, HEAVY, np.uint32); a[max(pn - 9, 0)::2] = RARE; parts.append(a)
    return np.ascontiguousarray(np.concatenate(parts))


PAGED_KW = kw_of(6)
EXACT_LISTS = ([16384, 16383, 20000, 300], [20736, 16385])
EQUAL_CASES = ((40000, 16384), (49152, 16384))       # (n, max_page_n): three pages of 13 334 / 13 333 (none is long) and three of 16 384
SIMPLE_MAX_PAGE_N = (120000, 50000)                  # through simple_compress: three chunks of 40 000


def equal_pages(n, max_page_n):
    k = -(-n // max_page_n)
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


@functools.lru_cache(maxsize=None)
def paged_case(key):
    """("exact", i) / ("equal", i) -> (numbers, page sizes, oracle (meta, pages, page_ns))"""
    kind, i = key
    pages = list(EXACT_LISTS[i]) if kind == "exact" else equal_pages(*EQUAL_CASES[i])
    a = paged_numbers(pages); a.setflags(write=False)
    cfg = O.make_config(max_page_n=0 if kind == "exact" else EQUAL_CASES[i][1], **PAGED_KW)
    return a, pages, O.wrapped_compress(a, cfg, max_pages=len(pages) + 1, exact_pages=pages if kind == "exact" else None)


PAGED_KEYS = (("exact", 0), ("exact", 1), ("equal", 0), ("equal", 1))


def configs():
    """The rows by config: one pco_gfx_compress_chunks call each."""
    out = collections.OrderedDict()
    for r in ROWS():
        out.setdefault(tuple(sorted(r.kw.items())), []).append(r.name)
    for name in SHORT:
        out.setdefault(tuple(sorted(kw(name).items())), []).append(name)
    return out
