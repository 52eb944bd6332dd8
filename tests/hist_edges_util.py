"""The rows that stand on every comparison of the quantile histogram's bin walk (histograms.rs; K2 of pcodec_amd/csrc/encode_kernels.hip), for
tests/test_hist_model.py (-m "not gpu") and tests/test_gpu_hist_edges.py (-m gpu).  The plain model is tests/hist_model.py.

A row is DESIGNED IN RANK SPACE: the sorted multiset of one variable's latents is "rank r holds key r" (all distinct) except for a few runs
[st, en) of equal values (key st), placed against c_count(b) of a bin in the middle; latent = base + step * key, so `step` alone moves the
same design through the counting tiers of latent_window_util.TIERS (direct, small, mid, wide, select), and the stored order is a seeded
shuffle with a chosen latent in front (the 16-bit speculation is centred on the first one).  Where a design has a free length or gap, the
builder searches the few candidates for the first one on which the model reports the branches the row is named for AND whose bins change
under every variant it names; a design that cannot be realised fails the build of the rows, it is not dropped.

Sections: (a) the walk's comparisons, at 256 bins (n = 4096 and 4500) and 64 bins (n = 300); (b) counts on both sides of n >= B, 8 and
16-bit types; (c) a subset of (a) through every producer of rank records, plus the radix-sort fallback of enc_hist_select_kernel, a lookback
delta variable and an int-mult secondary capped at 64 bins; (d) consecutive deltas whose unstored positions hold the heavy value or values
outside [min, max]; (e) more than 256 bins (levels 9 and 12); (f) the no-delta rows of (a) and (b) once more with strict histograms."""
import collections
import functools

import numpy as np

import format_limits_util as F
import hist_model as M
import latent_window_util as W
import lookback_model as LB
import oracle_lib as O

Row = collections.namedtuple("Row", "name about arr kw pages paging section variants strict gives_up var needs")
# var: the variable the design lives in (0 delta, 1 primary, 2 secondary); needs: {run start rank: branch names the model must report there};
# gives_up: enc_hist_select_kernel hands the variable to enc_hist_sort_kernel (hist_path == 2)
Design = collections.namedtuple("Design", "name about runs variants needs")

CLASSIC = dict(mode=1, delta=1)


def cfg_kw(level=8, **kw):
    out = dict(CLASSIC); out.update(kw); out["level"] = level
    return out


# ------------------------------------------------------------------------------------------------ rank space
def keys_of(n, runs):
    key = list(range(n)); last = 0
    for st, en in sorted(runs):
        assert last <= st < en <= n, (runs, n)
        key[st:en] = [st] * (en - st); last = en
    return key


class Geo:
    def __init__(self, n, bl):
        self.n, self.bl, self.B = n, bl, 1 << bl
        self.binw = n // self.B
        self.k = self.B // 2
        self.p0 = self.cc(self.k - 1)

    def cc(self, b): return M.c_count(b, self.n, self.bl)
    def bi(self, c): return M.bin_idx(c, self.n, self.bl)


def _check(n, bl, runs, needs, variants):
    s = keys_of(n, runs)
    bins, rep = M.histogram_sorted(s, bl)
    for st, names in needs.items():
        step = rep.step_of(st)
        if step is None or not set(names) <= set(step[0]):
            return False
    return all(M.histogram_sorted(s, bl, (v,))[0] != bins for v in variants)


def _search(n, bl, cands, what):
    """The first (runs, needs, variants) of `cands` that the model confirms."""
    for runs, needs, variants in cands:
        if all(0 <= st < en <= n for st, en in runs) and _check(n, bl, runs, needs, variants):
            return runs, needs
    raise AssertionError(("no realisation", what, n, bl))


@functools.lru_cache(maxsize=None)
def designs(n, bl):
    """Every design of section (a) at n latents and 2^bl bins."""
    g = Geo(n, bl); cc, bi, k, p0, w = g.cc, g.bi, g.k, g.p0, g.binw
    assert w >= 4 and g.B >= 16
    out = []

    def add(name, about, runs, variants=(), needs=None):
        needs = needs or {}
        assert _check(n, bl, runs, needs, variants), (name, n, bl, runs)
        out.append(Design(name, about, tuple(runs), tuple(variants), needs))

    def found(name, about, cands, variants):
        runs, needs = _search(n, bl, [(r, nd, variants) for r, nd in cands], name)
        out.append(Design(name, about, tuple(runs), tuple(variants), needs))

    h = max(3, w // 2 + 1); c = cc(k)
    add("heavy-mid-ends@c-1", "a run inside a middle bin ends one rank before the bin's end: nothing straddles", [(c - 1 - h, c - 1)])
    add("heavy-mid-ends@c", "a run of several ranks ends exactly on c_count(b): en <= c absorbs it", [(c - h, c)], needs={c - h: ("absorb_run_ends_at_c",)})
    add("heavy-mid-ends@c+1", "the same run one rank longer straddles c: prefix, no spare, joins the prefix and completes beyond", [(c + 1 - h, c + 1)],
        needs={c + 1 - h: ("prefix", "no_spare", "joins_pending", "completes_beyond")})
    for d in (-1, 0, 1):
        if cc(0) + d >= 2:
            add(f"first-bin-run-from-rank0-ends@c{d:+d}", "the run starts at rank 0 and ends around the first bin's end", [(0, cc(0) + d)],
                needs={0: ("absorb_run_ends_at_c",) if d == 0 else (("no_spare", "completes_beyond") if d == 1 else ())} if d >= 0 else {})
    add("last-bin-run-ends@n", "the run ends at n, the last bin's end", [(cc(g.B - 2) + 1, n)], needs={cc(g.B - 2) + 1: ("absorb_run_ends_at_c",)})
    add("last-bin-run-ends@n-1", "the run ends one rank before n", [(cc(g.B - 2) + 1, n - 1)])
    add("long-run-ends@n", "a run from the middle to n: its prefix is completed in the spare bin", [(p0 + 1, n)], ("bin_of_start", "spare_never"), {p0 + 1: ("prefix", "spare_completed")})
    add("long-run-from-rank0", "a run from rank 0 over half the bins, nothing pending: it takes the spare bin", [(0, p0 + 2)], (), {0: ("spare_taken",)})
    # a run that ends around c_count(t) AFTER an earlier run skipped bins: only then is next_avail behind the target, and the run's prefix has a spare bin
    skips = [(L1, gap) for L1 in range(2 * w + 1, 5 * w) for gap in (1, 2, 3)]

    def after_skip(d, needs2):
        cands = []
        for L1, gap in skips:
            en1 = p0 + L1; t = bi(en1); st2 = en1 + gap; en2 = cc(t) + d
            if en2 - st2 >= 2 and bi(en1) == bi(st2):
                cands.append(([(p0, en1), (st2, en2)], {st2: needs2} if needs2 is not None else {}))
        return cands
    found("after-skip-run-ends@c", "bins were skipped, then a run ends exactly on c: absorbed whole; apply_sorted would give its prefix the spare bin",
          after_skip(0, ("absorb_run_ends_at_c",)), ("absorb_strict", "sorted_rule"))
    found("after-skip-run-ends@c+1", "bins were skipped, then a run straddles c by one rank: its prefix is completed in the spare bin",
          after_skip(1, ("prefix", "spare_completed")), ("spare_never",))
    found("after-skip-run-ends@c-1", "bins were skipped, then a run ends one rank before c: absorbed", after_skip(-1, None), ())
    lens = list(range(w + 1, 4 * w + 3))
    # (the bin a run is put in shows in next_avail alone while the run completes either way: a second run behind it, whose prefix finds a spare
    #  bin or not, brings it out)
    taken = [L for L in lens if bi(p0 + L // 2) == k + 1][:3]
    found("spare-taken", "no prefix and the run's middle lies one bin beyond next_avail: the run moves into the spare bin, which the next run's prefix then cannot have",
          [([(p0, p0 + L), (p0 + L + gap, p0 + L + gap + L2)], {p0: ("spare_taken",), p0 + L + gap: ("prefix",)}) for L in taken for gap in (1, 2) for L2 in range(2, 3 * w)], ("spare_never",))
    found("mid-at-next_avail", "no prefix and the run's middle is the last rank of bin next_avail: no spare (one rank further there is one)",
          [([(p0, p0 + L), (p0 + L + gap, p0 + L + gap + L2)], {p0: ("no_spare",), p0 + L + gap: ("prefix",)})
           for L in lens if bi(p0 + L // 2) == k and bi(p0 + (L + 1) // 2) == k + 1 for gap in (1, 2) for L2 in range(2, 3 * w)], ("mid_rounds_up",))
    found("spare-completed", "a prefix is pending and the run's middle lies beyond next_avail: the prefix is completed in the spare bin",
          [([(p0 + gap, p0 + gap + L)], {p0 + gap: ("prefix", "spare_completed")}) for gap in (1, 2, 3) for L in lens], ("spare_never",))
    found("prefix-mid-at-next_avail", "a prefix is pending and the run's middle lies in bin next_avail: the run joins the prefix",
          [([(p0 + gap, p0 + gap + L)], {p0 + gap: ("prefix", "no_spare", "joins_pending")}) for gap in (1, 2, 3) for L in lens], ("spare_always",))
    # completion: the run's end against c_count(b) of the bin it lands in after the spare rule
    comp = [(gap, L) for gap in (0, 1, 2) for L in lens]

    def completes(d):
        def ok(runs):
            s = keys_of(n, runs); _, rep = M.histogram_sorted(s, bl); step = rep.step_of(runs[0][0])
            return step is not None and step[2] == cc(step[3]) + d and ("left_pending" in step[0]) == (d < 0) and ("absorb" not in step[0])
        return [([(p0 + gap, p0 + gap + L)], {}) for gap, L in comp if ok([(p0 + gap, p0 + gap + L)])]
    found("run-completes@c_count(b)", "the run's end equals c_count(b) of the bin it lands in: en >= c_count(b) completes it", completes(0), ("complete_strict",))
    found("run-completes@c_count(b)+1", "the run's end is one past c_count(b): completes", completes(1), ())
    pend = _search(n, bl, [(r, nd, ()) for r, nd in completes(-1)], "left pending")[0]
    out.append(Design("run-left-pending-then-absorb", "the run's end is one short of c_count(b): left pending, the next step absorbs onto it", tuple(pend), (), {pend[0][0]: ("left_pending",)}))
    en1 = pend[0][1]
    # (the follower's middle is at or beyond c_count(b), one bin on: it can only complete the pending run in the spare bin, never join it)
    found("run-left-pending-then-run", "a run left pending is followed at once by another constant run, which completes it in the spare bin",
          [([pend[0], (en1, en1 + L)], {pend[0][0]: ("left_pending",), en1: ("spare_completed",)}) for L in range(2, 4 * w)], ("spare_never",))
    add("two-heavy-back-to-back", "two runs of different values, each straddling a bin end, one behind the other", [(p0 + 1, p0 + w + 3), (p0 + w + 3, p0 + 2 * w + 6)],
        needs={p0 + 1: ("prefix",)})
    kq = g.B // 4; q0 = cc(kq - 1)
    for m in (1, 2, 100 if g.B >= 256 else g.B // 3):
        add(f"run-covers-{m}-bins", f"a run {m} bins long behind a one-rank prefix", [(q0 + 1, q0 + 1 + cc(kq + m - 1) - q0 + 1)], ("bin_of_start",) if m >= 2 else (),
            {q0 + 1: ("prefix",)})
    add("all-equal", "one value: a single run from rank 0 to n", [(0, n)])
    add("two-values", "two values only, 40 % and 60 %", [(0, 2 * n // 5), (2 * n // 5, n)])
    add("all-distinct", "every run has length 1, every bin ends on one: the one-thread-per-bin shortcut", [], ("c_count_floor",) if n % g.B else ())
    return out


PRODUCER_DESIGNS = ("after-skip-run-ends@c-1", "after-skip-run-ends@c", "after-skip-run-ends@c+1", "spare-completed", "spare-taken", "run-completes@c_count(b)",
                    "run-left-pending-then-absorb", "all-distinct")


def design(n, bl, name):
    return next(d for d in designs(n, bl) if d.name == name)


# ------------------------------------------------------------------------------------------------ from ranks to numbers
def ordered(keys, seed, first="median"):
    """The keys in a seeded shuffle with the median (or the minimum) in front."""
    rng = np.random.default_rng([77, seed])
    k = np.array(keys, np.int64)[rng.permutation(len(keys))]
    want = np.sort(k)[len(k) // 2] if first == "median" else k.min()
    i = int(np.flatnonzero(k == want)[0]); k[0], k[i] = k[i], k[0]
    return k


def latents_of(keys, w, step):
    """base + step * key with the middle key on 2^(w-1)."""
    mid = 1 << (w - 1)
    return [(mid + step * (int(x) - len(keys) // 2)) % (1 << w) for x in keys]


def _row(name, about, arr, kw, section, variants=(), pages=None, paging=None, strict=False, gives_up=False, var=1, needs=None):
    return Row(name, about, np.ascontiguousarray(arr), dict(kw), list(pages) if pages is not None else [arr.size], paging, section, tuple(variants), strict, gives_up, var, needs or {})


def design_row(prefix, d, n, dt, step, seed, section, level=8, first="median"):
    k = ordered(keys_of(n, d.runs), seed, first)
    return _row(f"{prefix}-{d.name}", d.about, W.from_latents(latents_of(k, F.width(dt), step), dt), cfg_kw(level), section, d.variants, needs=d.needs)


A_SHAPES = ((4096, np.uint32), (4500, np.int64), (300, np.uint16))     # 256 bins, 256 bins with uneven bin ends, 64 bins


@functools.lru_cache(maxsize=None)
def rows_a():
    rows = []
    for si, (n, dt) in enumerate(A_SHAPES):
        bl = W.unopt_bins_log(8, n)
        for di, d in enumerate(designs(n, bl)):
            rows.append(design_row(f"a-{W.tname(dt)}-n{n}", d, n, dt, 1, si * 100 + di, "a"))
    return rows


B_COUNTS = (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 4099)   # 4099: the first prime above 4096


@functools.lru_cache(maxsize=None)
def rows_b():
    rows = []
    for i, n in enumerate(B_COUNTS):
        bl = W.unopt_bins_log(8, n); B = 1 << bl; g = Geo(n, bl)
        variants = (("shortcut_below_B",) if n < B else ()) + (("c_count_floor",) if n % B and n > B else ())
        k = ordered(keys_of(n, []), 1000 + i)
        rows.append(_row(f"b-uint32-n{n}-all-distinct", f"{n} distinct latents at {B} bins", W.from_latents(latents_of(k, 32, 1), np.uint32), cfg_kw(8), "b", variants))
        if n >= 15:
            c = g.cc(g.k); runs = [(c - 1, c + 1)]
            variants = ("spare_never",) if n >= 255 else ()
            assert _check(n, bl, runs, {}, variants), n
            k = ordered(keys_of(n, runs), 1100 + i)
            rows.append(_row(f"b-uint32-n{n}-one-straddling-run", f"{n} latents at {B} bins, two equal ones on either side of a bin end: no shortcut",
                             W.from_latents(latents_of(k, 32, 1), np.uint32), cfg_kw(8), "b", variants))
    n = 4096; rng = np.random.default_rng(12)
    rows.append(_row("b-uint8-n4096-all-256-values-16-each", "u8, every value 16 times: every run ends exactly on a bin end", rng.permutation(np.repeat(np.arange(256), 16)).astype(np.uint8), cfg_kw(8), "b"))
    x = np.concatenate([np.arange(256), rng.integers(0, 256, n - 256)]); rng.shuffle(x)
    rows.append(_row("b-uint8-n4096-all-256-values-random-counts", "u8, all 256 values with random counts: fewer distinct values than bins' worth of ends, every value a constant run", x.astype(np.uint8), cfg_kw(8), "b"))
    x = (rng.integers(0, 100, n) * 37 - 1800).astype(np.int16)
    rows.append(_row("b-int16-n4096-100-values", "i16, 100 distinct values at 256 bins", x, cfg_kw(8), "b"))
    return rows


# (c) every producer: the tier follows from (numeric range, latents)
TIER_SHAPES = {"direct": (4096, 1, np.uint32), "small": (4096, 2, np.uint32), "mid": (10240, 1, np.int32), "wide": (10240, 2, np.uint32), "select": (10240, 4, np.uint64)}
IMULT_BASE = 200003
FALLBACK_N = 20480


def fallback_array():
    """What makes enc_hist_select_kernel give up: its map is built from a sample of 2048 evenly spaced positions (every 10th here).  Those hold
    distinct values spread evenly over 2^30, so the map is the flat one with buckets 2^17 wide -- and every other position holds one of two
    neighbouring values, 9216 each: one bucket of 18 432 latents with two values in it, beyond what the block orders in LDS."""
    n = FALLBACK_N; rng = np.random.default_rng(31)
    x = np.zeros(n, np.int64)
    sampled = np.arange(2048) * n // 2048
    x[sampled] = rng.permutation(2048) * (1 << 19) + 12345
    rest = np.setdiff1d(np.arange(n), sampled)
    v = 700 * (1 << 19) + 1000
    x[rest] = v + rng.permutation(np.repeat([0, 1], rest.size // 2))
    return (x + (1 << 31) - (1 << 29)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def rows_c():
    rows = []
    for ti, (tier, (n, step, dt)) in enumerate(TIER_SHAPES.items()):
        for di, name in enumerate(PRODUCER_DESIGNS):
            rows.append(design_row(f"c-{tier}-{W.tname(dt)}-n{n}", design(n, 8, name), n, dt, step, 2000 + ti * 50 + di, "c"))
    # the wide tier once more with the minimum in front: the maximum lies beyond the 16-bit window, the chunk is split again at full width
    n, step, dt = TIER_SHAPES["wide"]
    for di, name in enumerate(("after-skip-run-ends@c", "spare-taken", "all-distinct")):
        rows.append(design_row(f"c-wide-full-width-{W.tname(dt)}-n{n}", design(n, 8, name), n, dt, step, 2400 + di, "c", first="min"))
    rows.append(_row("c-select-gives-up-uint32-n20480", "two neighbouring heavy values in one bucket of the select kernel's map: the radix-sort fallback orders the variable",
                     fallback_array(), cfg_kw(8), "c", gives_up=True))
    # a lookback delta: variable 0 holds the lookbacks (one value dominates: counted with aggregation), variable 1 the residuals
    base = np.random.default_rng(40).integers(-(1 << 40), 1 << 40, 365)
    periodic = (base[np.arange(4608) % 365] + np.random.default_rng(4).integers(-3, 4, 4608)).astype(np.int64)
    rows.append(_row("c-lookback-int64-n4608-period365", "lookbacks of a periodic series: one heavy value in variable 0", periodic, dict(mode=1, delta=3, level=8), "c", var=0))
    # int-mult: the secondary's histogram is capped at 64 bins
    n = 4096; bl2 = min(W.unopt_bins_log(8, n), 6)
    for di, name in enumerate(("after-skip-run-ends@c", "spare-completed", "spare-taken", "run-completes@c_count(b)", "all-distinct")):
        d = design(n, bl2, name)
        r = ordered(keys_of(n, d.runs), 2600 + di).tolist()
        m0 = (1 << 63) // IMULT_BASE + 1000
        m = [m0 + int(x) for x in np.random.default_rng([26, di]).integers(-50, 51, n)]
        arr = W.from_latents([mm * IMULT_BASE + 7 + rr for mm, rr in zip(m, r)], np.int64)
        rows.append(_row(f"c-imult-secondary-64-bins-int64-n{n}-{d.name}", d.about, arr, dict(mode=F.MODE_INT_MULT, mode_u64=IMULT_BASE, delta=1, level=8), "c", d.variants, var=2, needs=d.needs))
    return rows


# (d) unstored positions
D_STORED = 4096
D_ORDERS = (1, 2, 7)


def delta_array(dd_full, order, pages, w):
    """Numbers (as latents) whose order-th differences, with zeros in front of every page, are dd_full: what the counting kernels see at EVERY
    position, the first `order` of each page included."""
    mask = (1 << w) - 1; out = []; start = 0
    for pn in pages:
        seg = [int(x) & mask for x in dd_full[start:start + pn]]
        for _ in range(order):
            acc = 0; nxt = []
            for x in seg:
                acc = (acc + x) & mask; nxt.append(acc)
            seg = nxt
        out += seg; start += pn
    return out


@functools.lru_cache(maxsize=None)
def rows_d():
    rows = []; w = 32; mid = 1 << (w - 1)
    heavy_designs = (design(D_STORED, 8, "heavy-mid-ends@c"), design(D_STORED, 8, "after-skip-run-ends@c"))
    for oi, order in enumerate(D_ORDERS):
        for si, (sname, paging, n_pg) in enumerate((("one-page", None, 1), ("exact", "exact", 3), ("equal", "equal", 3))):
            n = D_STORED + order * n_pg
            if paging == "exact": pages = [1400 + order, 1111 + order, n - 2511 - 2 * order]
            elif paging == "equal": pages = LB.equal_pages(n, -(-n // 3))
            else: pages = [n]
            kw = dict(mode=1, delta=2, delta_order=order, level=8)
            if paging == "equal": kw["max_page_n"] = -(-n // 3)
            for ji, junk in enumerate(("heavy", "outside")):
                d = heavy_designs[(oi + si + ji) % 2]
                keys = ordered(keys_of(D_STORED, d.runs), 3000 + oi * 20 + si * 4 + ji).tolist()
                st = d.runs[-1][0]
                dd = []; it = iter(keys)
                for pi, pn in enumerate(pages):
                    for j in range(pn):
                        if j < order: dd.append((st - D_STORED // 2) if junk == "heavy" else ((1 << 30) + 12345 * (pi + 1)) * (1 if (pi + j) % 2 else -1))
                        else: dd.append(next(it) - D_STORED // 2)
                arr = W.from_latents(delta_array(dd, order, pages, w), np.uint32)
                about = d.about + ("; the unstored positions hold the heavy value: counted with them, its run would end past c" if junk == "heavy" else "; the unstored positions hold values far outside [min, max] of the stored ones")
                rows.append(_row(f"d-uint32-o{order}-{sname}-junk-{junk}-{d.name}", about, arr, kw, "d", d.variants, pages=pages, paging=paging, needs=d.needs))
    return rows


# (e) more than 256 bins
def big_row(name, about, n, level, runs, variants=(), seed=0):
    keys = ordered(keys_of(n, runs), 4000 + seed)
    return _row(f"e-uint32-L{level}-n{n}-{name}", about, W.from_latents(latents_of(keys, 32, 3), np.uint32), cfg_kw(level), "e", variants)


@functools.lru_cache(maxsize=None)
def rows_e():
    rows = []; seed = 0
    for n, level in ((1 << 13, 9), (1 << 13, 12), (1 << 16, 12)):
        bl = W.unopt_bins_log(level, n); g = Geo(n, bl); cc = g.cc; B = g.B
        assert B == {(1 << 13, 9): 512, (1 << 13, 12): 1024, (1 << 16, 12): 4096}[(n, level)]
        e = cc(255)                                       # the first rank of window 1
        specs = [("all-distinct", "every window is simple", [], ()),
                 ("run-straddles-window-end", "a run straddles the last bin end of window 0: window 1 is entered off its first rank", [(e - 3, e + 2)], ("window_clean_ignores_pos",)),
                 ("run-ends@window-end", "a run ends exactly on c_count(255): both windows stay simple", [(e - 5, e)], ()),
                 ("pending-across-window-end", "a prefix completed in bin 255 and a run left pending in bin 256, absorbed in window 1", [(e - 3, e + 5)], ()),
                 ("run-from-window0-to-n", "a run from window 0 to n: every later window is skipped", [(cc(100) + 2, n)], ("bin_of_start",))]
        if B >= 1024:
            specs += [("run-skips-one-window", "a run from window 0 into window 2", [(cc(200) + 1, cc(600) + 3)], ("bin_of_start",)),
                      ("walked-between-simple", "one straddling run inside window 1: simple, walked, simple", [(cc(300) - 2, cc(300) + 3)], ("spare_never",)),
                      ("walked-simple-walked", "straddling runs inside windows 0 and 2 only", [(cc(100) - 2, cc(100) + 3), (cc(700) - 2, cc(700) + 3)], ("spare_never",))]
        if B >= 4096:
            specs += [("run-skips-several-windows", "a run from window 0 into window 7", [(cc(100) + 1, cc(2000) + 3)], ("bin_of_start",)),
                      ("runs-in-many-windows", "a straddling run at the end of every second window", [(cc(512 * j + 255) - 3, cc(512 * j + 255) + 2) for j in range(8)], ("window_clean_ignores_pos",))]
        for name, about, runs, variants in specs:
            seed += 1
            rows.append(big_row(name, about, n, level, runs, variants, seed))
    return rows


@functools.lru_cache(maxsize=None)
def rows_f():
    """(f) the no-delta rows of (a) and (b) under PCO_GFX_CFG_STRICT_HISTOGRAM: encode_hist_literal.hip's own builder."""
    return [r._replace(name="f-strict-" + r.name, section="f", strict=True) for r in rows_a() + rows_b()]


def all_rows():
    return rows_a() + rows_b() + rows_c() + rows_d() + rows_e() + rows_f()


@functools.lru_cache(maxsize=None)
def BY_NAME():
    rows = all_rows()
    out = {r.name: r for r in rows}
    assert len(out) == len(rows), "row names repeat"
    return out


def config_key(row):
    return W.config_key(row) + (row.strict,)


# ------------------------------------------------------------------------------------------------ what the model says of a row
Var = collections.namedtuple("Var", "var latents bins_log tier hist_path")


@functools.lru_cache(maxsize=None)
def variables(name):
    """Per present variable of a row: its latents in stored order, its n_bins_log, the counting tier and the hist_path the device must report."""
    r = BY_NAME()[name]
    n = r.arr.size; w = F.width(r.arr.dtype); ubl = W.unopt_bins_log(r.kw.get("level", 8), n); big = ubl > W.kMaxUnoptBinsLog
    p, s = W.ordered_latents(r.arr, r.kw)
    lat = {}
    if r.kw.get("delta") == 3:
        assert len(r.pages) == 1
        lbs = [int(x) for x in O.choose_lookbacks(p, LB.window_log(n), 0)]
        _, deltas = LB.apply_lookbacks([int(x) for x in p], lbs, w, 0)
        lat[0] = np.array(lbs, np.uint32); lat[1] = np.array(deltas, p.dtype); route = "never"
    else:
        d, stored = W.page_differences(p, W.order_of(r.kw), r.pages)
        lat[1] = d[stored]; route = W.analyse(r.arr, r.kw, r.pages).route
    if s is not None: lat[2] = s
    out = []
    for v, x in sorted(lat.items()):
        bl = min(ubl, 6) if v == 2 else ubl
        rng_ = int(x.max()) - int(x.min()) if x.size else 0
        tier = "select" if big else W.tier_of(rng_, x.size)
        if big: path = 1
        elif r.gives_up and v == r.var: path = 2
        elif tier == "small": path = 0 if route == "c16" and v != 0 else 1
        else: path = 1 if tier == "select" else 0
        out.append(Var(v, x, bl, tier, path))
    return tuple(out), route


@functools.lru_cache(maxsize=None)
def model_of(name, var):
    v = next(x for x in variables(name)[0] if x.var == var)
    return M.histogram(v.latents, v.bins_log)


def producer_of(row, v):
    """Which implementation produces the rank records of variable v of `row`."""
    if row.strict: return "literal"
    if W.unopt_bins_log(row.kw.get("level", 8), row.arr.size) > W.kMaxUnoptBinsLog: return "big"
    return "sort-fallback" if v.hist_path == 2 else v.tier
