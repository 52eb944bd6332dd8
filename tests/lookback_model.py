"""The lookback search (delta/lookback.rs:22-185) as a PLAIN MODEL, the prediction of which device kernel decides a page, and the rows that
put a chosen lookback, a count or a table entry exactly on a threshold of those kernels.  Shared by tests/test_lookback_edges.py
(-m "not gpu") and tests/test_gpu_lookback_edges.py (-m gpu).

The model is Python integers masked to the latent width and shares no code with oracle/ or the library:

  * choose_lookbacks: sixteen proposals per element -- brute force 0..5, repeating 6..9, hashed 10..15 --, buckets and their neighbours in
    64 bits, the multiplicative hash with the two xor-shifts, strict > (the first maximum wins), counts from 1;
  * apply_lookbacks / undo_lookbacks: the delta itself and its inverse;
  * call_shape / page_route: what the host and the kernels decide from sizes alone -- the pipeline instantiation and the one-wave layout of a
    call, and per page the screen (enc_lookback_seq_kernel), the hand-back (enc_lookback_kernel) or the pipeline;
  * Log: per page, how often each lookback was chosen and at which lanes, every count that crossed a power of two (position, lane, lookback,
    proposal group) and every decision in which two groups tied on goodness and proposal order decided.

Every constant is read from the .hip sources and pco_gfx_encode_api.inc, so a moved threshold fails tests/test_lookback_edges.py instead of
silently moving the rows.

Rows are an OPENING that selects the route (quiet: a short period; noisy: substitutions a[j] = a[j - q] in one tile, each of which costs two
changes of the lookback; narrow: all values inside 4 n - 1) and a BODY that carries the edge (a long period P of wide random values plus noise
in the low two bits: from one period into the body on, the chosen lookback is P at every lane)."""
import collections
import functools
import os
import re

import numpy as np

import latent_window_util as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcodec_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (what, found)
    return found.pop()


_P, _K, _A = _read("encode_lookback.hip"), _read("encode_kernels.hip"), _read("pco_gfx_encode_api.inc")
kRing = dict(zip(("small", "large"), map(int, _one(r"\bkRing\s*=\s*kSmall\s*\?\s*(\d+)u\s*:\s*(\d+)u\s*;", _P, "kRing"))))
kCounts = dict(zip(("small", "large"), map(int, _one(r"\bkCounts\s*=\s*kSmall\s*\?\s*(\d+)u\s*:\s*(\d+)u\s*;", _P, "kCounts"))))
kFront = int(_one(r"\bkFront\s*=\s*(\d+)\s*;", _P, "kFront"))
kWaves = kFront + int(_one(r"\bkWaves\s*=\s*kFront\s*\+\s*(\d+)\s*,", _P, "kWaves"))
_one(r"\b(kNear\s*=\s*kRing\s*-\s*64\s*\*\s*kWaves)\s*;", _P, "kNear's formula")
kNear = {k: v - 64 * kWaves for k, v in kRing.items()}
kLbPipeSmallMaxPage = int(_one(r"\bkLbPipeSmallMaxPage\s*=\s*(\d+)\s*;", _P, "kLbPipeSmallMaxPage"))
kLbSweepPeriod = 1 << int(_one(r"\bkLbSweepPeriod\s*=\s*1u\s*<<\s*(\d+)\s*;", _P, "kLbSweepPeriod"))
kLbSeqTiles, kLbAbortWindow, kLbAbortRounds = map(int, _one(r"\bkLbSeqTiles\s*=\s*(\d+)\s*,\s*kLbAbortWindow\s*=\s*(\d+)\s*,\s*kLbAbortRounds\s*=\s*(\d+)\s*;", _P, "the abort constants"))
_one(r"(d_rounds\s*>\s*kLbAbortRounds\s*&&\s*ts\s*<\s*kLbSeqTiles\s*\+\s*kLbAbortWindow\s*&&\s*n_tiles\s*>\s*4\s*\*\s*\(kLbSeqTiles\s*\+\s*kLbAbortWindow\))", _P, "the abort condition")
kScreenSpan = int(_one(r"screened\s*=\s*hi\s*-\s*lo\s*<\s*(\d+)ull\s*\*\s*n\s*;", _P, "the screen"))
kLbSeqMaxPage = int(_one(r"\bkLbSeqMaxPage\s*=\s*(\d+)\s*;", _P, "kLbSeqMaxPage"))
kLhWorkers, kLhChunk = int(_one(r"\bkLhWorkers\s*=\s*(\d+)\s*,", _P, "kLhWorkers")), int(_one(r"\bkLhChunk\s*=\s*(\d+)\s*;", _P, "kLhChunk"))
kLbCountsLds, kLbRing = {}, {}
for _name in ("LbFull", "LbSmall"):
    _c, _r = _one(r"typedef\s+LbCfg<(\d+),\s*(\d+)>\s+%s\s*;" % _name, _K, _name)
    kLbCountsLds[_name], kLbRing[_name] = int(_c), int(_r)
_one(r"(lb\s*<\s*kLbRing\s*-\s*64\s*\?)", _K, "the one-wave kernel's ring threshold")
kLbNear = {k: v - 64 for k, v in kLbRing.items()}
kLbSmallMaxPage = int(_one(r"\bkLbSmallMaxPage\s*=\s*(\d+)\s*;", _K, "kLbSmallMaxPage"))
kSmallWmax = int(_one(r"small\s*=\s*page_max\s*<=\s*kLbPipeSmallMaxPage\s*&&\s*wmax\s*<=\s*(\d+)\s*;", _A, "the small pipeline's window"))

PIPE_KERNEL = {"small": "enc_lookback_pipe_kernel<small,props,fastd>", "large": "enc_lookback_pipe_kernel<props,fastd>"}
ONEWAVE_KERNEL = {"LbSmall": "enc_lookback_kernel<small>", "LbFull": "enc_lookback_kernel"}
for _k in list(PIPE_KERNEL.values()) + list(ONEWAVE_KERNEL.values()):
    assert '"%s"' % _k in _A, _k
ROUTES = ("pipe", "seq", "back")          # pco_gfx_debug_lookback_routes: 0, 1, 2
BRUTE, REPEATING, PROPOSED = 6, 4, 16
GROUPS = ("brute", "repeating", "hashed")

# ------------------------------------------------------------------------------------------------ the search
_M64 = (1 << 64) - 1
_MUL = 11400714819323197441


def hash_fn(x, mask):
    x &= _M64
    x = ((x ^ (x >> 32)) * _MUL) & _M64
    return (x ^ (x >> 32)) & mask


def window_log(n):
    """delta/mod.rs:37-48: the window of a chunk of n numbers."""
    return min(max((n - 1).bit_length(), 4), 15)


def group_of(slot):
    return GROUPS[0 if slot < BRUTE else 1 if slot < BRUTE + REPEATING else 2]


class Log:
    """What happened on a page: chosen[lb] = times; lanes[lb] = set of (i - state_n) % 64 it was chosen at; crossings = (i, lane, lb, new
    count, group of the winning slot); ties = (i, winning group, losing group)."""

    def __init__(self):
        self.chosen = collections.Counter(); self.lanes = collections.defaultdict(set); self.crossings = []; self.ties = []


def choose_lookbacks(latents, bits, window_n_log, state_n_log=0, log=None, hashed=None):
    """The lookbacks of positions state_n .. n - 1.  log: a Log to fill; hashed: a list that receives the six hashed proposals of every position."""
    mask = (1 << bits) - 1
    lat = [int(x) & mask for x in latents]
    n = len(lat); state_n = 1 << state_n_log
    if n <= state_n:
        return []
    hash_table_n = 1 << (window_n_log + 1); hmask = hash_table_n - 1; window_n = 1 << window_n_log
    assert window_n >= PROPOSED
    counts = [1] * min(window_n, n)
    tables = ([0] * hash_table_n, [0] * hash_table_n)
    proposed = [min(k + 1, state_n) for k in range(PROPOSED)]
    best, rep_idx, out = 1, 0, []
    for i in range(state_n, n):
        l = lat[i]
        nb = min(i, PROPOSED)
        proposed[nb - 1] = nb
        slot = BRUTE + REPEATING
        for tbl, coarse in zip(tables, (0, 8)):
            bucket = l >> coarse                                   # (a 64-bit value: its neighbours wrap at 2^64, whatever the latent's width)
            h1 = hash_fn(bucket, hmask)
            for h in (hash_fn(bucket - 1, hmask), h1, hash_fn(bucket + 1, hmask)):
                lb = i - tbl[h]
                proposed[slot] = lb if lb <= window_n else min(slot, i)
                slot += 1
            tbl[h1] = i
        if hashed is not None: hashed.append(tuple(proposed[BRUTE + REPEATING:]))
        best_g, new_best, win = 0, 0, -1
        gs = []
        for s, lb in enumerate(proposed):
            o = lat[i - lb]
            d = min((l - o) & mask, (o - l) & mask)
            g = counts[lb - 1].bit_length() + bits - d.bit_length()
            gs.append(g)
            if g > best_g:
                best_g, new_best, win = g, lb, s
        if log is not None:   # two groups tied on goodness with different lookbacks: proposal order decided
            for s in range(win + 1, PROPOSED):
                if gs[s] == best_g and proposed[s] != new_best and group_of(s) != group_of(win):
                    log.ties.append((i, group_of(win), group_of(s))); break
        if new_best != best:
            rep_idx += 1
        proposed[BRUTE + rep_idx % REPEATING] = new_best
        best = new_best
        out.append(best)
        counts[best - 1] += 1
        if log is not None:
            lane = (i - state_n) % 64
            log.chosen[best] += 1; log.lanes[best].add(lane)
            c = counts[best - 1]
            if c & (c - 1) == 0:
                log.crossings.append((i, lane, best, c, group_of(win)))
    return out


def apply_lookbacks(latents, lbs, bits, state_n_log=0):
    """lookback.rs:166-185: (delta state, the page's deltas with the centre toggled; the first state_n positions hold no delta)."""
    mask = (1 << bits) - 1; mid = 1 << (bits - 1); state_n = 1 << state_n_log
    lat = [int(x) & mask for x in latents]
    real = min(len(lat), state_n)
    out = [(lat[i] - lat[i - lbs[i - state_n]] + mid) & mask for i in range(real, len(lat))]
    return [0] * (state_n - real) + lat[:real], out


def undo_lookbacks(state, deltas, lbs, bits):
    mask = (1 << bits) - 1; mid = 1 << (bits - 1)
    lat = list(state)
    for d, lb in zip(deltas, lbs):
        lat.append((d - mid + lat[len(lat) - lb]) & mask)
    return lat


# ------------------------------------------------------------------------------------------------ the routes
def call_shape(chunk_ns, page_ns):
    """(pipeline instantiation, one-wave layout) of a call from its lookback chunks' sizes and ALL its pages' sizes."""
    page_max = max(page_ns); wmax = max(window_log(n) for n in chunk_ns)
    return ("small" if page_max <= kLbPipeSmallMaxPage and wmax <= kSmallWmax else "large"), ("LbSmall" if page_max <= kLbSmallMaxPage else "LbFull")


def tile_rounds(lbs, state_n=1):
    """Rounds stage D needs per tile of 64 positions from state_n: one more than the positions whose lookback differs from the position before
    (the running lookback starts at 1), or as many when the last of them is the tile's last lane."""
    out = []; prev = 1
    for t0 in range(0, len(lbs), 64):
        tile = lbs[t0:t0 + 64]; m = 0; last = -1
        for e, lb in enumerate(tile):
            if lb != prev: m += 1; last = e
            prev = lb
        out.append(m if m and last == len(tile) - 1 else m + 1)
    return out


def page_route(lat, lbs, state_n=1):
    n = len(lat)
    if n <= kLbPipeSmallMaxPage and max(lat) - min(lat) < kScreenSpan * n:
        return "seq"
    rounds = tile_rounds(lbs, state_n)
    if len(rounds) > 4 * (kLbSeqTiles + kLbAbortWindow) and any(r > kLbAbortRounds for r in rounds[kLbSeqTiles:kLbSeqTiles + kLbAbortWindow]):
        return "back"
    return "pipe"


def u16_table_proposals(lat, window_n_log, sweep=True):
    """The hashed proposals of a page as the pre-pass keeps them: positions mod 2^16, swept at the first step boundary (kLhWorkers tiles) behind
    every multiple of kLbSweepPeriod.  Returns the six proposal streams; with sweep=False, what a table without the sweep would say.  (CPU only:
    it shows that the sweep makes the u16 table exact, and which rows tell a table without it apart.)"""
    n = len(lat); hash_table_n = 2 << window_n_log; hmask = hash_table_n - 1; window_n = 1 << window_n_log
    tables = ([0] * hash_table_n, [0] * hash_table_n)
    out = [[1] * n for _ in range(6)]
    next_sweep = kLbSweepPeriod
    for i in range(1, n):
        if (i - 1) % (64 * kLhWorkers) == 0 and i >= next_sweep:
            if sweep:
                T = i & 0xffff; marker = (i - window_n - 1) & 0xffff
                for tbl in tables:
                    for v, e in enumerate(tbl):
                        if ((T - e) & 0xffff) > window_n: tbl[v] = marker
            next_sweep += kLbSweepPeriod
        slot = 0
        for tbl, coarse in zip(tables, (0, 8)):
            bucket = lat[i] >> coarse
            h1 = hash_fn(bucket, hmask)
            for h in (hash_fn(bucket - 1, hmask), h1, hash_fn(bucket + 1, hmask)):
                lb = (i - tbl[h]) & 0xffff
                out[slot][i] = lb if lb <= window_n else min(10 + slot, i)
                slot += 1
            tbl[h1] = i & 0xffff
    return out


# ------------------------------------------------------------------------------------------------ rows
Row = collections.namedtuple("Row", "name arr kw pages paging routes shape claims body")
# routes: per page; shape: the (pipeline, one-wave layout) of the call the row is built for; claims: what the event log must show --
# ("lb", page, L): lookback L chosen >= 64 times on that page at every lane; ("at", page, i, L): position i chose L; ("not", page, i, L);
# ("rounds", page, tile, R): stage D's rounds of that tile
LOOKBACK = dict(mode=1, delta=3)
T0 = 18                                   # the body starts with tile T0: behind the abort window
BODY_START = 1 + 64 * T0
Q0, QS, QS2 = 53, 17, 19                  # the opening's period, and the distances of a substitution


def wide(rng, k, w):
    """k wide random latents in the middle half of the type."""
    lo = 1 << (w - 2)
    return [lo + int(x) % (2 * lo) for x in rng.integers(0, 1 << 62, k)] if w > 16 else [int(x) for x in rng.integers(0, 1 << w, k)]


def opening(rng, w, rounds=None, tile=None, base=None):
    """BODY_START latents of period Q0 with noise in the low two bits.  rounds / tile: substitutions in that tile -- a[j] = a[j - QS] at every
    second lane from lane 2, kept in every later period so that nothing echoes -- which make stage D need exactly `rounds` rounds there:
    23 = 11 substitutions, 25 = 12, 24 = 10 and two neighbours at distances QS and QS2 (three changes)."""
    base = wide(rng, Q0, w) if base is None else base
    a = [(base[i % Q0] & ~3) + int(x) for i, x in enumerate(rng.integers(0, 4, BODY_START))]
    if rounds is not None:
        j0 = 1 + 64 * tile + 2
        subs = {23: [(j0 + 2 * m, QS) for m in range(11)], 25: [(j0 + 2 * m, QS) for m in range(12)],
                24: [(j0 + 2 * m, QS) for m in range(10)] + [(j0 + 30, QS), (j0 + 31, QS2)]}[rounds]
        for j, q in subs:
            v = a[j - q]
            for i in range(j, BODY_START, Q0): a[i] = v
    return a


def extend(rng, a, n):
    """`a` continued to n latents at the opening's period (compressible filler: a chunk of wide random numbers under a lookback delta is larger
    than its size guarantee, and the reference then writes it without any delta)."""
    a = list(a)
    for x in rng.integers(0, 4, max(n - len(a), 0)): a.append((a[len(a) - Q0] & ~3) + int(x))
    return a


def body(rng, w, P, n_body):
    base = wide(rng, P, w)
    return [(base[i % P] & ~3) + int(x) for i, x in enumerate(rng.integers(0, 4, n_body))]


def threshold_periods():
    """route -> the periods one step either side of each threshold of that route."""
    def around(x): return (x - 1, x, x + 1)
    return {("pipe", "small"): around(kNear["small"]),
            ("pipe", "large"): around(kNear["large"]) + around(kCounts["large"] + 1),
            ("back", "LbFull"): around(kLbNear["LbFull"]) + around(kLbCountsLds["LbFull"] + 1),
            ("back", "LbSmall"): around(kLbNear["LbSmall"]) + around(kLbCountsLds["LbSmall"] + 1)}


TYPES_ALL = {64: (np.uint64, np.int64, np.float64), 32: (np.uint32, np.int32, np.float32)}


def _mk(name, lat, dt, routes, shape, claims, body_, pages=None, paging=None, kw=None):
    arr = W.from_latents(lat, dt)
    return Row(name, arr, dict(kw or LOOKBACK), list(pages) if pages else [arr.size], paging, list(routes), shape, list(claims), body_)


@functools.lru_cache(maxsize=None)
def rows_thresholds():
    """(1) and (8): every threshold period on its route, behind a quiet opening (pipeline) or a noisy one of 25 rounds in tile 8 (one-wave),
    and the hand-back edge itself: 23, 24 and 25 rounds in tile 8, 15 and 16, pages of 4097 and 4098 numbers."""
    rows = []
    for w in (64, 32):
        dt = TYPES_ALL[w][0]
        for (route, kind), periods in threshold_periods().items():
            for P in periods:
                rng = np.random.default_rng([1, w, P, route == "back"])
                noisy = dict(rounds=25, tile=kLbSeqTiles) if route == "back" else {}
                n_body = max(P + 64 * 5, (4200 - BODY_START) if route == "back" else 0)   # (the hand-back needs more than 64 tiles)
                lat = opening(rng, w, **noisy) + body(rng, w, P, n_body)
                shape = ("small", "LbSmall") if kind in ("small", "LbSmall") else ("large", "LbFull")
                claims = [("lb", 0, P)]
                if kind == "LbFull" and P > kLbCountsLds["LbFull"]: claims.append(("big", 0, P))   # a far count crosses a power of two inside one tile's big[] list
                rows.append(_mk(f"t-u{w}-{route}-{kind}-P{P}", lat, dt, [route], shape, claims, "threshold"))
    return rows


def _quiet_then(rng, w, tail, first=None, noisy=False):
    """A quiet opening -- or a noisy one of kLbAbortRounds + 1 rounds in the first tile of the abort window -- (whose element 0 is `first`, a
    value of its own, when given) and `tail` behind it."""
    a = opening(rng, w, **(dict(rounds=kLbAbortRounds + 1, tile=kLbSeqTiles) if noisy else {}))
    if first is not None: a[0] = first
    return a + list(tail)


@functools.lru_cache(maxsize=None)
def rows_handback():
    """(8) 23, 24 and 25 rounds in tile 8 only, tile 15 only and tile 16 only, on pages of 4097 (64 tiles: never handed back) and 4098 numbers;
    the body is the small pipeline's ring threshold, or the small one-wave layout's count threshold where the page is handed back."""
    rows = []
    for w in (64, 32):
        for n in (4097, 4098):
            for tile in (kLbSeqTiles, kLbSeqTiles + kLbAbortWindow - 1, kLbSeqTiles + kLbAbortWindow):
                for R in (kLbAbortRounds - 1, kLbAbortRounds, kLbAbortRounds + 1):
                    back = R > kLbAbortRounds and tile < kLbSeqTiles + kLbAbortWindow and n >= 4098
                    P = kLbCountsLds["LbSmall"] + 1 if back else kNear["small"]
                    rng = np.random.default_rng([8, w, n, tile, R])
                    lat = opening(rng, w, rounds=R, tile=tile) + body(rng, w, P, n - BODY_START)
                    rows.append(_mk(f"b-u{w}-n{n}-tile{tile}-rounds{R}-P{P}-{'back' if back else 'pipe'}", lat, TYPES_ALL[w][0], ["back" if back else "pipe"],
                                    ("small", "LbSmall"), [("rounds", 0, tile, R), ("lb", 0, P)], "handback"))
    return rows


WINDOW15 = 1 << 15


@functools.lru_cache(maxsize=None)
def rows_window():
    """(2) the first occurrence of element 0's value at window_n - 1, window_n and window_n + 1 (the hash entry is the untouched 0), a value that
    returns after exactly window_n and window_n + 1, behind a quiet opening (pipeline) and behind a noisy one (handed back); pages
    of window_n numbers at window_n_log 13 and 14; wrapped chunks whose pages are shorter than the window."""
    rows = []
    for w in (64, 32):
        dt = TYPES_ALL[w][0]
        for quiet in (True, False):
            for i in (WINDOW15 - 1, WINDOW15, WINDOW15 + 1):
                rng = np.random.default_rng([2, w, quiet, i])
                n = WINDOW15 + 2400
                v0, u1, u2 = wide(rng, 3, w)
                lat = extend(rng, _quiet_then(rng, w, [], first=v0, noisy=not quiet), n)
                lat[i] = v0
                claims = [("at", 0, i, i)] if i <= WINDOW15 else [("not", 0, i, i)]
                if i == WINDOW15:   # ... and two returns beside it
                    lat[2000] = u1; lat[2000 + WINDOW15] = u1; lat[2100] = u2; lat[2100 + WINDOW15 + 1] = u2
                    claims += [("at", 0, 2000 + WINDOW15, WINDOW15), ("not", 0, 2100 + WINDOW15 + 1, WINDOW15 + 1)]
                route = "pipe" if quiet else "back"
                rows.append(_mk(f"w-u{w}-wlog15-first@{i}-{'quiet' if quiet else 'noisy'}-{route}", lat, dt, [route], ("large", "LbFull"), claims, "window"))
        for wlog in (13, 14):   # (a page longer than window_n has the next window: window_n and window_n + 1 cannot be reached below 15)
            n = 1 << wlog; rng = np.random.default_rng([2, w, wlog]); v0 = wide(rng, 1, w)[0]
            lat = _quiet_then(rng, w, wide(rng, n - BODY_START, w), first=v0); lat[n - 1] = v0
            rows.append(_mk(f"w-u{w}-wlog{wlog}-first@{n - 1}-quiet-pipe", lat, dt, ["pipe"], ("small", "LbSmall") if wlog == 13 else ("large", "LbFull"), [("at", 0, n - 1, n - 1)], "window"))
        # pages shorter than the window: the counts have min(window_n, n) entries and the last position of every page reaches back to its first
        for paging, pages, extra in (("exact", [5000, 8192, 8193, 11385], {}), ("equal", equal_pages(WINDOW15 + 2, 4098), dict(max_page_n=4098))):
            assert sum(pages) >= WINDOW15 + 1
            rng = np.random.default_rng([2, w, len(pages)]); lat = []; claims = []
            for pi, pn in enumerate(pages):
                v0 = wide(rng, 1, w)[0]
                pg = _quiet_then(rng, w, wide(rng, pn - BODY_START, w), first=v0); pg[pn - 1] = v0
                lat += pg; claims.append(("at", pi, pn - 1, pn - 1))
            rows.append(_mk(f"w-u{w}-wlog15-{paging}{pages[0]}-last-is-first-pipe", lat, dt, ["pipe"] * len(pages), ("large", "LbFull" if max(pages) > kLbSmallMaxPage else "LbSmall"),
                            claims, "window", pages=pages, paging=paging, kw=dict(LOOKBACK, **extra)))
    return rows


def equal_pages(n, max_page_n):
    """PagingSpec::EqualPagesUpTo"""
    k = -(-n // max_page_n); lo, r = divmod(n, k)
    return [lo + 1] * r + [lo] * (k - r)


def sweep_positions(n):
    """Where the pre-pass sweeps its tables: the first step boundary (kLhWorkers tiles) at or behind every multiple of kLbSweepPeriod."""
    out = []; nxt = kLbSweepPeriod
    for p2 in range(1, n, 64 * kLhWorkers):
        if p2 >= nxt: out.append(p2); nxt += kLbSweepPeriod
    return out


N17 = 1 << 17
ALIAS_D = (0, 1, 5, 100, WINDOW15)


@functools.lru_cache(maxsize=None)
def rows_sweep():
    """(3) one page of 2^17 per width, lookback Q0 throughout, with values of their own planted so that they return after 65536 + d positions (the
    u16 age would say d; for d = 100 and window_n the position d back holds a near value, so a device that believed the alias would choose
    it), after exactly window_n and window_n + 1 with the earlier occurrence around a multiple of kLbSweepPeriod, and with an entry that is
    exactly window_n and window_n + 1 old at the moment of a sweep."""
    rows = []
    for w in (64, 32):
        rng = np.random.default_rng([3, w])
        base = wide(rng, Q0, w)
        lat = [(base[i % Q0] & ~3) + int(x) for i, x in enumerate(rng.integers(0, 4, N17))]
        own = iter(wide(rng, 64, w)); claims = []
        for k, d in enumerate(ALIAS_D):
            p = 3001 + 2003 * k; i = p + 65536 + d; x = next(own)
            lat[p] = x; lat[i] = x
            if d >= 100: lat[i - d] = x + 4103
            if d: claims.append(("not", 0, i, d))
        for k, q in enumerate((kLbSweepPeriod - 1, kLbSweepPeriod, kLbSweepPeriod + 1, 2 * kLbSweepPeriod - 1, 2 * kLbSweepPeriod, 2 * kLbSweepPeriod + 1)):
            y = next(own); lat[q] = y; lat[q + WINDOW15] = y; claims.append(("at", 0, q + WINDOW15, WINDOW15))
            z = next(own); lat[q + 300 + k] = z; lat[q + 300 + k + WINDOW15 + 1] = z; claims.append(("not", 0, q + 300 + k + WINDOW15 + 1, WINDOW15 + 1))
        T = [t for t in sweep_positions(N17) if t > WINDOW15 + 2000][1]
        for off, lb_ok in ((0, True), (7, True), (3, False)):   # at the sweep: window_n old (kept) twice, window_n + 1 old (rewritten, and still too old)
            y = next(own); back = WINDOW15 if lb_ok else WINDOW15 + 1
            lat[T + off - back] = y; lat[T + off] = y
            claims.append(("at", 0, T + off, WINDOW15) if lb_ok else ("not", 0, T + off, WINDOW15 + 1))
        rows.append(_mk(f"a-u{w}-n{N17}-alias-and-sweep-pipe", lat, TYPES_ALL[w][0], ["pipe"], ("large", "LbFull"), claims, "sweep"))
    return rows


BUCKET_TYPES = {8: (np.uint8, np.int8), 16: (np.uint16, np.int16, np.float16), 32: (np.uint32, np.int32, np.float32), 64: (np.uint64, np.int64, np.float64)}


def holds(lat, bits, claims):
    """Whether the model's lookbacks of one page bear out its ("at" | "not", 0, i, L) claims."""
    lbs = choose_lookbacks(lat, bits, window_log(len(lat)))
    return all((lbs[c[2] - 1] == c[3]) == (c[0] == "at") for c in claims)


@functools.lru_cache(maxsize=None)
def rows_bucket():
    """(4) 0 after Lmax and Lmax after 0, 900 positions apart: bucket - 1 and bucket + 1 are 64-bit values, so only 64-bit latents link them
    (lookback 900); the coarse table never does (0 - 1 is 2^64 - 1, not the all-ones bucket of 56 bits); x, x + 1, x + 2 in neighbouring lanes.
    8-bit pages are screened; the wider ones come behind a quiet opening (pipeline) and a noisy one (handed back).  The seed is searched until
    no other element has overwritten the table entry in between (a table of 2 << window_n_log entries is small)."""
    rows = []
    for w, types in BUCKET_TYPES.items():
        lmax = (1 << w) - 1
        for ti, dt in enumerate(types):
            for first, second, tag in ((lmax, 0, "0-after-max"), (0, lmax, "max-after-0"), (lmax - 100, 200, "coarse-low-after-ones"), (200, lmax - 100, "coarse-ones-after-low")):
                for route in (("seq",) if w == 8 else ("pipe", "back")):
                    links = w == 64 and tag in ("0-after-max", "max-after-0")
                    for attempt in range(64):
                        rng = np.random.default_rng([4, w, ti, first & 0xffff, route == "back", attempt])
                        if w == 8: lat = extend(rng, [int(x) & ~3 for x in rng.integers(64, 192, Q0)], 1300); s0 = 0      # (the middle half: no bucket near either end)
                        else:
                            s0 = BODY_START
                            tail = wide(rng, 3047 if route == "back" else 1300, w) if w > 16 else [int(x) for x in rng.integers(1 << 14, 3 << 14, 3047 if route == "back" else 1300)]
                            lat = _quiet_then(rng, w, tail, noisy=route == "back")
                        lat[s0 + 100] = first; lat[s0 + 1000] = second
                        claims = [("at", 0, s0 + 1000, 900) if links else ("not", 0, s0 + 1000, 900)]
                        if w >= 32:   # a lane's side slot is an earlier lane's centre slot of the same tile
                            x = lat[s0 + 500] & ~7
                            lat[s0 + 1100:s0 + 1103] = [x, x + 1, x + 2]; lat[s0 + 1164:s0 + 1167] = [x + 2, x + 1, x]
                            claims += [("at", 0, s0 + 1101, 1), ("at", 0, s0 + 1102, 1), ("at", 0, s0 + 1165, 1), ("at", 0, s0 + 1166, 1)]
                        if holds(lat, w, claims): break
                    else:
                        raise AssertionError((w, dt, tag, route))
                    rows.append(_mk(f"k-{W.tname(dt)}-{tag}-{'linked' if links else 'apart'}-{route}", lat, dt, [route], ("small", "LbSmall"), claims, "bucket"))
    return rows


def colliding_buckets(rng, w, wlog, k):
    """k pairs of distinct wide fine buckets with equal hash in a table of 2 << wlog entries, found by search."""
    hmask = (2 << wlog) - 1; seen = {}; out = []
    while len(out) < k:
        v = wide(rng, 1, w)[0]; h = hash_fn(v, hmask)
        if h in seen and seen[h] >> 9 != v >> 9: out.append((seen.pop(h), v))
        else: seen[h] = v
    return out


@functools.lru_cache(maxsize=None)
def rows_hazard():
    """(5) distinct buckets with equal hash in one tile, in neighbouring tiles, across the pre-pass's 15-tile step and 5-tile chunk boundaries;
    one value at many lanes of a tile (only the last may write) and a hit at lane 63 that feeds the next tile."""
    rows = []
    for w in (64, 32):
        n = 4000; rng = np.random.default_rng([5, w]); wlog = window_log(n)
        lat = _quiet_then(rng, w, wide(rng, n - BODY_START, w))
        pairs = colliding_buckets(rng, w, wlog, 4)
        def pos(tile, lane): return 1 + 64 * tile + lane
        spots = [((20, 5), (20, 40), (20, 50)), ((22, 60), (23, 2), (23, 9)), ((29, 61), (30, 1), (30, 6)), ((34, 62), (35, 0), (35, 3))]   # tiles 29|30: a step; 34|35: a chunk
        claims = []
        for (v1, v2), (a, b, c) in zip(pairs, spots):
            lat[pos(*a)] = v1; lat[pos(*b)] = v2; lat[pos(*c)] = v1     # v1 again: its fine entry now names v2's position; the coarse table still finds it
            claims.append(("at", 0, pos(*c), pos(*c) - pos(*a)))
        v = wide(rng, 1, w)[0]
        for lane in (3, 20, 41, 63): lat[pos(40, lane)] = v
        lat[pos(41, 7)] = v
        claims += [("at", 0, pos(40, 20), 17), ("at", 0, pos(40, 41), 21), ("at", 0, pos(40, 63), 22), ("at", 0, pos(41, 7), 8)]
        v = wide(rng, 1, w)[0]   # written at lane 63, read at lane 0 of the next tile: the shortest way from the sequencer's write to a read
        lat[pos(44, 30)] = v; lat[pos(44, 63)] = v; lat[pos(45, 0)] = v; lat[pos(45, 9)] = v
        claims += [("at", 0, pos(44, 63), 33), ("at", 0, pos(45, 0), 1), ("at", 0, pos(45, 9), 9)]
        rows.append(_mk(f"h-u{w}-n{n}-collisions-and-repeats-pipe", lat, TYPES_ALL[w][0], ["pipe"], ("small", "LbSmall"), claims, "hazard"))
    return rows


CROSS_LANES = (0, 31, 63)


CROSS_KINDS = (("brute", 3, ("small", "LbSmall")), ("near", 100, ("small", "LbSmall")), ("far", kCounts["large"] + 104, ("large", "LbFull")))
CROSS_TOP = 4096
# the first crossings after a lookback is first chosen.  Behind the period-53 opening a brute-force lookback has made its first ones already (a
# page's first sixteen positions propose nothing but 1 .. 16, and random latents let each of them win a few times); behind a CONSTANT opening
# lookback 1 wins every position, the count of lookback 6 is still 1 when the body starts, and 2, 4 and 8 can be placed like the others
CROSS_FIRST = {"brute": (6, (2, 4, 8, 16, 32)), "near": (100, (2, 4, 8, 16, 32)), "far": (kCounts["large"] + 104, (2, 4, 8, 16, 32))}


# (width, P, lane, first count) -> (seed attempt, pad): found by search_crossing
CROSSING_PADS = {
    (64, 3, 0, 64): (2, 0), (64, 6, 0, 16): (0, 44), (64, 6, 0, 32): (0, 28), (64, 3, 31, 64): (1, 34), (64, 6, 31, 16): (0, 11), (64, 6, 31, 32): (0, 59),
    (64, 3, 63, 64): (0, 1), (64, 6, 63, 16): (0, 43), (64, 6, 63, 32): (0, 27), (64, 100, 0, 64): (0, 30), (64, 100, 0, 2): (0, 28), (64, 100, 0, 4): (0, 26),
    (64, 100, 0, 8): (0, 22), (64, 100, 0, 16): (0, 14), (64, 100, 0, 32): (0, 62), (64, 100, 31, 64): (0, 61), (64, 100, 31, 2): (0, 59), (64, 100, 31, 4): (0, 57),
    (64, 100, 31, 8): (0, 53), (64, 100, 31, 16): (0, 45), (64, 100, 31, 32): (0, 29), (64, 100, 63, 64): (0, 29), (64, 100, 63, 2): (0, 27), (64, 100, 63, 4): (0, 25),
    (64, 100, 63, 8): (0, 21), (64, 100, 63, 16): (0, 13), (64, 100, 63, 32): (0, 61), (64, 4200, 0, 64): (0, 26), (64, 4200, 0, 2): (0, 24), (64, 4200, 0, 4): (2, 22),
    (64, 4200, 0, 8): (0, 18), (64, 4200, 0, 16): (0, 10), (64, 4200, 0, 32): (0, 58), (64, 4200, 31, 64): (0, 57), (64, 4200, 31, 2): (0, 55), (64, 4200, 31, 4): (0, 53),
    (64, 4200, 31, 8): (0, 49), (64, 4200, 31, 16): (0, 41), (64, 4200, 31, 32): (0, 25), (64, 4200, 63, 64): (0, 25), (64, 4200, 63, 2): (0, 23), (64, 4200, 63, 4): (0, 21),
    (64, 4200, 63, 8): (0, 17), (64, 4200, 63, 16): (0, 9), (64, 4200, 63, 32): (0, 57), (32, 3, 0, 64): (0, 63), (32, 6, 0, 16): (0, 44), (32, 6, 0, 32): (0, 28),
    (32, 3, 31, 64): (0, 35), (32, 6, 31, 16): (0, 11), (32, 6, 31, 32): (0, 59), (32, 3, 63, 64): (0, 0), (32, 6, 63, 16): (0, 43), (32, 6, 63, 32): (0, 27),
    (32, 100, 0, 64): (0, 30), (32, 100, 0, 2): (0, 28), (32, 100, 0, 4): (0, 26), (32, 100, 0, 8): (0, 22), (32, 100, 0, 16): (0, 14), (32, 100, 0, 32): (0, 62),
    (32, 100, 31, 64): (0, 61), (32, 100, 31, 2): (0, 59), (32, 100, 31, 4): (0, 57), (32, 100, 31, 8): (0, 53), (32, 100, 31, 16): (0, 45), (32, 100, 31, 32): (0, 29),
    (32, 100, 63, 64): (0, 29), (32, 100, 63, 2): (0, 27), (32, 100, 63, 4): (0, 25), (32, 100, 63, 8): (0, 21), (32, 100, 63, 16): (0, 13), (32, 100, 63, 32): (0, 61),
    (32, 4200, 0, 64): (0, 26), (32, 4200, 0, 2): (1, 24), (32, 4200, 0, 4): (0, 22), (32, 4200, 0, 8): (0, 18), (32, 4200, 0, 16): (0, 10), (32, 4200, 0, 32): (0, 58),
    (32, 4200, 31, 64): (0, 57), (32, 4200, 31, 2): (0, 55), (32, 4200, 31, 4): (0, 53), (32, 4200, 31, 8): (0, 49), (32, 4200, 31, 16): (0, 41), (32, 4200, 31, 32): (1, 25),
    (32, 4200, 63, 64): (0, 25), (32, 4200, 63, 2): (0, 23), (32, 4200, 63, 4): (0, 21), (32, 4200, 63, 8): (0, 17), (32, 4200, 63, 16): (0, 9), (32, 4200, 63, 32): (1, 57),
    (64, 6, 0, 2): (0, 58), (64, 6, 0, 4): (0, 56), (64, 6, 0, 8): (0, 52), (64, 6, 31, 2): (0, 25), (64, 6, 31, 4): (0, 23), (64, 6, 31, 8): (0, 19),
    (64, 6, 63, 2): (0, 57), (64, 6, 63, 4): (0, 55), (64, 6, 63, 8): (0, 51), (32, 6, 0, 2): (0, 58), (32, 6, 0, 4): (0, 56), (32, 6, 0, 8): (0, 52),
    (32, 6, 31, 2): (0, 25), (32, 6, 31, 4): (0, 23), (32, 6, 31, 8): (0, 19), (32, 6, 63, 2): (0, 57), (32, 6, 63, 4): (0, 55), (32, 6, 63, 8): (0, 51),
}


def _crossing_lat(w, P, lane, c0, attempt, pad, n_after):
    """A quiet opening, `pad` more positions of it, then a body of period P.  The first crossings of a brute-force lookback come behind a constant
    opening instead (see CROSS_FIRST)."""
    rng = np.random.default_rng([6, w, P, lane, c0, attempt])
    if P <= BRUTE and c0 < 64:
        return wide(rng, 1, w) * (BODY_START + pad) + body(rng, w, P, P + n_after)
    a = opening(rng, w)
    return a + [a[BODY_START - Q0 + i % Q0] for i in range(pad)] + body(rng, w, P, P + n_after)


def search_crossing(w, P, lane, counts, n_after):
    """(attempt, pad) for which the count of P crosses every one of `counts` at `lane`: count c is reached c - 2 positions behind the first
    choice of P, so the first guess is right when the body settles at once; noise in which another lookback wins a position now and then
    moves a later crossing, and another seed is tried.  CROSSING_PADS below holds what this found (the CPU module checks every row's claim
    against the model's log, so a stale entry fails there)."""
    for attempt in range(8):
        for pad in sorted(range(64), key=lambda x: (x - (lane - P - counts[0] + 2)) % 64)[:8 if attempt < 7 else 64]:
            lat = _crossing_lat(w, P, lane, counts[0], attempt, pad, n_after)
            log = Log(); choose_lookbacks(lat, w, window_log(len(lat)), 0, log)
            got = {c: l for i, l, lb, c, _ in log.crossings if lb == P and i >= BODY_START}
            if all(got.get(c) == lane for c in counts): return attempt, pad
    raise AssertionError((w, P, lane, counts))


def _crossing_row(w, P, lane, counts, n_after):
    attempt, pad = CROSSING_PADS[(w, P, lane, counts[0])]
    return _crossing_lat(w, P, lane, counts[0], attempt, pad, n_after)


@functools.lru_cache(maxsize=None)
def rows_crossing():
    """(6) the running lookback's count crosses a power of two at the first lane of a tile, in the middle and at the last lane, for a
    brute-force lookback (3), a hashed near one (100) and, on the large pipeline, a far one (kCounts + 104): one row per lane for the crossings
    64 ... 4096 (from 64 on they all fall on one lane), and one short row per lane and crossing for 2, 4, 8, 16 and 32 -- the first crossings
    after a lookback is first chosen, where the bit length moves in every tile."""
    rows = []
    for w in (64, 32):
        for kind, P, shape in CROSS_KINDS:
            for lane in CROSS_LANES:
                counts = tuple(1 << k for k in range(6, CROSS_TOP.bit_length()))
                lat = _crossing_row(w, P, lane, counts, CROSS_TOP + 200)
                rows.append(_mk(f"c-u{w}-P{P}-crosses-64-to-{CROSS_TOP}@lane{lane}-pipe", lat, TYPES_ALL[w][0], ["pipe"], shape, [("lb", 0, P), ("cross", 0, P, lane, counts)], "crossing"))
                P1, firsts = CROSS_FIRST[kind]
                for c in firsts:
                    lat = _crossing_row(w, P1, lane, (c,), 160)
                    rows.append(_mk(f"c-u{w}-P{P1}-crosses-{c}@lane{lane}-pipe", lat, TYPES_ALL[w][0], ["pipe"], shape, [("lb", 0, P1), ("cross", 0, P1, lane, (c,))], "crossing"))
    return rows


TIE_P, TIE_Q, TIE_BLOCK = 4, 40, 44


# (width, lane, seed) -> phase A's length: found by search_tie
TIE_PHASE_A = {
    (64, 0, 0): 401, (64, 31, 0): 432, (64, 63, 0): 400, (64, 0, 1): 401, (64, 31, 1): 432, (64, 63, 1): 400,
    (32, 0, 0): 401, (32, 31, 0): 432, (32, 63, 0): 400, (32, 0, 1): 401, (32, 31, 1): 432, (32, 63, 1): 400,
}


def _tie_lat(rng, w, n_a, n_blocks):
    """Latents V[i % 4] + e[i] * 2^20.  Phase A (n_a positions): e repeats every TIE_Q positions and differs TIE_P back, so lookback TIE_Q is
    chosen and gathers a count.  Then blocks of TIE_BLOCK positions with e = the block's number: at a block's offsets 4 .. 39 only TIE_P back has
    delta 0 (its count grows), at offsets 40 .. 43 and 0 .. 3 of the next block the deltas TIE_P and TIE_Q back are IDENTICAL (0, then 2^20)."""
    V = wide(rng, TIE_P, w); r = [1 + int(x) for x in rng.permutation(TIE_Q)]
    lat = [V[i % TIE_P] + (r[i % TIE_Q] << 20) for i in range(n_a)]
    for k in range(n_blocks): lat += [V[(n_a + k * TIE_BLOCK + j) % TIE_P] + ((100 + k) << 20) for j in range(TIE_BLOCK)]
    return lat


def _tie_claims(lat, w):
    """(position of the flip, claims) or None: the FLIP is the first position with identical deltas at which the brute-force lookback TIE_P,
    whose count has just reached the bit length of TIE_Q's, wins on proposal order against TIE_Q in a repeating slot."""
    mask = (1 << w) - 1
    log = Log(); lbs = choose_lookbacks(lat, w, window_log(len(lat)), 0, log)
    same = [i for i in range(TIE_Q + 1, len(lat)) if (lat[i] - lat[i - TIE_P]) & mask == (lat[i] - lat[i - TIE_Q]) & mask]
    flip = next((i for a, i in zip(same, same[1:]) if lbs[a - 1] == TIE_Q and lbs[i - 1] == TIE_P), None)
    if flip is None or (flip, "brute", "repeating") not in log.ties: return None
    before = max(i for i in same if i < flip)
    return flip, [("at", 0, before, TIE_Q), ("at", 0, flip, TIE_P), ("tie", 0, flip, "brute", "repeating"), ("same", 0, before, TIE_P, TIE_Q), ("same", 0, flip, TIE_P, TIE_Q)]


def search_tie(w, lane, seed):
    """Phase A's length for which the flip falls on `lane`; TIE_PHASE_A below holds what this found."""
    for n_a in range(400, 400 + 3 * 64):
        found = _tie_claims(_tie_lat(np.random.default_rng([10, w, seed]), w, n_a, 30), w)
        if found is not None and (found[0] - 1) % 64 == lane: return n_a
    raise AssertionError((w, lane, seed))


def _tie_row(w, lane, seed):
    lat = _tie_lat(np.random.default_rng([10, w, seed]), w, TIE_PHASE_A[(w, lane, seed)], 30)
    flip, claims = _tie_claims(lat, w)
    assert (flip - 1) % 64 == lane and flip > 1 + 64 * (kLbSeqTiles + 1), (w, lane, seed, flip)   # behind tile 9: stage D may take the ready-made maxima
    return lat, claims


@functools.lru_cache(maxsize=None)
def rows_tie():
    """(6) two lookbacks of different groups with identical deltas whose counts overtake each other: lookback 40 sits in a repeating slot with
    the larger count and wins the positions where 4 and 40 back give the same delta; the count of lookback 4 (brute force) grows in between, and
    at the first such position where the two counts have the same bit length the goodness ties and proposal order gives it to 4.  The flip is
    put at lane 0, 31 and 63, behind tile 9 (where stage D takes the ready-made maxima), on the small and the large pipeline."""
    rows = []
    for w in (64, 32):
        for si, shape in enumerate((("small", "LbSmall"), ("large", "LbFull"))):
            for lane in CROSS_LANES:
                lat, claims = _tie_row(w, lane, si)
                rows.append(_mk(f"e-u{w}-{shape[0]}-brute4-overtakes-repeating40@lane{lane}-pipe", lat, TYPES_ALL[w][0], ["pipe"], shape, claims, "tie"))
    return rows


@functools.lru_cache(maxsize=None)
def rows_screen():
    """(7) max - min exactly 4 n - 1 (screened) and 4 n at 8191, 8192 and 8193 numbers (8193 is never screened); at 8192 numbers and a span of
    32767 pairs that differ by exactly 32767 with low halves that wrap; 8-bit pages with differences of exactly 127, 128 and 129."""
    rows = []
    for w in (64, 32, 16):
        for n in (kLbPipeSmallMaxPage - 1, kLbPipeSmallMaxPage, kLbPipeSmallMaxPage + 1):
            for span in (kScreenSpan * n - 1, kScreenSpan * n):
                rng = np.random.default_rng([7, w, n, span & 1])
                lo = 65536 - 16384 if w > 16 else 100
                seq = n <= kLbPipeSmallMaxPage and span < kScreenSpan * n
                if w > 16: lat = [lo + int(x) for x in rng.integers(0, span + 1, n)]; route = "seq" if seq else "back"    # narrow random numbers: a new lookback at nearly every element
                else:   # (16 bits: random numbers over half the type do not compress under a lookback delta; a period inside the span does)
                    lat = extend(rng, opening(rng, w, base=[lo + int(x) for x in rng.integers(4, span - 4, Q0)]), n); route = "seq" if seq else "pipe"
                lat[11] = lo; lat[12] = lo + span; lat[4000] = lo + span; lat[4001] = lo
                shape = ("small", "LbSmall") if n <= kLbPipeSmallMaxPage else ("large", "LbFull")
                rows.append(_mk(f"s-u{w}-n{n}-span{'4n-1' if span & 1 else '4n'}-{route}", lat, UINT[w], [route], shape, [], "screen"))
    for d in (127, 128, 129):
        for dt in (np.uint8, np.int8):
            rng = np.random.default_rng([7, 8, d]); n = 700
            lat = [int(x) for x in rng.choice([10, 11, 10 + d, 11 + d, 60], n)]
            rows.append(_mk(f"s-{W.tname(dt)}-differences-of-{d}-seq", lat, dt, ["seq"], ("small", "LbSmall"), [], "screen"))
    return rows


UINT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
INT_MULT_BASE = 1000


@functools.lru_cache(maxsize=None)
def rows_types():
    """Signed and float types through Classic mode, and one int-mult chunk whose secondary sits beside the lookbacks."""
    rows = []
    P = kNear["small"]
    for dt in (np.int64, np.float64, np.int32, np.float32):
        w = np.dtype(dt).itemsize * 8; rng = np.random.default_rng([9, w, np.dtype(dt).kind == "f"])
        lat = opening(rng, w) + body(rng, w, P, P + 320)
        rows.append(_mk(f"y-{W.tname(dt)}-pipe-small-P{P}", lat, dt, ["pipe"], ("small", "LbSmall"), [("lb", 0, P)], "threshold"))
    rng = np.random.default_rng([9, 99])
    m = [x >> 12 for x in opening(rng, 32) + body(rng, 32, P, P + 320)]
    arr = (np.array(m, np.uint64) * np.uint64(INT_MULT_BASE) + rng.integers(0, INT_MULT_BASE, len(m)).astype(np.uint64)).astype(np.uint32)
    rows.append(Row(f"y-uint32-int-mult-pipe-small-P{P}", arr, dict(mode=4, mode_u64=INT_MULT_BASE, delta=3), [arr.size], None, ["pipe"], ("small", "LbSmall"), [("lb", 0, P)], "threshold"))
    return rows


def all_rows():
    return rows_thresholds() + rows_handback() + rows_window() + rows_sweep() + rows_bucket() + rows_hazard() + rows_crossing() + rows_tie() + rows_screen() + rows_types()


PageResult = collections.namedtuple("PageResult", "lbs log route rounds")


@functools.lru_cache(maxsize=None)
def analysis_of(name):
    """Per page of a row, from the finished array: the model's lookbacks, its event log, the predicted route and stage D's rounds per tile."""
    r = BY_NAME()[name]
    p, _ = W.ordered_latents(r.arr, r.kw)
    bits = p.dtype.itemsize * 8; wlog = window_log(r.arr.size); out = []; start = 0
    for pn in r.pages:
        lat = [int(x) for x in p[start:start + pn]]; start += pn
        log = Log(); lbs = choose_lookbacks(lat, bits, wlog, 0, log)
        out.append(PageResult(lbs, log, page_route(lat, lbs), tile_rounds(lbs)))
    return out


@functools.lru_cache(maxsize=None)
def BY_NAME():
    rows = all_rows()
    out = {r.name: r for r in rows}
    assert len(out) == len(rows), "row names repeat"
    return out


def group_key(row):
    """What rows share to share a call: the config, the entry point, and the call's shape."""
    return (tuple(sorted(row.kw.items())), row.paging, row.shape)


def groups():
    out = collections.OrderedDict()
    for r in all_rows():
        out.setdefault(group_key(r), []).append(r)
    return list(out.values())
