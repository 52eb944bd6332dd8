"""The front of the encoder -- the speculative 16-bit latent window and the histogram tiers behind it -- as a PLAIN MODEL, and the rows that
sit on every edge of it.  Shared by tests/test_latent_window.py (-m "not gpu") and tests/test_gpu_latent_window.py (-m gpu).

The model is numpy and Python integers and shares no code with the library.  It restates what the kernels decide:

  * enc_init_kernel: a chunk speculates unless its delta is lookback or Conv1 or its histogram has more than 256 bins ("never");
  * enc_split_body<..., kSpec = true>: a latent is stored as the key (latent - (ref - bias)) mod 2^w, and fits iff the key is below
    kC16KeyRange.  ref of the primary is the toggle 2^(w-1) under a consecutive delta, else the CHUNK's first primary latent clamped to
    [bias, Lmax - bias]; ref of the secondary is the chunk's first secondary latent, clamped the same way.  The first `order` positions of
    every page hold no latent of the primary and are not checked (the secondary is checked everywhere); 8-bit latents always fit;
  * enc_presample_kernel: one-page chunks of at least 4096 numbers of 16 bits or more are sampled at 64 positions lane * ((n - 8) / 64)
    (the latent examined sits `order` behind the position); one bad sample takes the chunk out up front ("sample").  Any other bad latent
    is found by its tile and the chunk is split again at full width ("redo"); a chunk without a bad latent stays ("c16");
  * hist_var: per variable, from (numeric max - min, number of latents), the counting kernel: "direct" below kDirectHistRange, else "small"
    up to kSmallHistCap latents, else "mid" below kMidHistRange, "wide" below kWideHistRange, "select" beyond.

Two consequences of the clamp that the rows pin (both follow from the window being [ref - 2^14, ref + 2^14 - 1]): with the first latent
within 2^14 of the type's upper end the window is [Lmax - 2^15, Lmax - 1], so a latent of Lmax itself -- the first one included -- leaves;
and a 16-bit type is covered by [0, 32767] and [32767, 65534], not by [32768, 65535].

Every constant is read from the .hip sources, so a moved threshold fails tests/test_latent_window.py instead of silently moving the rows."""
import collections
import functools
import os
import re

import numpy as np

import format_limits_util as F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pcodec_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = set(re.findall(pattern, text))
    assert len(found) == 1, (what, found)
    return found.pop()


_K = _read("encode_kernels.hip")
kC16KeyRange = int(_one(r"\bkC16KeyRange\s*=\s*(\d+)u?\s*;", _K, "kC16KeyRange"))
kDirectHistRange = int(_one(r"\bkDirectHistRange\s*=\s*(\d+)\s*;", _K, "kDirectHistRange"))
kMidHistRange = int(_one(r"\bkMidHistRange\s*=\s*(\d+)\s*;", _K, "kMidHistRange"))
kWideHistRange = int(_one(r"\bkWideHistRange\s*=\s*(\d+)\s*,", _K, "kWideHistRange"))
kSmallHistCap = int(_one(r"\bkSmallHistCap\s*=\s*(\d+)\s*;", _K, "kSmallHistCap"))
kSplitE = int(_one(r"\bkSplitE\s*=\s*(\d+)\s*,", _K, "kSplitE"))
kSplitTile = int(_one(r"\bkSplitTile\s*=\s*(\d+)\s*\*\s*kSplitE\s*;", _K, "kSplitTile")) * kSplitE
kMaxUnoptBinsLog = int(_one(r"\bkMaxUnoptBinsLog\s*=\s*(\d+)\s*;", _K, "kMaxUnoptBinsLog"))
# the bias literal: once in the split tile, once in the presample, and the same in both
_BIAS = re.findall(r"kBias\s*=\s*sizeof\(L\)\s*==\s*1\s*\?\s*\(L\)0\s*:\s*\(L\)(\d+)\s*,", _K)
assert len(_BIAS) == 2 and len(set(_BIAS)) == 1, _BIAS
kBias = int(_BIAS[0])
kPresampleMinN = int(_one(r"ch->n\)\s*<\s*(\d+)\)\s*return", _K, "the presample's floor"))
_PS = _one(r"pos\s*=\s*\(uint64_t\)lane\s*\*\s*\(\(n\s*-\s*(\d+)\)\s*/\s*(\d+)\)", _K, "the presample's positions")
kPresampleTail, kPresampleLanes = int(_PS[0]), int(_PS[1])

ROUTES = ("never", "sample", "redo", "c16")
TIERS = ("direct", "small", "mid", "wide", "select")
# what a synchronous call launches behind enc_hist_kernel for a variable of each tier (pco_gfx_encode_api.inc: only what the device flagged)
TIER_KERNELS = {"direct": (), "small": ("enc_hist_small_kernel",), "mid": ("enc_hist_wide_kernel<%d>" % kMidHistRange,),
                "wide": ("enc_hist_wide_kernel<%d>" % kWideHistRange,), "select": ("enc_hist_select_kernel", "enc_hist_sort_kernel")}
HIST_KERNELS = tuple(sorted({k for ks in TIER_KERNELS.values() for k in ks}))
SPLIT_KERNELS = ("enc_split_kernel", "enc_split_kernel(redo)", "enc_split_kernel<c16>")


def split_kernels_for(routes):
    """The split kernels a synchronous call launches for chunks of these routes."""
    routes = set(routes); out = set()
    if routes & {"c16", "redo"}: out.add("enc_split_kernel<c16>")
    if routes & {"sample", "never"}: out.add("enc_split_kernel")
    if "redo" in routes: out.add("enc_split_kernel(redo)")
    return out


# ------------------------------------------------------------------------------------------------ the model
def order_of(kw):
    return kw.get("delta_order", 0) if kw.get("delta") == 2 else 0


def unopt_bins_log(level, n):
    """wrapped/chunk_compressor.rs choose_unoptimized_bins_log"""
    log_n = n.bit_length() - 1
    fast = max(log_n - 4, 0)
    return level if level <= fast else fast + (level - fast) // 2


def speculates(kw, n):
    """enc_init_kernel: c16_ok starts at 1 unless the delta is lookback (3) or Conv1 (4) or the chunk has more than 256 bins."""
    return kw.get("delta") not in (3, 4) and unopt_bins_log(kw.get("level", 8), n) <= kMaxUnoptBinsLog


def ordered_latents(arr, kw):
    """(primary, secondary or None) before any delta, as arrays of the width's unsigned type."""
    u = F.UINT[F.width(arr.dtype)]
    p, s, _ = F.model_split(arr, kw)
    return np.array(p, dtype=u), (np.array(s, dtype=u) if s is not None else None)


def page_differences(p, order, pages):
    """The primary as the split stores it: per page `order` rounds of adjacent differences in the type's modular arithmetic, plus the
    toggle 2^(w-1) when order > 0.  Returns (values, stored): page positions below `order` hold no latent (what is computed there, with
    zeros in front of the page, is in `values` all the same: it is what a tile sees and must not judge)."""
    w = p.dtype.itemsize * 8; u = p.dtype.type
    out = p.copy(); stored = np.ones(p.size, bool); start = 0
    for pn in pages:
        seg = p[start:start + pn].copy()
        for _ in range(order):
            nxt = seg.copy(); nxt[1:] = seg[1:] - seg[:-1]; seg = nxt
        out[start:start + pn] = seg
        stored[start:start + min(order, pn)] = False
        start += pn
    assert start == p.size
    if order > 0:
        out = out + u(1 << (w - 1))
    return out, stored


def clamp_ref(x, w):
    lmax = (1 << w) - 1
    return max(kBias, min(int(x), lmax - kBias))


def keys_of(lat, ref):
    """(latent - (ref - bias)) mod 2^w"""
    w = lat.dtype.itemsize * 8
    return lat - lat.dtype.type((ref - kBias) % (1 << w))


def sample_indices(n, order):
    step = (n - kPresampleTail) // kPresampleLanes
    return [lane * step + order for lane in range(kPresampleLanes)]


def tier_of(rng, n_lat):
    if rng < kDirectHistRange: return "direct"
    if n_lat <= kSmallHistCap: return "small"
    if rng < kMidHistRange: return "mid"
    if rng < kWideHistRange: return "wide"
    return "select"


Analysis = collections.namedtuple("Analysis", "route tiers bad1 bad2 junk_inside junk_pages_outside n_lat ranges min_keys")


def analyse(arr, kw, pages):
    """Everything the model says about a chunk: the route, the tier per variable (primary, secondary; None for an absent one or for a chunk
    that never speculates under a lookback delta, whose primary the model does not compute), the positions that do not fit, how many
    unstored positions would fit if they were judged, how many pages have an unstored position that would NOT fit, latents per variable, numeric ranges and the smallest key per variable."""
    n = arr.size; w = F.width(arr.dtype); order = order_of(kw)
    p, s = ordered_latents(arr, kw)
    spec = speculates(kw, n)
    if kw.get("delta") in (3, 4):
        return Analysis("never", (None, None), [], [], 0, 0, (None, None), (None, None), (None, None))
    d, stored = page_differences(p, order, pages)
    ref1 = (1 << (w - 1)) if order > 0 else clamp_ref(p[0], w)
    ref2 = clamp_ref(s[0], w) if s is not None else None
    if w == 8:
        k1 = d.astype(np.uint64); k2 = s.astype(np.uint64) if s is not None else None   # stored as they are: always below the bound
    else:
        k1 = keys_of(d, ref1).astype(np.uint64); k2 = keys_of(s, ref2).astype(np.uint64) if s is not None else None
    bad1 = np.flatnonzero((k1 >= kC16KeyRange) & stored).tolist()
    bad2 = np.flatnonzero(k2 >= kC16KeyRange).tolist() if k2 is not None else []
    junk_inside = int(((k1 < kC16KeyRange) & ~stored).sum())
    starts = np.concatenate([[0], np.cumsum(pages)]).astype(int)
    junk_pages_outside = sum(bool(((k1 >= kC16KeyRange) & ~stored)[a:b].any()) for a, b in zip(starts[:-1], starts[1:]))
    if not spec:
        route = "never"
    else:
        sampled = set(sample_indices(n, order)) if len(pages) == 1 and n >= kPresampleMinN and w >= 16 else set()
        if sampled & (set(bad1) | set(bad2)): route = "sample"
        elif bad1 or bad2: route = "redo"
        else: route = "c16"
    lat1 = [int(x) for x in d[stored]]; n1 = len(lat1)
    r1 = max(lat1) - min(lat1) if n1 else 0
    big = unopt_bins_log(kw.get("level", 8), n) > kMaxUnoptBinsLog
    t1 = "select" if big else tier_of(r1, n1)
    mk1 = int(k1[stored].min()) if n1 else None
    if s is None:
        return Analysis(route, (t1, None), bad1, bad2, junk_inside, junk_pages_outside, (n1, None), (r1, None), (mk1, None))
    r2 = int(s.max()) - int(s.min())
    return Analysis(route, (t1, "select" if big else tier_of(r2, n)), bad1, bad2, junk_inside, junk_pages_outside, (n1, n), (r1, r2), (mk1, int(k2.min())))


def route(arr, kw, pages):
    return analyse(arr, kw, pages).route


# ------------------------------------------------------------------------------------------------ building data from latents
def from_latents(lat, dt):
    """Numbers of type dt whose ordered latents are `lat` (Number::from_latent_ordered, vectorised)."""
    dt = np.dtype(dt); w = F.width(dt); u = F.UINT[w]
    l = np.array([int(x) % (1 << w) for x in lat], dtype=u)
    mid = u(1 << (w - 1)); ones = u((1 << w) - 1)
    if dt.kind == "u": b = l
    elif dt.kind == "i": b = l ^ mid
    else: b = np.where(l & mid != 0, l ^ mid, l ^ ones).astype(u)
    return np.ascontiguousarray(b.view(dt))


def integrate(dd, order, moments, w):
    """Latents whose `order`-th differences at positions >= order are dd[order:] (mod 2^w); moments[r] is the r-th difference at position r."""
    mask = (1 << w) - 1
    cur = [int(x) & mask for x in dd]
    n = len(cur)
    for r in range(order, 0, -1):
        nxt = [0] * n
        acc = int(moments[r - 1]) & mask
        nxt[r - 1] = acc
        for i in range(r, n):
            acc = (acc + cur[i]) & mask
            nxt[i] = acc
        cur = nxt
    return cur


Row = collections.namedtuple("Row", "name arr kw pages route tiers section paging")
# paging: None = a standalone chunk (pco_gfx_compress_chunks); "exact" = a wrapped chunk in exactly `pages` (PagingSpec::Exact); "equal" = a
# wrapped chunk cut by kw["max_page_n"] (PagingSpec::EqualPagesUpTo) into `pages`

CLASSIC = dict(mode=1, delta=1)
WINDOW_TYPES = [np.uint16, np.int16, np.float16, np.uint32, np.int32, np.float32, np.uint64, np.int64, np.float64]
N_BIG, N_SMALL = 4608, 300            # two full split tiles and one of 512; below the presample's floor
INSIDE, OUTSIDE = (-kBias, kBias - 1), (-kBias - 1, kBias)


def tname(dt):
    return np.dtype(dt).name


def sampled_index(n, order, lane=17):
    return sample_indices(n, order)[lane]


def unsampled_index(n, order, lane=17):
    i = sample_indices(n, order)[lane] + 1
    assert i not in sample_indices(n, order) and order <= i < n
    return i


def leaving_route(n, order, idx, single_page=True):
    """By construction: a chunk whose only latents outside the window sit at `idx`."""
    if single_page and n >= kPresampleMinN and set(idx) & set(sample_indices(n, order)):
        return "sample"
    return "redo"


def _row(name, arr, kw, route_, section, pages=None, tiers=None, paging=None):
    return Row(name, arr, dict(kw), list(pages) if pages is not None else [arr.size], route_, tiers, section, paging)


@functools.lru_cache(maxsize=None)
def rows_a():
    """(a) window edges without delta: one latent at ref - 2^14, ref + 2^14 - 1 (stay) and one step beyond each (leave)."""
    rows = []
    for ti, dt in enumerate(WINDOW_TYPES):
        w = F.width(dt); first = (1 << (w - 1)) + 12345
        for n in (N_BIG, N_SMALL):
            rng = np.random.default_rng([1, ti, n])
            base = [first + int(x) for x in rng.integers(-100, 101, n)]; base[0] = first
            places = {"any": 157} if n < kPresampleMinN else {"sampled": sampled_index(n, 0), "unsampled": unsampled_index(n, 0), "i2047": kSplitTile - 1,
                                                             "i2048": kSplitTile, "last": n - 1}
            for off in INSIDE + OUTSIDE:
                for place, idx in places.items():
                    lat = list(base); lat[idx] = first + off
                    r = "c16" if off in INSIDE else leaving_route(n, 0, [idx])
                    rows.append(_row(f"a-{tname(dt)}-n{n}-ref{off:+d}@{place}-{r}", from_latents(lat, dt), CLASSIC, r, "a"))
    for n in (N_SMALL, N_BIG):   # the control: 8-bit latents are stored as they are
        rows.append(_row(f"a-uint8-n{n}-whole-type-c16", np.random.default_rng([1, 99, n]).integers(0, 256, n).astype(np.uint8), CLASSIC, "c16", "a"))
    return rows


@functools.lru_cache(maxsize=None)
def rows_b():
    """(b) the clamp: first latents at and next to both ends of the type and of the clamp, later latents at the ends of the clamped window."""
    rows = []
    for ti, dt in enumerate(WINDOW_TYPES):
        w = F.width(dt); lmax = (1 << w) - 1
        firsts = {"0": 0, "1": 1, "bias-1": kBias - 1, "bias": kBias, "max-bias": lmax - kBias, "max-bias+1": lmax - kBias + 1, "max": lmax}
        for fi, (fname, first) in enumerate(firsts.items()):
            ref = min(max(first, kBias), lmax - kBias)                  # (stated again: the builder's claim does not go through clamp_ref)
            lo, hi = ref - kBias, ref + kBias - 1
            first_fits = lo <= first <= hi                              # false for the type's maximum alone
            sizes = (N_SMALL, N_BIG) if fname == "max" and dt in (np.uint16, np.int32, np.float64) else (N_SMALL,)   # (at 4608 lane 0 of the presample reads the first latent)
            for n in sizes:
                rng = np.random.default_rng([2, ti, fi, n])
                base = [min(max(first + int(x), lo), hi) for x in rng.integers(-100, 101, n)]; base[0] = first
                idx = 157
                for vname, v in (("base", None), ("lo", lo), ("hi", hi), ("below", lo - 1), ("above", hi + 1)):
                    if v is not None and not 0 <= v <= lmax:
                        continue                                         # that step does not exist inside the type
                    lat = list(base)
                    if v is not None: lat[idx] = v
                    bad = ([] if first_fits else [0]) + ([idx] if vname in ("below", "above") else [])
                    r = leaving_route(n, 0, bad) if bad else "c16"
                    rows.append(_row(f"b-{tname(dt)}-n{n}-first@{fname}-{vname}-{r}", from_latents(lat, dt), CLASSIC, r, "b"))
    for ti, dt in enumerate((np.uint16, np.int16)):   # a 16-bit type in halves
        n = N_BIG; i_min, i_max = unsampled_index(n, 0), kSplitTile - 1
        for lo, hi, first, r in ((0, 32767, 5, "c16"), (32767, 65534, 60000, "c16"), (32768, 65535, 60000, "redo"), (0, 32768, 5, "redo")):
            rng = np.random.default_rng([2, 50 + ti, lo, hi])
            lat = [int(x) for x in rng.integers(lo, hi, n)]   # (the upper end once, below: where it is outside the window it is the only such latent)
            lat[0] = first; lat[i_min] = lo; lat[i_max] = hi
            rows.append(_row(f"b-{tname(dt)}-n{n}-covers[{lo},{hi}]-{r}", from_latents(lat, dt), CLASSIC, r, "b"))
    return rows


ORDER_TYPES = [np.uint16, np.int32, np.float32, np.uint64]
ORDERS = (1, 2, 7)
EXACT_PAGES = [2049, 1111, 1448]      # pages that start at an odd index (2049) and at an even one (3160)
EQUAL_N, EQUAL_MAX_PAGE_N = 4611, 1537   # EqualPagesUpTo: three pages of 1537, starting at 1537 and 3074


def _huge_moments(w, order, rng):
    return [(1 << (w - 3)) + int(rng.integers(0, 1 << 62)) % (3 << (w - 3)) for _ in range(order)]   # anywhere in [2^(w-3), 2^(w-1))


def _delta_row(name, dt, order, n, special, route_, seed, huge=False, pages=None, paging=None, kw_extra=None):
    """A chunk whose order-th differences are noise within +-50 except `special` = {index: difference}."""
    w = F.width(dt)
    kw = dict(mode=1, delta=2, delta_order=order, **(kw_extra or {}))
    for attempt in range(64):
        rng = np.random.default_rng([3, seed, attempt])
        dd = [int(x) for x in rng.integers(-50, 51, n)]
        for i, v in special.items(): dd[i] = v
        moments = _huge_moments(w, order, rng) if huge else [int(x) for x in rng.integers(0, 1000, order)]
        arr = from_latents(integrate(dd, order, moments, w), dt)
        an = analyse(arr, kw, pages or [n]) if huge else None
        # a junk row: every page has an unstored position that would fail if it were judged -- all of them do at 32 and 64 bits (at 16 bits half
        # of all values lie inside any window)
        if not huge or (an.junk_pages_outside == len(pages or [n]) and (w == 16 or an.junk_inside == 0)):
            return _row(name, arr, kw, route_, "c", pages=pages, paging=paging)
    raise AssertionError(name)


@functools.lru_cache(maxsize=None)
def rows_c():
    """(c) consecutive orders 1, 2 and 7: the window is centred on the toggle.  One page, then the same as wrapped chunks of several pages."""
    rows = []
    for ti, dt in enumerate(ORDER_TYPES):
        for order in ORDERS:
            n = N_BIG; seed = ti * 10 + order
            places = {"sampled": sampled_index(n, order), "unsampled": unsampled_index(n, order)}
            for off in INSIDE + OUTSIDE:
                for place, idx in places.items():
                    r = "c16" if off in INSIDE else leaving_route(n, order, [idx])
                    rows.append(_delta_row(f"c-{tname(dt)}-o{order}-n{n}-diff{off:+d}@{place}-{r}", dt, order, n, {idx: off}, r, seed))
            rows.append(_delta_row(f"c-{tname(dt)}-o{order}-n{n}-junk-c16", dt, order, n, {}, "c16", seed, huge=True))
            for m in (N_BIG, N_SMALL):   # the first stored position: lane 0 of the presample reads it
                r = leaving_route(m, order, [order])
                rows.append(_delta_row(f"c-{tname(dt)}-o{order}-n{m}-junk-diff{kBias:+d}@first-stored-{r}", dt, order, m, {order: kBias}, r, seed, huge=True))
            # several pages: no presample, so every leaving row is a redo
            for paging, n, pages, extra in (("exact", sum(EXACT_PAGES), EXACT_PAGES, None), ("equal", EQUAL_N, [EQUAL_MAX_PAGE_N] * 3, dict(max_page_n=EQUAL_MAX_PAGE_N))):
                p2 = pages[0]
                for off in INSIDE + OUTSIDE:
                    r = "c16" if off in INSIDE else "redo"
                    rows.append(_delta_row(f"c-{tname(dt)}-o{order}-{paging}{pages[0]}-diff{off:+d}@page2+500-{r}", dt, order, n, {p2 + 500: off}, r, seed, pages=pages, paging=paging, kw_extra=extra))
                rows.append(_delta_row(f"c-{tname(dt)}-o{order}-{paging}{pages[0]}-junk-c16", dt, order, n, {}, "c16", seed, huge=True, pages=pages, paging=paging, kw_extra=extra))
                # differences far outside AT the unstored positions of the later pages (they are part of those pages' delta state, not latents)
                far = 20000 if F.width(dt) == 16 else (1 << (F.width(dt) - 2)) + 12345   # (outside the window as a difference, and it keeps the raw values outside too)
                junk = {pages[0] + j: far for j in range(order)}; junk.update({pages[0] + pages[1] + j: -far for j in range(order)})
                rows.append(_delta_row(f"c-{tname(dt)}-o{order}-{paging}{pages[0]}-junk-differences-at-unstored-c16", dt, order, n, junk, "c16", seed, huge=True, pages=pages, paging=paging, kw_extra=extra))
                rows.append(_delta_row(f"c-{tname(dt)}-o{order}-{paging}{pages[0]}-junk-diff{kBias:+d}@page2-first-stored-redo", dt, order, n, {p2 + order: kBias}, "redo", seed, huge=True, pages=pages, paging=paging, kw_extra=extra))
    return rows


@functools.lru_cache(maxsize=None)
def rows_d():
    """(d) secondary variables: either variable may end the speculation."""
    rows = []
    n = N_BIG; i_s, i_u, i_edge = sampled_index(n, 0), unsampled_index(n, 0, lane=18), unsampled_index(n, 0)
    # int-mult: first remainder 0, so ref2 is clamped to 2^14 and the window is [0, 32767]
    for ti, dt in enumerate((np.uint32, np.uint64)):
        for base in (32768, 32769, 40000):
            kw = dict(mode=F.MODE_INT_MULT, mode_u64=base, delta=1)
            rng = np.random.default_rng([4, ti, base])
            m0 = 50000
            m = [m0 + int(x) for x in rng.integers(-100, 101, n)]; m[0] = m0
            r = [int(x) for x in rng.integers(0, 32768, n)]; r[0] = 0; r[i_edge] = 32767
            def make(mm, rr): return from_latents([a * base + b for a, b in zip(mm, rr)], dt)
            rows.append(_row(f"d-{tname(dt)}-imult{base}-remainders-to-32767-c16", make(m, r), kw, "c16", "d"))
            if base > 32768:
                for place, idx in (("sampled", i_s), ("unsampled", i_u)):
                    rr = list(r); rr[idx] = 32768
                    rt = leaving_route(n, 0, [idx])
                    rows.append(_row(f"d-{tname(dt)}-imult{base}-remainder32768@{place}-{rt}", make(m, rr), kw, rt, "d"))
            for place, idx in (("sampled", i_s), ("unsampled", i_u)):
                mm = list(m); mm[idx] = m0 + kBias
                rt = leaving_route(n, 0, [idx])
                rows.append(_row(f"d-{tname(dt)}-imult{base}-primary{kBias:+d}@{place}-{rt}", make(mm, r), kw, rt, "d"))
    # float-quant: the secondary is the low k bits (mirrored for negative numbers; these are positive)
    for ti, ft in enumerate((np.float32, np.float64)):
        w = F.width(ft)
        for k in (15, 16):
            kw = dict(mode=F.MODE_FLOAT_QUANT, mode_u64=k, delta=1)
            rng = np.random.default_rng([4, 10 + ti, k])
            p0 = ((1 << (w - 1)) + (1 << (w - 3))) >> k
            p = [p0 + int(x) for x in rng.integers(-100, 101, n)]; p[0] = p0
            low = [int(x) for x in rng.integers(0, 32768, n)]; low[0] = 0; low[i_edge] = 32767
            def make(pp, ll): return from_latents([(a << k) | b for a, b in zip(pp, ll)], ft)
            rows.append(_row(f"d-{tname(ft)}-fquant{k}-first0-lows-to-32767-c16", make(p, low), kw, "c16", "d"))
            if k == 15:   # all k bits set in the first number: ref2 = 32767, the window is [16383, 49150] and a low of 16382 or less is outside
                hi_low = [int(x) for x in rng.integers(16383, 32768, n)]; hi_low[0] = 32767; hi_low[i_edge] = 16383
                rows.append(_row(f"d-{tname(ft)}-fquant15-first32767-lows-from-16383-c16", make(p, hi_low), kw, "c16", "d"))
                outs = (16382, 0)
            else:
                outs = (32768, 65535)
            for v in outs:
                for place, idx in (("sampled", i_s), ("unsampled", i_u)):
                    ll = list(hi_low if k == 15 else low); ll[idx] = v
                    rt = leaving_route(n, 0, [idx])
                    rows.append(_row(f"d-{tname(ft)}-fquant{k}-low{v}@{place}-{rt}", make(p, ll), kw, rt, "d"))
            for place, idx in (("sampled", i_s), ("unsampled", i_u)):
                pp = list(p); pp[idx] = p0 + kBias
                rt = leaving_route(n, 0, [idx])
                rows.append(_row(f"d-{tname(ft)}-fquant{k}-primary{kBias:+d}@{place}-{rt}", make(pp, low), kw, rt, "d"))
    # float-mult 0.01: multiples of the base are within a few ulps of mult * base; one number half a base away is tens of thousands of ulps off
    for ti, (ft, lo_m, odd) in enumerate(((np.float32, 10, 0.505), (np.float64, 1000, 55.555))):
        kw = dict(mode=F.MODE_FLOAT_MULT, mode_f64=0.01, delta=1)
        rng = np.random.default_rng([4, 20 + ti])
        mult = rng.integers(lo_m, 10 * lo_m, n)
        clean = (mult / 100.0).astype(ft)
        rows.append(_row(f"d-{tname(ft)}-fmult0.01-multiples-c16", clean, kw, "c16", "d"))
        for place, idx in (("sampled", i_s), ("unsampled", i_u)):
            x = clean.copy(); x[idx] = odd
            rt = leaving_route(n, 0, [idx])
            rows.append(_row(f"d-{tname(ft)}-fmult0.01-no-multiple@{place}-{rt}", x, kw, rt, "d"))
            x = clean.copy(); x[idx] = ft((int(mult[0]) + 20000) / 100.0)
            rows.append(_row(f"d-{tname(ft)}-fmult0.01-primary+20000@{place}-{rt}", x, kw, rt, "d"))
    return rows


# (e) histogram tiers
COMPACT_RANGES = (kDirectHistRange - 1, kDirectHistRange, kMidHistRange - 1, kMidHistRange, kWideHistRange - 2, kWideHistRange - 1)
FULL_RANGES = (kMidHistRange, kWideHistRange - 1, kWideHistRange, 100000)
RESIDUES = (0, 1, kDirectHistRange // 2, kDirectHistRange - 1)
TIER_N_LAT = (kSmallHistCap, kSmallHistCap + 1, 20000)
TIER_KINDS = ("u64", "d1-u32", "imult-i64")
TIER_BASE = 200003


def compact_split(rng_, residue):
    """(a, b, residue reached) with a + b = rng_, a <= bias, b <= bias - 1, and the smallest key bias - a as close to `residue` modulo
    kDirectHistRange as the window allows (the widest ranges leave one or two choices of a)."""
    lo_a, hi_a = max(0, rng_ - (kBias - 1)), min(kBias, rng_)
    fit = [a for a in range(lo_a, hi_a + 1) if (kBias - a) % kDirectHistRange == residue]
    a = fit[len(fit) // 2] if fit else hi_a
    return a, rng_ - a, (kBias - a) % kDirectHistRange


@functools.lru_cache(maxsize=None)
def rows_e():
    rows = []
    specs = [("compact", r) for r in COMPACT_RANGES] + [("full", r) for r in FULL_RANGES]
    for ri, (form, R) in enumerate(specs):
        for ki, kind in enumerate(TIER_KINDS):
            for si, n_lat in enumerate(TIER_N_LAT):
                j = ki * 3 + si
                residue = RESIDUES[(j + ri) % 4]; level = 0 if (j + ri) % 3 == 0 else 8
                order = 1 if kind == "d1-u32" else 0
                n = n_lat + order
                rng = np.random.default_rng([5, ri, j])
                i_min, i_max, i_s = unsampled_index(n, order, 20), unsampled_index(n, order, 40), sampled_index(n, order, 5)
                if form == "compact":
                    a, b, residue = compact_split(R, residue)
                    rel = [int(x) for x in rng.integers(-a, b + 1, n)]; rel[order] = 0; rel[i_min] = -a; rel[i_max] = b
                    r = "c16"
                elif R == kMidHistRange:   # the first latent is the minimum; only the maximum, ref + 2^14, is outside the window
                    rel = [int(x) for x in rng.integers(0, kBias, n)]; rel[order] = 0; rel[i_max] = R
                    r = "redo"
                else:
                    rel = [int(x) for x in rng.integers(0, R + 1, n)]; rel[order] = 0; rel[i_s] = R
                    r = "sample"
                tier = tier_of(R, n_lat)                                 # (the tiers' own statement is pinned in tests/test_latent_window.py)
                if kind == "u64":
                    first = (1 << 40) + 4096 * 7 + (residue if form == "full" else 0)
                    arr = from_latents([first + x for x in rel], np.uint64); kw = dict(mode=1, delta=1, level=level); tiers = (tier, None)
                elif kind == "d1-u32":
                    arr = from_latents(integrate(rel, 1, [1 << 31], 32), np.uint32); kw = dict(mode=1, delta=2, delta_order=1, level=level); tiers = (tier, None)
                else:
                    first = 40000 if form == "compact" else 20000 + residue
                    m0 = (1 << 63) // TIER_BASE + 1000
                    m = [m0 + int(x) for x in rng.integers(-50, 51, n)]
                    arr = from_latents([mm * TIER_BASE + first + x for mm, x in zip(m, rel)], np.int64)
                    kw = dict(mode=F.MODE_INT_MULT, mode_u64=TIER_BASE, delta=1, level=level); tiers = ("direct", tier)
                rows.append(_row(f"e-{kind}-{form}{R}-res{residue}-lat{n_lat}-L{level}-{r}-{tier}", arr, kw, r, "e", tiers=tiers))
    return rows


@functools.lru_cache(maxsize=None)
def rows_never():
    """Chunks that never speculate: a lookback delta, and more than 256 bins."""
    n = N_BIG
    base = np.random.default_rng(40).integers(-(1 << 40), 1 << 40, 365)
    periodic = (base[np.arange(n) % 365] + np.random.default_rng(4).integers(-3, 4, n)).astype(np.int64)
    ramp = (np.arange(20000) * 3 + np.random.default_rng(6).integers(0, 50, 20000)).astype(np.uint32)
    return [_row("n-int64-lookback-never", periodic, dict(mode=1, delta=3), "never", "n"),
            _row("n-uint32-level12-n20000-never", ramp, dict(mode=1, delta=2, delta_order=1, level=12), "never", "n")]


def all_rows():
    return rows_a() + rows_b() + rows_c() + rows_d() + rows_e() + rows_never()


@functools.lru_cache(maxsize=None)
def analysis_of(name):
    r = BY_NAME()[name]
    return analyse(r.arr, r.kw, r.pages)


@functools.lru_cache(maxsize=None)
def BY_NAME():
    rows = all_rows()
    out = {r.name: r for r in rows}
    assert len(out) == len(rows), "row names repeat"
    return out


def config_key(row):
    """What rows must share to share a call: the config (a call has one) and the entry point."""
    return (tuple(sorted(row.kw.items())), row.paging is not None)
