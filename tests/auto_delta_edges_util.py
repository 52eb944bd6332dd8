"""The row table of the Auto delta edge tests (test_auto_delta_model.py on the CPU, test_gpu_auto_delta_edges.py on the device).

Every row is a small deterministic chunk named after the edge of DeltaSpec::Auto resolution it sits on -- the shape of the sample, an exact
tie between two size estimates, a sequence of estimates whose first non-improvement is not its minimum, a lookback that is kept or
overtaken, a sample that must be taken from ordered primary latents, a level that changes the histogram the estimates come from.  A row
carries a claim about the ORACLE's nine estimates and decision (oracle_lib.auto_delta_costs) that certifies it sits on its edge -- a row
that does not reach its edge fails test_auto_delta_model.py, it does not quietly test something else -- and the wrong readings
(auto_delta_model.VARIANTS) that must change what is predicted for it.

The estimates c[0..9): c[0] no delta, c[1] lookback without its penalty of sample_n / 4, c[1 + k] consecutive order k.  The tie rows were
found by search over short running sums of small noise and are written out number by number; an estimate is a whole number of bytes, so
ties are common in short chunks and exact by construction in incompressible ones (a latent and a delta moment both cost the type's width).

`lookback + penalty == no delta` needs a sample length divisible by 4 (the penalty's fraction); the row lb_tie_u64_n80 has one, of 80
latents: a short pattern repeated exactly, where consecutive deltas are no improvement either, so the strict comparison alone decides.
The gate `no-delta cost > penalty` has no row: below it a lookback cost plus the penalty cannot be an improvement, so it changes nothing."""
import functools
from collections import namedtuple

import numpy as np

import auto_delta_model as M
import oracle_lib as O

Row = namedtuple("Row", "name edge arr kw claim variants")
_ROWS = []
DEFAULT = dict(level=8, mode=O.MODE_AUTO, mode_f64=0.0, mode_u64=0)   # oracle_lib.make_config / pcodec_amd._lib.make_config keywords; DeltaSpec::Auto always


def row(name, edge, variants=(), **kw):
    def deco(fn):
        _ROWS.append((name, edge, fn, dict(DEFAULT, **kw), tuple(variants))); return fn
    return deco


def cums(r, k, dt):
    """the k-th running sum of r, wrapping at the type's width"""
    x = np.asarray(r).astype(dt)
    for _ in range(k): x = np.cumsum(x, dtype=dt)
    return x


def noise012(n, seed): return np.random.default_rng(seed).integers(0, 3, n)


def stops_at(dec, k): return dec == ((M.CONSECUTIVE, k, 0) if k else (M.NONE, 0, 0))


def decreasing_to(c, k): return all(c[1 + j] < (c[j] if j > 1 else c[0]) for j in range(1, k + 1))


def with_penalty(sn, c): return np.float32(c[1] + np.float32(0.25) * np.float32(sn))


# ------------------------------------------------------------ (a) the shape of the sample ------------------------------------------------------------
def shaped(n, dt, smooth_inside, seed=3):
    """smooth (a ramp of small steps, in sample order) at exactly the sampled positions and full-width noise everywhere else, or the reverse"""
    rng = np.random.default_rng(seed); info = np.iinfo(dt)
    pos = M.sample_positions(n)
    noise = rng.integers(0, int(info.max) + 1, n, dtype=np.uint64).astype(dt)
    ramp = (1000 + 7 * np.arange(n, dtype=np.uint64) + rng.integers(0, 4, n).astype(np.uint64)).astype(dt)
    inside = np.zeros(n, bool); inside[pos] = True
    return np.where(inside == smooth_inside, ramp, noise).astype(dt)


for _n in (9, 10, 11, 199, 200, 201, 7649, 7650, 7651, 15649, 15650):
    _groups = 0 if _n < 10 else 1 if _n < 7650 else 2 if _n < 15650 else 3
    _named = ["stride_without_max"] if _groups == 1 else []

    @row(f"shape_n{_n}_smooth_inside", f"n = {_n}: {_groups} group(s); a ramp at the sampled positions, noise everywhere else", _named)
    def _(n=_n, groups=_groups):
        sn = M.sample_n(n)
        return shaped(n, np.uint32, True), lambda s, c, d: s == sn == groups * min(n, 200) and (n < 199 or (stops_at(d, 1) and c[2] < c[0]))

    if _n >= 200:
        @row(f"shape_n{_n}_noise_inside", f"n = {_n}: {_groups} group(s); noise at the sampled positions, a ramp everywhere else", _named)
        def _(n=_n):
            return shaped(n, np.uint32, False), lambda s, c, d: s == M.sample_n(n) and stops_at(d, 0) and c[0] == c[2] == c[3]


@row("shape_n1048576_walk_u64", "n = 2^20: 132 groups, 26400 latents -- trial encodes on histogram tiers no 2^18 chunk reaches")
def _():
    rng = np.random.default_rng(20)
    a = (np.uint64(1 << 40) + np.cumsum(rng.integers(0, 1000, 1 << 20)).astype(np.uint64))
    return a, lambda s, c, d: s == 26400 and c[2] < with_penalty(s, c) < c[0] and stops_at(d, 1)


_NARROW = {
    # (type, n): numbers.  Ten numbers: an order-7 trial has three latents; the lookback trial's window of 16 is longer than the sample.
    "narrow_u8_n10_sums": (np.uint8, [3, 9, 19, 34, 55, 82, 116, 158, 208, 11]),
    "narrow_u8_n17_period": (np.uint8, [7, 200, 31, 7, 201, 31, 8, 200, 32, 7, 200, 31, 9, 200, 31, 7, 202]),
    "narrow_u16_n10_ramp": (np.uint16, [100, 1100, 2101, 3100, 4102, 5100, 6103, 7100, 8101, 9100]),
    "narrow_u16_n17_cubic": (np.uint16, [i * i * i * 9 + i * 5 for i in range(17)]),
}
for _name, (_dt, _vals) in _NARROW.items():
    @row(_name, f"{np.dtype(_dt).name}, n = {len(_vals)}: a sample shorter than the lookback window and barely longer than the orders")
    def _(dt=_dt, vals=_vals): return np.array(vals, dtype=dt), lambda s, c, d, n=len(vals): s == n


# ------------------------------------------------------------ (b) ties and strictness ------------------------------------------------------------
@row("tie_noop_order1_noise_u32", "no delta == order 1 (== every order): incompressible u32, the decision stays at no delta", ["non_strict"])
def _():
    a = np.random.default_rng(1).integers(0, 1 << 32, 30000, dtype=np.uint64).astype(np.uint32)
    return a, lambda s, c, d: s == 800 and c[0] == c[2] == c[8] and stops_at(d, 0)


@row("tie_noop_order1_sum7_u32", "no delta == order 1 with order 7 seven times smaller: the seventh running sum of {0, 1, 2}", ["non_strict", "global_minimum"])
def _():
    return cums(noise012(30000, 5), 7, np.uint32), lambda s, c, d: c[0] == c[2] and c[8] * 7 < c[0] and stops_at(d, 0)


_TIES = {   # order k == order k + 1 behind estimates that all improved: (type, numbers); k = 1, 3, 5 inside a wave, k = 2, 4, 6 on a wave boundary
    1: (np.uint32, [1, 5, 16, 41, 91, 181, 331, 567, 922, 1437, 2161, 3152, 4478]),
    2: (np.uint32, [0, 1, 6, 20, 51, 110, 211, 372, 615, 967, 1460, 2131, 3022, 4180, 5657, 7510, 9802, 12603]),
    3: (np.uint16, [2, 10, 30, 71, 145, 269, 466, 767, 1212, 1851, 2746]),
    4: (np.uint16, [2, 18, 88, 310, 883, 2163, 4734, 9499, 17796, 31541]),
    5: (np.uint16, [1, 7, 28, 84, 210, 461, 917, 1688, 2920, 4801, 7567, 11508, 16975, 24388]),
    6: (np.uint32, [7, 50, 210, 668, 1775, 4147, 8786, 17233, 31754, 55565, 93102, 150338, 235152, 357753, 531163, 771764, 1099916, 1540648]),
}
for _k, (_dt, _vals) in _TIES.items():
    @row(f"tie_order{_k}_order{_k + 1}", f"order {_k} == order {_k + 1} {'inside a wave' if _k % 2 else 'on a wave boundary'}: the decision stays at {_k}", ["non_strict"])
    def _(k=_k, dt=_dt, vals=_vals):
        return np.array(vals, dtype=dt), lambda s, c, d: c[1 + k] == c[2 + k] and stops_at(d, k)


@row("lb_tie_u64_n80", "lookback + penalty == no delta (220 + 80 / 4 == 240): the lookback is not taken", ["non_strict", "lookback_without_penalty"])
def _():
    pat = np.array([486, 502, 315, 370, 15, 278, 158, 120, 230], dtype=np.uint64)
    return pat[np.arange(80) % 9], lambda s, c, d: s == 80 and with_penalty(s, c) == c[0] and c[2] >= c[0] and stops_at(d, 0)


# ------------------------------------------------------------ (c) estimates that are not convex ------------------------------------------------------------
def quad_ramp(n, mult, mod=None):
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"): q = (i * (i + np.uint64(1)) // np.uint64(2)) * np.uint64(mult)
    return q % np.uint64(mod) if mod else q


@row("nonconvex_stop0_u32", "x = 0x9E3779B1 * i(i+1)/2 mod 2^32: no delta == order 1, order 2 a seventeenth of them; the decision is no delta", ["global_minimum", "non_strict"])
def _():
    return quad_ramp(30000, 0x9E3779B1).astype(np.uint32), lambda s, c, d: c[0] == c[2] and c[3] * 2 <= c[0] and stops_at(d, 0)


@row("quad_ramp_40503_u32", "the same ramp with multiplier 40503: order 1 is an improvement and order 2 is reached")
def _():
    return quad_ramp(30000, 40503).astype(np.uint32), lambda s, c, d: stops_at(d, 2) and c[3] * 2 <= c[2]


for _k in (2, 3, 4, 5):
    @row(f"nonconvex_stop{_k}_u64", f"the {_k}-th running sum of a quadratic ramp mod 2^20: order {_k + 1} is worse than order {_k}, order {_k + 2} at most half of it"
         + (" -- the stop is the last order of a wave" if _k % 2 == 0 else " -- the stop is inside a wave"), ["global_minimum"])
    def _(k=_k):
        # (k = 5 in a chunk of 1000 numbers and mod 2^16: at 30000 the sums' carries leave order 7 above half of order 5)
        q = quad_ramp(30000, 0x9E3779B1, 1 << 20) if k < 5 else quad_ramp(1000, 0x9E3779B1, 1 << 16)
        return cums(q, k, np.uint64), lambda s, c, d: decreasing_to(c, k) and c[2 + k] > c[1 + k] and c[3 + k] * 2 <= c[1 + k] and stops_at(d, k)


for _k in range(1, 8):
    @row(f"monotone_stop{_k}_u64", f"the {_k}-th running sum of {{0, 1, 2}}: every order up to {_k} an improvement, " + ("order 7 the strict minimum" if _k == 7 else f"order {_k + 1} none"),
         [])
    def _(k=_k):
        def claim(s, c, d):
            return s == 200 and decreasing_to(c, k) and stops_at(d, k) and (c[8] < min(c[:8]) if k == 7 else c[2 + k] >= c[1 + k])
        return cums(noise012(1000, 40 + k), k, np.uint64), claim


# ------------------------------------------------------------ (d) lookback ------------------------------------------------------------
def periodic(n, dt, seed=0, period=32, shift=10):
    """a ramp of i << shift plus 24-bit values repeated every `period` numbers plus noise of -3..3: the lookback finds the copy, a consecutive
    delta sees 24-bit differences"""
    rng = np.random.default_rng(seed); pat = rng.integers(0, 1 << 24, period)
    return ((np.arange(n) << shift) + pat[np.arange(n) % period] + rng.integers(-3, 4, n) + 8).astype(dt)


@row("lookback_kept_u32_n30000", "lookback chosen and kept: order 1 is an improvement on no delta and none on lookback + penalty; the window log is 15 from n = 30000, 10 from the sample",
     ["window_from_sample"])
def _():
    def claim(s, c, d): return s == 800 and with_penalty(s, c) < c[2] < c[0] and d == (M.LOOKBACK, 0, 15) and M.window_log(s) == 10
    return periodic(30000, np.uint32), claim


@row("lookback_kept_i64_n3000", "lookback chosen and kept in a chunk of one group: window log 12 from n = 3000, 8 from the sample", ["window_from_sample"])
def _():
    return periodic(3000, np.int64, seed=8), lambda s, c, d: s == 200 and with_penalty(s, c) < min(c[0], c[2]) and d == (M.LOOKBACK, 0, 12) and M.window_log(s) == 8


@row("lookback_overtaken_by_order1_u32", "lookback + penalty improves on no delta, order 1 on the lookback, order 2 not: the plan loses its window log")
def _():
    return cums(noise012(30000, 5), 1, np.uint32), lambda s, c, d: with_penalty(s, c) < c[0] and c[2] < with_penalty(s, c) and d == (M.CONSECUTIVE, 1, 0)


@row("lookback_overtaken_by_order2_u32", "lookback + penalty improves on no delta, orders 1 and 2 on the lookback: the plan loses its window log")
def _():
    return cums(noise012(30000, 5), 2, np.uint32), lambda s, c, d: with_penalty(s, c) < c[0] and c[3] < c[2] < with_penalty(s, c) and d == (M.CONSECUTIVE, 2, 0)


@row("lookback_only_without_penalty_u32", "the lookback's estimate is below no delta, with its penalty it is not", ["lookback_without_penalty"])
def _():
    a = np.random.default_rng(1).integers(0, 1 << 32, 30000, dtype=np.uint64).astype(np.uint32)
    a[2::8] = a[0::8]                                                           # one number in eight is a copy from two back: worth four bits per number, the penalty is two and the lookbacks cost too
    return a, lambda s, c, d: c[1] < c[0] <= with_penalty(s, c)


# ------------------------------------------------------------ (e) the sample is latents, not numbers ------------------------------------------------------------
def mode_is(arr, kw, kind): return O.split_latents(arr, O.make_config(**kw))[2] == kind


CLASSIC, INT_MULT, FLOAT_MULT, FLOAT_QUANT = 0, 1, 2, 3
for _dt in (np.int32, np.int64):
    for _mode in ("given", "auto"):
        @row(f"latents_{np.dtype(_dt).name}_ramp_through_zero_{_mode}", "a signed ramp through zero: smooth as ordered latents, two far ends as raw bits", mode=O.MODE_CLASSIC if _mode == "given" else O.MODE_AUTO)
        def _(dt=_dt):
            n = 3000; rng = np.random.default_rng(11)
            return ((np.arange(n) - 90) * 5 + rng.integers(0, 3, n)).astype(dt), lambda s, c, d: stops_at(d, 1) and c[2] < c[0]

for _dt in (np.float32, np.float64):
    for _mode in ("given", "auto"):
        @row(f"latents_{np.dtype(_dt).name}_ramp_through_zero_{_mode}", "a float ramp through -0.0 and +0.0: ordered latents mirror the negative half", mode=O.MODE_CLASSIC if _mode == "given" else O.MODE_AUTO)
        def _(dt=_dt):
            n = 3000; rng = np.random.default_rng(12)
            k = (np.arange(n) - 90) * 3 + rng.integers(0, 2, n)
            u = {np.float32: np.uint32, np.float64: np.uint64}[dt]; bits = np.dtype(dt).itemsize * 8
            a = (np.abs(k).astype(u) | np.where(k < 0, 1 << (bits - 1), 0).astype(u)).view(dt)   # subnormals counted up from zero, both signs
            a[90] = dt(0.0); a[89] = dt(-0.0)
            return a, lambda s, c, d: stops_at(d, 1) and c[2] < c[0]

for _mode in ("given", "auto"):
    @row(f"latents_int_mult_{_mode}", "int mult: the sample is the primary (a running sum), the secondary is noise" + (" in a tenth of the numbers" if _mode == "auto" else ""),
         **(dict(mode=O.MODE_TRY_INT_MULT, mode_u64=1000) if _mode == "given" else dict(mode=O.MODE_AUTO)))
    def _(mode=_mode):
        n = 4000; rng = np.random.default_rng(13)
        p = cums(noise012(n, 14), 2, np.uint64)
        r = rng.integers(0, 1000, n) if mode == "given" else np.where(rng.integers(0, 10, n) == 0, rng.integers(0, 1000, n), 0)
        a = (p * np.uint64(1000) + r.astype(np.uint64)).astype(np.uint32)
        kw = dict(mode=O.MODE_TRY_INT_MULT, mode_u64=1000) if mode == "given" else dict(mode=O.MODE_AUTO)
        return a, lambda s, c, d: mode_is(a, kw, INT_MULT) and stops_at(d, 2)

    @row(f"latents_float_mult_{_mode}", "float mult: decimals k / 100 with k a running sum; the sample is k",
         **(dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01) if _mode == "given" else dict(mode=O.MODE_AUTO)))
    def _(mode=_mode):
        a = (100000 + cums(noise012(4000, 15), 1, np.int64)) / 100.0
        kw = dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01) if mode == "given" else dict(mode=O.MODE_AUTO)
        return a, lambda s, c, d: mode_is(a, kw, FLOAT_MULT) and stops_at(d, 1)

    @row(f"latents_float_quant_{_mode}", "float quant: f32 with 12 low mantissa bits clear; the sample is the quantised part",
         **(dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=12) if _mode == "given" else dict(mode=O.MODE_AUTO)))
    def _(mode=_mode):
        k = (0x3F800000 >> 12) + cums(noise012(4000, 16), 1, np.int64) * 3
        a = (k.astype(np.uint32) << np.uint32(12)).view(np.float32)
        kw = dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=12) if mode == "given" else dict(mode=O.MODE_AUTO)
        return a, lambda s, c, d: mode_is(a, kw, FLOAT_QUANT) and stops_at(d, 1)


def jumpy(n=30000):
    """the second running sum of {0, 1, 2} with a step of 2^16 every fifty numbers or so: one wide bin (level 0) pays a bit per number for the
    second difference's two-sided steps, 16 bins and more set them aside"""
    rng = np.random.default_rng(7)
    base = cums(rng.integers(0, 3, n), 2, np.uint64)
    return base + np.cumsum((rng.integers(0, 50, n) == 0).astype(np.uint64) << np.uint64(16))


for _lv in (0, 4, 8, 12):
    @row(f"level{_lv}_jumpy_u64", f"level {_lv}: the trials' histogram size comes from the chunk's n = 30000 ({'one bin: order 1' if _lv == 0 else 'order 2'})", level=_lv)
    def _(lv=_lv): return jumpy(), lambda s, c, d: stops_at(d, 1 if lv == 0 else 2)


@row("latents_i32_noise_level0", "level 0, signed noise around zero: one bin of 11 bits as ordered latents (no delta), of 32 bits as raw bits (order 1)", ["raw_bits"], level=0)
def _():
    return np.random.default_rng(7).integers(-1024, 1024, 1000).astype(np.int32), lambda s, c, d: stops_at(d, 0) and c[0] < c[2]


# -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows():
    out = []
    for name, edge, fn, kw, variants in _ROWS:
        arr, claim = fn()
        out.append(Row(name, edge, np.ascontiguousarray(arr), kw, claim, variants))
    assert len({r.name for r in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def by_name(): return {r.name: r for r in rows()}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(sample length, the nine estimates, the decision) of a row by the oracle"""
    r = by_name()[name]
    return O.auto_delta_costs(r.arr, O.make_config(**r.kw))


def config_key(kw): return tuple(sorted(kw.items()))


def groups():
    """the rows by config, for one batched call each: [(kw, [row])]; the 2^20 row travels alone"""
    out = {}
    for r in rows(): out.setdefault((config_key(r.kw), r.arr.size > 30000), []).append(r)
    return [(dict(k[0]), v) for k, v in out.items()]


def batch_call():
    """The chunks of one batched call under the default config, in shuffled order: [(name, array)].  Every stop 0..7, a lookback kept and one
    overtaken -- so that every deeper wave runs over a scattered, shrinking sub-list --, chunks below 10 numbers between them, chunks of
    equal n and different width (one pooled index list, samples of 10 and 80 or 200 and 1600 bytes), a u8 sample of 10 bytes directly in
    front of a u64 one (the next sample starts 16 bytes on, not 10), signed, float and two-variable chunks, and one row at three places."""
    r = by_name(); rng = np.random.default_rng(66)
    names = ["nonconvex_stop0_u32", "lookback_kept_u32_n30000", "lookback_overtaken_by_order1_u32", "tie_order2_order3", "tie_order4_order5", "tie_order6_order7",
             "latents_int_mult_auto", "latents_float_mult_auto", "latents_float_quant_auto", "latents_int64_ramp_through_zero_auto", "latents_float32_ramp_through_zero_auto",
             "nonconvex_stop3_u64", "shape_n15650_smooth_inside", "lb_tie_u64_n80", "shape_n9_smooth_inside"] + [f"monotone_stop{k}_u64" for k in range(1, 8)]
    chunks = [[(n, r[n].arr)] for n in names]
    chunks += [[("monotone_stop5_u64", r["monotone_stop5_u64"].arr)] for _ in range(2)]
    chunks.append([("five_u64", np.arange(5, dtype=np.uint64) * 3)])
    chunks.append([("noise_u8_n1000", rng.integers(0, 256, 1000).astype(np.uint8))])                          # n = 1000 like the u64 rows above
    chunks.append([("narrow_u8_n10_sums", r["narrow_u8_n10_sums"].arr), ("sums_u64_n10", cums([1, 0, 2, 2, 1, 0, 1, 2, 0, 1], 3, np.uint64))])   # the pair stays together
    order = rng.permutation(len(chunks))
    return [c for i in order for c in chunks[i]]


WRAPPED = (("lookback_kept_u32_n30000", [9999, 1, 20000]), ("lookback_overtaken_by_order2_u32", [7, 14996, 14997]))   # one wrapped chunk each, in these pages
