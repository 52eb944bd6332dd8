"""The case table of the Auto mode edge tests (test_auto_mode_model.py on the CPU, test_gpu_auto_edges.py on the device).

Every case is a small deterministic array built so that ONE gate of ModeSpec::Auto detection sits on its threshold: chosen values at
exactly the positions the mode sample draws (oracle_lib.mode_sample_indices, in draw order) and unrelated filler everywhere else.  A case
carries the gate it sits on, a claim about the model's record that says so (`claim(record)` must hold), and the wrong readings of the
gate (auto_mode_model.VARIANTS) that must change its record.  Sizes: a sample of S numbers needs n = 10 + 40 * (S - 10); only the
capacity cases (a sample of 6656 / 6657 numbers) are large.

Euclid with a zero weight sum (center_sample_base dividing 0 by 0) has no case: the picked value is one of the pair GCDs themselves, a
pair's GCD g is a remainder of its chain and every remainder kept is above hi * 2^-(PRECISION_BITS - 6) (is_approx_zero returns None
otherwise), so for the pair that produced the pick hi / g < 2^(PRECISION_BITS - 6) < 2^PRECISION_BITS and lo / g >= 1: its two numbers
have multipliers that are not 0 and have precision to spare, and the weight sum is positive on every sample that passes the Euclid gates.
test_auto_mode_model.py asserts the positive weight sum on every case with a Euclid candidate.
"""
import functools
from collections import namedtuple

import numpy as np

import auto_mode_model as M
import oracle_lib as O

Case = namedtuple("Case", "name gate arr claim variants both_auto")
_CASES = []


def n_for_sample(s): return 10 + 40 * (s - 10)


def place(n, dtype, sample, seed=1):
    """`sample` at the sampled positions of an n-number chunk in draw order; a few unrelated values everywhere else"""
    idx = O.mode_sample_indices(n)
    assert len(sample) == len(idx), (len(sample), len(idx))
    dt = np.dtype(dtype); rng = np.random.default_rng(seed)
    if dt.kind == "f": pool = (np.float64([1.2345, -7.75, 3.0e-3, 911.0625, 0.3]) * 1.0001).astype(dt)
    else: pool = np.array([3, 11, 12345 % (1 << (dt.itemsize * 8 - 1)), 77, 101], dtype=dt)
    arr = pool[rng.integers(0, len(pool), n)]
    arr[idx] = np.asarray(sample, dtype=dt)
    return arr


def case(name, gate, variants=(), both_auto=False):
    def deco(fn):
        _CASES.append((name, gate, fn, tuple(variants), both_auto)); return fn
    return deco


def _from_bits(bits, dt): return np.array(bits, dtype={4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]).view(dt)


FK = {np.float32: M.F32, np.float64: M.F64}

# ---------------------------------------------------------------- sizes ----------------------------------------------------------------
for _dt in (np.uint32, np.float32, np.float64):
    _nm = np.dtype(_dt).name

    @case(f"n9_{_nm}", "a chunk of 9 numbers has no sample")
    def _(dt=_dt): return (np.arange(9) * 8 + 8).astype(dt), lambda r: r["sample_n"] == 0 and r["route"] == "none"

    @case(f"n10_{_nm}", "a chunk of 10 numbers is its own sample")
    def _(dt=_dt): return (np.arange(10) * 24 + 8).astype(dt), lambda r: r["sample_n"] == 10 and r["route"] != "none"


def _cap_sample(dt, s, seed):
    rng = np.random.default_rng(seed)
    if dt == np.int64: return (rng.permutation(s).astype(np.int64) - s // 2) * 7919
    prec = FK[dt].prec; sh = prec - 15                         # all kept, >= sh trailing zeros, every shifted pattern distinct
    return _from_bits([((FK[dt].bias << prec) | (int(i) << sh)) for i in rng.permutation(s)], dt)


for _dt in (np.int64, np.float32, np.float64):
    _nm = np.dtype(_dt).name

    @case(f"cap_fits_{_nm}", "a sample of kAutoCap = 6656 numbers is decided on the device", both_auto=_dt != np.float64)
    def _(dt=_dt):
        full = lambda r: r["sample_n"] == M.AUTO_CAP and r["route"] in ("dev_int", "dev_float")
        if dt == np.int64: return place(265889, dt, _cap_sample(dt, 6656, 3)), full
        # floats: every number kept, and every float-quant key its own bucket: the first-appearance list is full
        return place(265889, dt, _cap_sample(dt, 6656, 3)), lambda r: full(r) and r["kept"] == 6656 and r["cands"]["quant"]["stage2"]["n_rare"] == 6656

    @case(f"cap_over_{_nm}", "a sample of 6657 numbers takes the host path")
    def _(dt=_dt): return place(265890, dt, _cap_sample(dt, 6657, 3)), lambda r: r["sample_n"] == M.AUTO_CAP + 1 and r["route"] == "host_size"


def _filtered(dt, good, n_bad):
    """a sample of len(good) + n_bad numbers of which the n_bad are filtered out (specials, subnormals, too large)"""
    K = FK[dt]
    inf = ((1 << (K.bits - 1 - K.prec)) - 1) << K.prec
    # NaN, +-inf, +-0, the largest and the smallest subnormal, one ulp above MAX_FOR_SAMPLING (both signs), the largest finite value (both signs)
    bad_bits = [K.mid - 1, inf, inf | K.mid, 0, K.mid, (1 << K.prec) - 1, 1, K.max_for_sampling + 1, K.mid | (K.max_for_sampling + 1), K.max_bits, K.mid | K.max_bits]
    bad = [bad_bits[i % len(bad_bits)] for i in range(n_bad)]
    both = list(good) + [K.from_bits(b) for b in bad]
    order = np.random.default_rng(9).permutation(len(both))
    return np.array(both, dtype=dt)[order]


for _dt in (np.float32, np.float64):
    _nm = np.dtype(_dt).name
    for _kept in (9, 10):
        @case(f"kept{_kept}_{_nm}", f"kept = {_kept}: the filtered sample is {'below' if _kept == 9 else 'at'} MIN_SAMPLE")
        def _(dt=_dt, kept=_kept):
            good = (np.arange(kept) * 3 + 5).astype(dt) * dt(0.125) * np.where(np.arange(kept) % 2, -1, 1).astype(dt)   # (negative numbers are kept as |x|)
            return place(n_for_sample(30), dt, _filtered(dt, good, 30 - kept)), lambda r: r["kept"] == kept and (r["route"] == "none") == (kept == 9)

    # ------------------------------------------------------------ float filter ------------------------------------------------------------
    @case(f"filter_edges_{_nm}", "|x| = smallest normal and MAX_FOR_SAMPLING are kept, largest subnormal and one ulp above are not", ["filter_lim_strict"])
    def _(dt=_dt):
        K = FK[dt]
        good = [K.from_bits(1 << K.prec), K.from_bits(K.mid | (1 << K.prec)), K.from_bits(K.max_for_sampling)] + [dt(-(3 + 2 * i) * 0.25) for i in range(7)]
        # (10 kept with MAX_FOR_SAMPLING among them: a strict limit keeps 9 and finds no sample at all)
        return place(n_for_sample(21), dt, _filtered(dt, good, 11)), lambda r: r["kept"] == 10 and r["route"] == "dev_float"


# ------------------------------------------------------------ trailing zeros ------------------------------------------------------------
def _tz_sample(dt, kept, n_tz, tz, seed=4):
    """kept numbers in [1, 2): n_tz of them with exactly `tz` trailing zero bits, the others with none"""
    K = FK[dt]; rng = np.random.default_rng(seed); out = []
    for i in range(kept):
        m = int(rng.integers(0, 1 << (K.prec - 8))) << 8
        m = (m | (1 << tz)) & ~((1 << tz) - 1) if i < n_tz else m | 1
        out.append((K.bias << K.prec) | m)
    return _from_bits([out[i] for i in rng.permutation(kept)], dt)


for _dt in (np.float32, np.float64):
    _nm = np.dtype(_dt).name

    @case(f"tz4_{_nm}", "trailing zeros: 4 is not interesting", ["tz_gate_4"])
    def _(dt=_dt): return place(n_for_sample(20), dt, _tz_sample(dt, 20, 10, 4)), lambda r: r["tz5"] == 0 and "tz" not in r["cands"]

    @case(f"tz5_{_nm}", "trailing zeros: 5 is interesting, and 10 of 20 are enough")
    def _(dt=_dt): return place(n_for_sample(20), dt, _tz_sample(dt, 20, 10, 5)), lambda r: r["tz5"] == r["required"] == 10 and "tz" in r["cands"]

    for _kept, _req in ((21, 11), (22, 11), (12, 10)):
        @case(f"tz5_required_kept{_kept}_{_nm}", f"tz5 = required = {_req} of {_kept}")
        def _(dt=_dt, kept=_kept, req=_req): return place(n_for_sample(kept), dt, _tz_sample(dt, kept, req, 6)), lambda r: r["tz5"] == r["required"] == req and "tz" in r["cands"]

        @case(f"tz5_below_kept{_kept}_{_nm}", f"tz5 = required - 1 = {_req - 1} of {_kept}", ["required_floor"] if _kept == 21 else [])
        def _(dt=_dt, kept=_kept, req=_req): return place(n_for_sample(kept), dt, _tz_sample(dt, kept, req - 1, 6)), lambda r: r["tz5"] == r["required"] - 1 == req - 1 and "tz" not in r["cands"]

    @case(f"tz_powers_of_two_{_nm}", "powers of two: the histogram clamps at the mantissa width, nothing to subtract from the exponent")
    def _(dt=_dt):
        s = np.array([2.0 ** (i % 13 - 6) for i in range(24)], dtype=dt)
        return place(n_for_sample(24), dt, s), lambda r: r["hist"][-1] == 24 and r["k"] == -6 and r["n_ints"] == 24

    for _short in (0, 1):
        @case(f"n_ints_{'below' if _short else 'at'}_required_{_nm}", f"n_ints = required{' - 1' if _short else ''}: a number 2^k * 2^bits or above is no integer of the sample")
        def _(dt=_dt, short=_short):
            K = FK[dt]
            small = [dt(1.0 + (2 * i + 1) * 2.0 ** -10) for i in range(10 - short)]                  # k = -10
            big = [dt(2.0 ** (K.bits - 10 + i)) for i in range(short)]                                # tz >= 5, but e >= k + bits
            odd = [K.from_bits((K.bias << K.prec) | (2 * i + 1)) for i in range(10)]                 # no trailing zeros, not a multiple of 2^-10
            s = np.array(small + big + odd, dtype=dt)[np.random.default_rng(2).permutation(20)]
            return place(n_for_sample(20), dt, s), lambda r: r["tz5"] == 10 == r["required"] and r["n_ints"] == 10 - short and ("tz" in r["cands"]) == (not short)


# --------------------------------------------------------------- GCD table ---------------------------------------------------------------
def _triples(gcds, n_triples, rng, hi):
    """a sample of n_triples triples: triple j is (a, a + g, a + 2g) for g = gcds[j] (GCD exactly g), and far-apart numbers with GCD 1 beyond the list"""
    out = []
    for j in range(n_triples):
        if j < len(gcds):
            g = gcds[j]; a = int(rng.integers(0, hi - 2 * g)); t = [a, a + g, a + 2 * g]
        else:                                                                       # (b and 2b + 1 have no common divisor)
            b = int(rng.integers(hi // 16, hi // 8)); a = int(rng.integers(0, hi // 2)); t = [a, a + b, a + 2 * b + 1]
        out += [t[i] for i in rng.permutation(3)]
    return out


def _home(v, shift, slots): return (((int(v) * 0x9E3779B97F4A7C15) & M._M64) >> shift) & (slots - 1)


def _values_with_home(slot, shift, slots, count, start):
    v = np.arange(start, start + 4000000, dtype=np.uint64)
    with np.errstate(over="ignore"): h = ((v * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(shift)) & np.uint64(slots - 1)
    got = v[h == slot][:count]
    assert len(got) == count
    return [int(x) for x in got]


def _gcd_sample(dt, sample_n, gcds, seed=6, hi=None):
    rng = np.random.default_rng(seed)
    hi = hi or (1 << 31)
    s = _triples(gcds, sample_n // 3, rng, hi) + [5] * (sample_n % 3)
    return place(n_for_sample(sample_n), dt, np.array(s, dtype=np.uint64).astype(dt))


def _as_float_ints(dt, sample_n, gcds):
    """the same triples as whole floats below 2^18: every one has >= 5 trailing zeros, k = 0 and the sample's integers are the numbers"""
    rng = np.random.default_rng(6)
    s = _triples(gcds, sample_n // 3, rng, 1 << 18) + [5] * (sample_n % 3)
    s = [x + 1 for x in s]                                                            # (no zero: it would be filtered out)
    return place(n_for_sample(sample_n), dt, np.array(s, dtype=np.float64).astype(dt))


@case("gcd_once_and_twice_u32", "a GCD seen in one triple is not listed, one seen in two is (and can win)", ["drop_count_two"])
def _(): return _gcd_sample(np.uint32, 90, [1009, 2003, 2003]), lambda r: r["gcd"]["n_distinct"] == 2 and r["gcd"]["n_listed"] == 1 and r["mode"] == ("int_mult", 2003)


for _cnt in (192, 193):
    @case(f"gcd_listed_{_cnt}_u32", f"{_cnt} values seen twice: {'the list is full' if _cnt == 192 else 'the list overflows'}", ["drop_count_two"] if _cnt == 192 else [])
    def _(cnt=_cnt):
        g = [1000 + 3 * j for j in range(cnt)]
        return _gcd_sample(np.uint32, 1169, g + g), lambda r: r["gcd"]["n_listed"] == cnt and r["route"] == ("dev_int" if cnt == 192 else "host_overflow")

    @case(f"gcd_listed_{_cnt}_f32", f"{_cnt} values seen twice among the trailing-zeros integers of floats")
    def _(cnt=_cnt):
        g = [100 + 3 * j for j in range(cnt)]
        return _as_float_ints(np.float32, 1169, g + g), lambda r: r["gcd"]["n_listed"] == cnt and r["route"] == ("dev_float" if cnt == 192 else "host_overflow")

for _cnt in (2047, 2048):
    @case(f"gcd_distinct_{_cnt}_u32", f"{_cnt} distinct values: {'the last free slot stays free' if _cnt == 2047 else 'the table is full'}")
    def _(cnt=_cnt):
        arr = _gcd_sample(np.uint32, 6656, [5000 + j for j in range(cnt)])
        return arr, lambda r: r["gcd"]["n_distinct"] == cnt and r["gcd"]["n_listed"] == 0 and r["route"] == ("dev_int" if cnt == 2047 else "host_overflow") and r["mode"][0] == "classic"


@case("gcd_probe_wraps_u32", "four values whose home slot is 2047: the probe sequence wraps to slot 0")
def _():
    g = _values_with_home(M.GCD_SLOTS - 1, 53, M.GCD_SLOTS, 4, 1000)
    assert all(_home(v, 53, M.GCD_SLOTS) == M.GCD_SLOTS - 1 for v in g)
    return _gcd_sample(np.uint32, 90, g + g), lambda r: r["gcd"]["n_listed"] == 4


@case("gcd_once_and_twice_f32", "the same among the trailing-zeros integers of floats: the value seen twice becomes the base's integer factor", ["drop_count_two"])
def _(): return _as_float_ints(np.float32, 90, [1009, 2003, 2003]), lambda r: r["gcd"]["n_distinct"] == 2 and r["gcd"]["n_listed"] == 1 and r["int_base"] == 2003


@case("gcd_probe_wraps_f32", "four values whose home slot is 2047 among the trailing-zeros integers of floats")
def _():
    g = _values_with_home(M.GCD_SLOTS - 1, 53, M.GCD_SLOTS, 4, 1000)
    return _as_float_ints(np.float32, 90, g + g), lambda r: r["gcd"]["n_listed"] == 4 and r["route"] == "dev_float"


for _cnt in (2047, 2048):
    @case(f"gcd_distinct_{_cnt}_f32", f"{_cnt} distinct values among the trailing-zeros integers of a full-capacity float sample")
    def _(cnt=_cnt):
        arr = _as_float_ints(np.float32, 6656, [5000 + j for j in range(cnt)])
        return arr, lambda r: r["kept"] == M.AUTO_CAP and r["gcd"]["n_distinct"] == cnt and r["route"] == ("dev_float" if cnt == 2047 else "host_overflow")


@case("gcd_two_to_63_u64", "u64 triples whose GCD is 2^63")
def _():
    rng = np.random.default_rng(8); s = []
    for j in range(20):
        a = int(rng.integers(0, 1 << 62))
        s += [a, a + (1 << 63), a] if j < 4 else [a, a + 1, a + 2]
    return place(n_for_sample(60), np.uint64, np.array(s, dtype=np.uint64)), lambda r: (1 << 63, 4) in r["gcd"]["counts"] and "int" in r["cands"]


for _dt, _base in ((np.int16, 12), (np.uint16, 12), (np.int8, 5), (np.uint8, 5)):
    @case(f"narrow_{np.dtype(_dt).name}", f"multiples of {_base} in a {np.dtype(_dt).itemsize * 8}-bit type")
    def _(dt=_dt, base=_base):
        info = np.iinfo(dt); rng = np.random.default_rng(12)
        q = rng.permutation(np.arange(info.min // base + 1, info.max // base))[:60] if info.bits == 16 else rng.integers(info.min // base + 1, info.max // base, 60)
        return place(n_for_sample(60), dt, (q * base).astype(dt)), lambda r, b=base: r["cands"]["int"]["base"] % b == 0


# ----------------------------------------------------------------- Euclid -----------------------------------------------------------------
def _pairs(dt, gcds, kept, hi_factor=3):
    """a sample of `kept` numbers whose pair j is (3g, 2g) for g = gcds[j] (its approximate GCD is g exactly) and two equal numbers
    (no GCD) beyond the list; every number has an odd mantissa, so nothing here has trailing zeros"""
    out = []
    for j in range(kept // 2):
        if j < len(gcds): out += [dt(hi_factor) * dt(gcds[j]), dt(hi_factor - 1) * dt(gcds[j])]
        else: out += [dt(1.0 + (2 * j + 1) * 2.0 ** -20)] * 2
    out += [dt(1.5 + 2.0 ** -20)] * (kept % 2)
    return np.array(out, dtype=dt)


def _odd(dt, x):
    """x with the last mantissa bit set, so that 3x and 2x are exact and x has no trailing zeros"""
    K = FK[dt]; b = K.to_bits(dt(x))
    return K.from_bits(((b >> 3) << 3) | 1)


def _euclid_case(dt, gcds, kept): return place(n_for_sample(kept), dt, _pairs(dt, [_odd(dt, g) for g in gcds], kept))


for _dt in (np.float32, np.float64):
    _nm = np.dtype(_dt).name

    @case(f"euclid_n_g_at_need_{_nm}", "n_g = need = 2 of 20")
    def _(dt=_dt): return _euclid_case(dt, [0.3, 0.3], 20), lambda r: r["n_g"] == r["need"] == 2 and r["has_euclid"]

    @case(f"euclid_n_g_below_need_{_nm}", "n_g = need - 1 = 1 of 20", ["need_no_plus_one"])
    def _(dt=_dt): return _euclid_case(dt, [0.3], 20), lambda r: r["n_g"] == 1 and r["need"] == 2 and not r["has_euclid"]

    for _kept in (1000, 1001):
        @case(f"euclid_kept{_kept}_{_nm}", f"kept = {_kept}: need = {2 if _kept == 1000 else 3}, two pairs agree")
        def _(dt=_dt, kept=_kept): return _euclid_case(dt, [0.3, 0.3], kept), lambda r: r["kept"] == kept and r["need"] == (2 if kept == 1000 else 3) and r["has_euclid"] == (kept == 1000)

    # ten GCDs, need = 2: the percentile values are the sorted GCDs 1, 3 and 5
    for _which, _g in (("first", [1, 1, 2, 3, 4, 5, 6, 7, 8, 9]), ("second", [1, 2, 3, 3, 4, 5, 6, 7, 8, 9]), ("third", [1, 2, 3, 4, 5, 5, 6, 7, 8, 9]),
                       ("none", [1, 2, 3, 4, 5, 6, 7, 7, 8, 9])):
        @case(f"euclid_pick_{_which}_{_nm}", f"sim = need at the {_which} percentile and need - 1 before it", ["percentile_order"] if _which in ("first", "third") else [])
        def _(dt=_dt, which=_which, g=_g):
            want = {"first": [2, 1, 1], "second": [1, 2, 1], "third": [1, 1, 2], "none": [1, 1, 1]}[which]
            return _euclid_case(dt, [0.37 * x for x in g][::-1], 20), lambda r: r["n_g"] == 10 and r["sim"] == want and r["has_euclid"] == (which != "none")

    for _ng in (1, 2, 3, 8, 9, 64, 65):
        @case(f"euclid_sort_{_ng}_{_nm}", f"n_g = {_ng}: the sort network's power-of-two padding")
        def _(dt=_dt, ng=_ng):
            rng = np.random.default_rng(ng)
            g = [0.11 * (1.0 + 0.001 * int(x)) for x in rng.permutation(ng)]          # distinct, shuffled, all within 1 % of the middle ones' neighbours
            return _euclid_case(dt, g, max(2 * ng, 12)), lambda r: r["n_g"] == ng

    for _on in (1, 0):
        @case(f"euclid_window_{'on' if _on else 'inside'}_{_nm}", f"a GCD {'exactly on' if _on else 'one ulp inside'} the 1 % window of the pick", ["sim_nonstrict"] if _on else [])
        def _(dt=_dt, on=_on):
            K = FK[dt]; F = dt
            c = None
            for m in range(1 << (K.prec - 2), (1 << (K.prec - 2)) + 200000):          # a pick c whose lower window edge c - 0.01 * c is exact
                cand = K.from_bits((K.bias << K.prec) | m); w = F(F(0.01) * cand); y = F(cand - w)
                if F(cand - y) == w: c = cand; edge = y; break
            assert c is not None
            other = edge if on else K.from_bits(K.to_bits(edge) + 1)
            # four GCDs (pairs (2g, g): 2g is exact whatever g's last bit), sorted: other, c, 5, 9.  The percentile values are other (its own,
            # narrower window does not reach c), c and 5: only c can have a second GCD in its window
            s = _pairs(dt, [dt(5), c, other, dt(9)], 20, hi_factor=2)
            return place(n_for_sample(20), dt, s), lambda r: r["n_g"] == 4 and r["sim"] == [1, 1 if on else 2, 1] and r["has_euclid"] == (not on)


# ----------------------------------------------------------------- stage 2 -----------------------------------------------------------------
def _mult_sample(s_n, base, rng, dup=()):
    """s_n multiples of `base` with distinct quotients, then quotient copies: dup = ((position, copied-from position), ...)"""
    q = rng.permutation(np.arange(1000, 1000 + 50 * s_n))[:s_n].astype(np.int64)
    for to, frm in dup: q[to] = q[frm]
    return q * base


for _s in (255, 256, 511, 512):
    @case(f"stage2_sample{_s}_u32", f"a sample of {_s}: cutoff {max(1, _s // 256)}, buckets of cutoff and cutoff + 1 numbers", ["cutoff_strict"])
    def _(s=_s):
        cut = max(1, s // 256); rng = np.random.default_rng(s)
        dup = [(100 + i, 7) for i in range(cut - 1)] + [(200 + i, 9) for i in range(cut)]       # bucket of 7: cut numbers; bucket of 9: cut + 1
        arr = place(n_for_sample(s), np.uint32, _mult_sample(s, 1000, rng, dup))
        return arr, lambda r: r["cands"]["int"]["stage2"]["cutoff"] == cut and sorted(r["cands"]["int"]["stage2"]["sizes"])[-2:] == [cut, cut + 1]


@case("stage2_first_appearance_u32", "rare buckets first seen at sample positions 63, 64, 255 and 256 with two numbers each among single ones: the f64 sum depends on the order",
      ["sum_sorted_by_key"], both_auto=True)
def _():
    rng = np.random.default_rng(77)
    dup = [(300, 63), (301, 64), (400, 255), (401, 256)]
    arr = place(n_for_sample(512), np.uint32, _mult_sample(512, 1000, rng, dup))
    return arr, lambda r: r["cands"]["int"]["stage2"]["cutoff"] == 2 and r["cands"]["int"]["stage2"]["sizes"].count(2) == 4


@case("stage2_home_slot_8191_u32", "int-mult keys whose home slot in stage 2's table is 8191: the probe wraps")
def _():
    keys = _values_with_home(M.SAVED_SLOTS - 1, 51, M.SAVED_SLOTS, 60, 1000)
    q = np.array(keys, dtype=np.int64)[np.random.default_rng(3).permutation(60)]
    assert int(q.max()) * 1000 < (1 << 32)
    return place(n_for_sample(60), np.uint32, q * 1000), lambda r: "int" in r["cands"] and all(_home(x, 51, M.SAVED_SLOTS) == M.SAVED_SLOTS - 1 for x in keys)


for _side in ("above", "at"):
    @case(f"stage2_int_estimate_{_side}_u32", f"int mult: the estimate {'just above' if _side == 'above' else 'at or just below'} 0.5, one number apart")
    def _(side=_side):
        # 150 multiples of 1000: the last j of them are one number (a bucket beyond the cutoff, worth nothing, and triples without a GCD); the
        # first j whose estimate is <= 0.5, and the chunk before it
        rng = np.random.default_rng(21); base = _mult_sample(150, 1000, rng)
        prev = None
        for j in range(3, 148):
            s = base.copy(); s[150 - j:] = s[0]
            arr = place(n_for_sample(150), np.uint32, s); r = M.analyse(arr)
            if "int" not in r["cands"]: break
            if r["cands"]["int"]["stage2"]["est"] <= 0.5:
                assert prev is not None
                return (prev if side == "above" else arr), lambda r: ("int" in r["cands"]) and (r["cands"]["int"]["stage2"]["est"] > 0.5) == (side == "above") and (r["mode"][0] == "int_mult") == (side == "above")
            prev = arr
        raise AssertionError("no crossing found")


for _dt in (np.float32, np.float64):
    _nm = np.dtype(_dt).name

    for _side in ("at", "below"):
        @case(f"stage2_mult_estimate_{_side}_{_nm}", f"float mult: the estimate {'exactly' if _side == 'at' else 'one bit below'} 0.5 (30 / 60 and 29 / 60), one number apart")
        def _(dt=_dt, side=_side):
            K = FK[dt]
            # 57 copies of one multiple of 1/8 (a bucket beyond the cutoff) and three single ones that save 10 bits each: m * 2^-3, m odd, 2^(prec - 11) <= m
            e = K.prec - 11
            m = [(1 << e) + 1, (1 << e) + 3, ((1 << (e + (side == "below"))) + 5)]
            s = [dt(77 * 0.125)] * 57 + [dt(x * 0.125) for x in m]
            s = np.array(s, dtype=dt)[np.random.default_rng(4).permutation(60)]
            return place(n_for_sample(60), dt, s), lambda r: r["cands"]["tz"]["s_int"] == (30 if side == "at" else 29) and (r["mode"][0] == "float_mult") == (side == "at")

    for _side in ("above", "at"):
        @case(f"stage2_quant_estimate_{_side}_{_nm}", f"float quant: the estimate {'above' if _side == 'above' else 'exactly'} 1.5 (10 * 10 / 60 and 9 * 10 / 60), one number apart")
        def _(dt=_dt, side=_side):
            K = FK[dt]
            rare = 10 if side == "above" else 9
            # every number has exactly 10 trailing zeros (best = 10.0 bits at k = 10); `rare` numbers are alone in their bucket, the others share one
            bits = [(K.bias << K.prec) | ((2 * i + 1) << 10) for i in range(rare)] + [(K.bias << K.prec) | (999 << 10)] * (60 - rare)
            s = _from_bits(bits, dt)[np.random.default_rng(4).permutation(60)]
            return place(n_for_sample(60), dt, s), lambda r: r["bk"] == 10 and r["best"] == 10.0 and (r["quant_est"] > 1.5) == (side == "above") and (r["mode"] == ("float_quant", 10)) == (side == "above")

    @case(f"stage2_kind0_signs_{_nm}", "float mult: adjustments of 0, multipliers of 0 and of 2^mantissa width and above, a negative total")
    def _(dt=_dt):
        K = FK[dt]
        exact = [dt(((1 << (K.prec - 12)) + 2 * i + 1) * 0.125) for i in range(12)]              # adj = 0, 11 bits saved each
        tiny = [K.from_bits(((K.bias - 90) << K.prec) | 1)]                                        # round(x / base) = 0 (such numbers share ONE bucket: one of them stays rare)
        huge = [dt(2.0 ** (K.prec + 8) * (1.0 + (2 * i + 1) * 2.0 ** -10)) for i in range(2)]     # multiplier exponent >= the mantissa width
        off = [K.from_bits(K.to_bits(dt((2 * i + 4001) * 0.125 * 1.01)) | 1) for i in range(9)]  # a hundredth off their multiple: large adjustments
        s = np.array(exact + tiny + huge + off, dtype=dt)[np.random.default_rng(4).permutation(24)]
        return place(n_for_sample(24), dt, s), lambda r: r["k"] == -3 and r["n_ints"] >= 12 == r["required"] and r["cands"]["tz"]["s_int"] < 0 and r.get("float_mult_winner") != "tz"

    # ------------------------------------------------------------------ bids ------------------------------------------------------------------
    @case(f"bids_tz_beats_euclid_{_nm}", "both float-mult candidates: trailing zeros wins", both_auto=True)
    def _(dt=_dt):
        # eighths.  Two pairs agree on 5/8, which most of the sample is no multiple of; 8 pairs are too far apart for a GCD; 20 pairs are twins
        # (no GCD, and buckets beyond the cutoff for every candidate alike)
        K = FK[dt]; g = 0.625
        s = [3 * g, 2 * g, 5 * g, 4 * g]
        for j in range(8): s += [((1 << (K.prec - 1)) + 2 * j + 1) * 0.125, (2 * j + 1) * 0.125]
        for j in range(20): s += [(1001 + 2 * j * j) * 0.125] * 2                                  # (twins whose distances are all different: no GCD of the sample's integers is seen twice)
        return place(n_for_sample(60), dt, np.array(s, dtype=dt)), lambda r: "tz" in r["cands"] and "euclid" in r["cands"] and r.get("float_mult_winner") == "tz"

    @case(f"bids_euclid_beats_tz_{_nm}", "both float-mult candidates: Euclid wins", both_auto=True)
    def _(dt=_dt):
        rng = np.random.default_rng(32)
        tenths = (rng.permutation(np.arange(11, 4000))[:24] / 10.0).astype(dt)
        halves = (rng.permutation(np.arange(3, 400, 2))[:36] * 0.5).astype(dt)
        s = np.concatenate([tenths, halves])[rng.permutation(60)]
        return place(n_for_sample(60), dt, s), lambda r: "tz" in r["cands"] and "euclid" in r["cands"] and r.get("float_mult_winner") == "euclid" and r["mode"][0] == "float_mult"

    @case(f"bids_quant_cut_below_{_nm}", "float quant: best above 1.5, the estimate after the bucket cut not")
    def _(dt=_dt):
        K = FK[dt]
        bits = [(K.bias << K.prec) | ((2 * i + 1) << 2) for i in range(40)] + [(K.bias << K.prec) | (4001 << 2)] * 17 + [(K.bias << K.prec) | 1, (K.bias << K.prec) | 3, (K.bias << K.prec) | 7]
        s = _from_bits(bits, dt)[np.random.default_rng(4).permutation(60)]
        return place(n_for_sample(60), dt, s), lambda r: r["bk"] == 2 and r["best"] > 1.5 and "quant" in r["cands"] and r["quant_est"] <= 1.5 and r["mode"][0] != "float_quant"


@case("bids_mult_beats_quant_f32", "float mult and float quant both bid: float mult wins (the capacity cases have float quant winning)")
def _():
    rng = np.random.default_rng(33)
    s = (rng.permutation(np.arange(3, 16384, 2))[:60] * 0.125).astype(np.float32)
    return place(n_for_sample(60), np.float32, s), lambda r: r["quant_est"] > 1.5 and r["mode"][0] == "float_mult"


# -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for name, gate, fn, variants, both in _CASES:
        arr, claim = fn()
        out.append(Case(name, gate, arr, claim, variants, both))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def by_name(): return {c.name: c for c in cases()}


@functools.lru_cache(maxsize=None)
def record(name, variant=None): return M.analyse(by_name()[name].arr, variant)


def mixed_call():
    """the chunks of one batched call in shuffled order: int chunks with a candidate, without one and overflowing; float chunks with 0, 1, 2
    and 3 stage-2 candidates; an f16 chunk; an oversize chunk; a chunk below 10 numbers; two pairs of chunks of equal n.  (name, array)"""
    c = by_name()
    rng = np.random.default_rng(55)
    f16 = (rng.integers(1, 400, 3000) * 0.25).astype(np.float16)
    noise_f32 = place(n_for_sample(60), np.float32, rng.standard_normal(60).astype(np.float32) * np.float32(3.3))
    noise_u32 = place(n_for_sample(60), np.uint32, rng.integers(0, 1 << 31, 60))
    names = ["stage2_sample256_u32", "gcd_listed_193_u32", "tz4_float32", "tz5_float32", "bids_tz_beats_euclid_float32", "bids_euclid_beats_tz_float64",
             "cap_over_float32", "n9_uint32", "stage2_quant_estimate_above_float32", "stage2_quant_estimate_at_float32", "euclid_kept1000_float32", "euclid_kept1000_float64"]
    chunks = [(n, c[n].arr) for n in names] + [("f16", f16), ("noise_f32", noise_f32), ("noise_u32", noise_u32)]
    # three stage-2 candidates: trailing zeros, Euclid and float quant on eighths
    chunks.append(("three_cands_f32", c["bids_mult_beats_quant_f32"].arr))
    order = rng.permutation(len(chunks))
    return [chunks[i] for i in order]
