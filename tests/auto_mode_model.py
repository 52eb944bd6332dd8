"""A plain model of ModeSpec::Auto detection, written from the reference's text (sampling.rs, mode/int_mult.rs, mode/float_mult.rs,
mode/float_quant.rs, data_types/float.rs, data_types/unsigned.rs, mode/mod.rs), not from the kernels: Python integers for everything
that is an integer, numpy scalars of the chunk's float type for every IEEE operation (one rounding per operation, no contraction), the
C library's cbrt / log2 / log10 / pow where the reference calls them.

analyse(arr) returns one record (a dict) for a chunk: every quantity a gate of the decision compares, the candidates with what
est_bits_saved_per_num makes of them, the final mode, and the route the product takes (which only depends on three capacities of its
detection kernels, named below).  Where the reference leaves an order open (it adds the buckets up in HashMap order) the model takes the
order of first appearance, as the oracle does.

VARIANTS names wrong readings of single gates; analyse(arr, variant=name) computes the record under that reading.  The case table
(auto_edges_util.py) names, per case, the variants that must change its record: a test input that no wrong reading changes does not
sit on its gate.
"""
import ctypes
import ctypes.util
import math

import numpy as np

MIN_SAMPLE, SAMPLE_RATIO = 10, 40                            # sampling.rs:10-12
MEMORIZABLE_BINS = 256.0                                     # sampling.rs:15 (1 << CLASSIC_MEMORIZABLE_BINS_LOG)
MULT_REQUIRED, QUANT_REQUIRED = 0.5, 1.5                     # constants.rs:48-49
# the product's capacities (auto_mode_kernels.hip: kAutoCap, kGcdMaxEntries, kGcdSlots, kSavedSlots): they decide the ROUTE only
AUTO_CAP, GCD_MAX_ENTRIES, GCD_SLOTS, SAVED_SLOTS = 6656, 192, 2048, 8192
QUANT_PREFILTER = 1.499                                      # the host step sends a float-quant candidate to stage 2 only above this
ROUTES = ("none", "dev_int", "dev_float", "host_size", "host_overflow")   # pco_gfx_debug_auto_mode: 0..4

VARIANTS = ("cutoff_strict", "required_floor", "need_no_plus_one", "percentile_order", "drop_count_two", "sum_sorted_by_key",
            "filter_lim_strict", "tz_gate_4", "sim_nonstrict")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cbrt.restype = ctypes.c_double; _libm.cbrt.argtypes = [ctypes.c_double]
_M64 = (1 << 64) - 1


# ---- sampling.rs:73-100: Floyd's sample, Xoroshiro128++ seeded from 0 through SplitMix64 ----
def _rotl(x, k): return ((x << k) | (x >> (64 - k))) & _M64


def sample_indices(n):
    """positions of the mode sample in draw order; None below MIN_SAMPLE numbers"""
    if n < MIN_SAMPLE: return None
    target = MIN_SAMPLE + (n - MIN_SAMPLE) // SAMPLE_RATIO
    state = []
    seed = 0
    for _ in range(2):
        seed = (seed + 0x9E3779B97F4A7C15) & _M64
        z = seed
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        state.append(z ^ (z >> 31))
    s0, s1 = state
    visited = set(); out = []
    for j in range(n - target, n):
        r = (_rotl((s0 + s1) & _M64, 17) + s0) & _M64
        s1 ^= s0
        s0 = _rotl(s0, 49) ^ s1 ^ ((s1 << 21) & _M64)
        s1 = _rotl(s1, 28)
        t = r % (j + 1)
        idx = j if t in visited else t
        visited.add(idx); out.append(idx)
    return out


# ---- sampling.rs:108-138 ----
def est_bits_saved(keys_and_savings, variant=None):
    """buckets in first-appearance order: (key, count, running sum of the savings); the sum over the rare ones; the estimate"""
    where = {}; buckets = []
    for key, saved in keys_and_savings:
        at = where.get(key)
        if at is None:
            at = where[key] = len(buckets); buckets.append([key, 0, 0.0])
        buckets[at][1] += 1
        buckets[at][2] = buckets[at][2] + saved
    n = len(keys_and_savings)
    cutoff = max(1, int(n / MEMORIZABLE_BINS))
    rare = [b for b in buckets if (b[1] < cutoff if variant == "cutoff_strict" else b[1] <= cutoff)]
    if variant == "sum_sorted_by_key": rare = sorted(rare, key=lambda b: b[0])
    total = 0.0
    for b in rare: total = total + b[2]
    return {"cutoff": cutoff, "sizes": [b[1] for b in buckets], "n_rare": len(rare), "sum": total, "est": total / n if n else 0.0}


# ---- mode/int_mult.rs:56-213, mode/mod.rs:7-18 ----
def _entropy1(p): return 0.0 if p == 0.0 or p == 1.0 else -p * math.log2(p)


def worst_case_entropy(p, n_m1): return _entropy1(p) + n_m1 * _entropy1((1.0 - p) / n_m1)


def score_triple_gcd(gcd, with_gcd, total):
    zeta2 = math.pi * math.pi / 6.0
    w, t = float(with_gcd), float(total)
    natural = 1.0 / (zeta2 * gcd * gcd)
    stdev = math.sqrt(natural * (1.0 - natural) / t)
    if (w / t - natural) / stdev < 3.0: return None
    lcb = w - 1.0 * math.sqrt(w)
    if lcb <= 0.0: return None
    congruence = min(zeta2 * lcb / t, 1.0)
    g1 = gcd - 1.0; inv_sq = 1.0 / (g1 * g1)
    f = lambda p: p * p * p + (1.0 - p) * (1.0 - p) * (1.0 - p) * inv_sq - congruence
    lb, ub = 1.0 / gcd, _libm.cbrt(congruence) + 2.0 ** -52
    flb, fub = f(lb), f(ub)
    if flb > 0.0 or fub < 0.0: return None
    while ub - lb > 1E-4 and fub - flb > 0.0:
        prop = 0.001 + 0.998 * fub / (fub - flb)
        mid = prop * lb + (1.0 - prop) * ub; fmid = f(mid)
        if fmid < 0.0: lb, flb = mid, fmid
        else: ub, fub = mid, fmid
    saved = math.log2(gcd) - worst_case_entropy((lb + ub) / 2.0, g1)
    return None if saved < MULT_REQUIRED else saved


def triple_gcds(sample):
    """the GCDs above 1 of the sample's sorted triples: (value, count) in first-appearance order"""
    where = {}; out = []
    for i in range(0, len(sample) - 2, 3):
        a, b, c = sorted(sample[i: i + 3])
        g = math.gcd(b - a, c - a)
        if g <= 1: continue
        at = where.get(g)
        if at is None: where[g] = len(out); out.append([g, 1])
        else: out[at][1] += 1
    return [tuple(x) for x in out]


def choose_candidate_base(sample, variant=None):
    """(counts, base or None, score): max_by_key keeps the last maximum"""
    counts = triple_gcds(sample)
    best = None
    for g, c in counts:
        if variant == "drop_count_two" and c <= 2: continue
        s = score_triple_gcd(float(min(g, _M64)), c, len(sample) // 3)
        if s is not None and (best is None or s >= best[1]): best = (g, s)
    return counts, (best[0] if best else None), (best[1] if best else 0.0)


def _gcd_table(counts):
    n_distinct = len(counts); n_listed = sum(1 for _, c in counts if c > 1)
    overflow = n_distinct >= GCD_SLOTS or n_listed > GCD_MAX_ENTRIES
    return {"counts": counts, "n_distinct": n_distinct, "n_listed": n_listed, "overflow": overflow, "n_entries": 0 if overflow else n_listed}


# ---- floats ----
class FloatKind:
    def __init__(self, F, U, bits, prec, bias):
        self.F, self.U, self.bits, self.prec, self.bias = F, U, bits, prec, bias
        self.mask = (1 << bits) - 1; self.mid = 1 << (bits - 1)
        self.max_bits = self.mid - 1 - (1 << prec)                     # the largest finite value
        self.max_for_sampling = self.max_bits - (1 << prec)            # float.rs:141, 257: half of it

    def from_bits(self, b): return self.U(b & self.mask).view(self.F)
    def to_bits(self, x): return int(self.F(x).view(self.U))
    def exponent(self, x): return ((self.to_bits(x) & (self.mid - 1)) >> self.prec) - self.bias          # float.rs:183-185
    def exp2(self, p): return self.from_bits(((self.bias + p) & self.mask) << self.prec)                 # float.rs:158-160

    def round(self, x):
        """f32::round / f64::round: half away from zero"""
        F = self.F
        a = F(abs(x)); fl = F(np.floor(a))
        r = F(fl + F(1)) if F(a - fl) >= F(0.5) else fl
        return F(-r) if self.to_bits(x) & self.mid else r

    def ordered(self, x):
        b = self.to_bits(x)
        return (~b) & self.mask if b & self.mid else b ^ self.mid

    def int_float_to_latent(self, x):                                   # float.rs:229-244
        a = self.F(abs(x)); gpi = 1 << (self.prec + 1); gf = self.F(gpi)
        ai = int(a) if a < gf else (gpi + self.to_bits(a) - self.to_bits(gf)) & self.mask
        return (self.mid - 1 - ai) & self.mask if self.to_bits(x) & self.mid else (self.mid + ai) & self.mask


F16 = FloatKind(np.float16, np.uint16, 16, 10, 15)
F32 = FloatKind(np.float32, np.uint32, 32, 23, 127)
F64 = FloatKind(np.float64, np.uint64, 64, 52, 1023)
FLOAT_KINDS = {"float16": F16, "float32": F32, "float64": F64}


def _tz(b): return (b & -b).bit_length() - 1


def _pair_gcd(hi, lo, F, prec):
    """mode/float_mult.rs:101-142 in numpy scalars of type F: one IEEE operation per step, as the device does them"""
    tiny, eps, p16, p6 = F(2.0) ** F(-(prec - 6)), F(2.0) ** F(-prec), F(2.0) ** F(-16), F(64.0)
    if lo <= hi * tiny or lo == hi: return None
    gv, ge, lv, le = hi, F(0), lo, F(0)
    while True:
        prev = gv
        q = F(gv / lv)
        fl = F(np.floor(q))
        ratio = F(fl + F(1)) if F(q - fl) >= F(0.5) else fl        # round half away from zero (q > 0; q - floor(q) is exact)
        ge = F(ge + F(F(ratio * le) + F(gv * eps)))
        gv = F(abs(F(gv - F(ratio * lv))))
        if gv <= F(prev * p16) or gv <= ge: return lv
        if gv <= F(hi * tiny) or gv <= F(ge * p6): return None
        gv, lv = lv, gv; ge, le = le, ge


def centre_base(basev, s, F, prec, bias, bits_n):
    """center_sample_base (mode/float_mult.rs:239-258): the two running sums in sample order; (centred base, weight sum)"""
    U = np.uint32 if F == np.float32 else (np.uint64 if F == np.float64 else np.uint16)
    inv = F(F(1.0) / basev); tsum = F(0); tw = F(0)
    with np.errstate(all="ignore"):
        for x in s:
            q = F(x * inv); fl = F(np.floor(q)); mult = F(fl + F(1)) if F(q - fl) >= F(0.5) else fl
            mb = int(np.array([mult]).view(U)[0]) & ((1 << (bits_n - 1)) - 1)
            me = (mb >> prec) - bias
            if 0 <= me < prec and mult != 0:
                over = F(F(mult * basev) - x)
                w = F(prec - me)
                tsum = F(tsum + F(w * F(over / mult))); tw = F(tw + w)
        return F(basev - F(tsum / tw)), tw


def _f64_round(x): return x if x != x or math.isinf(x) else math.copysign(math.floor(abs(x) + 0.5) if abs(x) < 2.0 ** 52 else abs(x), x)


def snap_to_int_reciprocal(K, base):                                    # mode/float_mult.rs:261-275
    F = K.F
    inv = F(F(1.0) / base); rinv = K.round(inv)
    try: dinv = F(math.pow(10.0, _f64_round(math.log10(float(inv)))))
    except (ValueError, OverflowError): dinv = F(np.nan)
    if F(abs(F(inv - rinv))) < F(0.02): return F(F(1.0) / rinv), rinv
    if F(F(abs(F(inv - dinv))) / inv) < F(0.01): return F(F(1.0) / dinv), dinv
    return base, inv


def float_mult_savings(K, base, inv, s):                                # mode/float_mult.rs:277-316
    F = K.F; out = []
    for x in s:
        mult = K.round(F(x * inv))
        key = K.int_float_to_latent(mult)
        e = K.exponent(mult)
        inter = K.prec - e if 0 <= e <= K.prec else 0
        approx, xu = K.ordered(F(mult * base)), K.ordered(x)
        saved = inter - (1 + 2 * abs(xu - approx).bit_length())
        out.append((key, float(saved)))
    return out


def _analyse_float(K, vals, variant):
    F = K.F; prec = K.prec
    rec = {}
    lim = K.max_for_sampling
    s_bits = []
    for v in vals:                                                      # float.rs:70-80
        a = K.to_bits(v) & (K.mid - 1); e = a >> prec
        if e == 0 or e == (1 << (K.bits - 1 - prec)) - 1: continue
        if a < lim or (a == lim and variant != "filter_lim_strict"): s_bits.append(a)
    kept = len(s_bits); rec["kept"] = kept
    if kept < MIN_SAMPLE: return rec, None
    s = [K.from_bits(b) for b in s_bits]
    tzs = [_tz(b) for b in s_bits]; exps = [(b >> prec) - K.bias for b in s_bits]
    hist = [0] * (prec + 1)
    for t in tzs: hist[min(prec, t)] += 1
    rec["hist"] = hist
    # -- choose_config_by_trailing_zeros (float_mult.rs:145-194)
    gate = 4 if variant == "tz_gate_4" else 5
    divp = [e - max(prec - t, 0) for e, t in zip(exps, tzs)]
    tz5 = sum(1 for t in tzs if t >= gate)
    k = min([d for d, t in zip(divp, tzs) if t >= gate], default=0x7fffffff)
    half = kept * 0.5
    required = max(math.floor(half) if variant == "required_floor" else math.ceil(half), MIN_SAMPLE)
    rec.update(tz5=tz5, k=k, required=required, n_ints=0, gcd=None)
    cands = {}
    if tz5 >= required:
        lshift = K.bits - prec - 1
        ints = [((((b << lshift) & K.mask) | K.mid) >> (K.bits - 1 - (e - k))) for b, e, d in zip(s_bits, exps, divp) if d >= k and e < k + K.bits]
        rec["n_ints"] = len(ints)
        if len(ints) >= required:
            counts, ib, _ = choose_candidate_base(ints, variant)
            rec["gcd"] = _gcd_table(counts); rec["int_base"] = ib
            base = F(F(ib if ib is not None else 1) * K.exp2(k))
            cands["tz"] = {"base": base, "inv": F(F(1.0) / base)}
    # -- approx_sample_gcd_euclidean (float_mult.rs:197-229)
    g = [_pair_gcd(max(s[i], s[i + 1]), min(s[i], s[i + 1]), F, prec) for i in range(0, kept - 1, 2)]
    g = sorted(x for x in g if x is not None)
    thousandth = math.ceil(kept * 0.001)
    need = thousandth if variant == "need_no_plus_one" else 1 + thousandth
    pcts = (0.5, 0.3, 0.1) if variant == "percentile_order" else (0.1, 0.3, 0.5)
    pv, sim = [F(0)] * 3, [0, 0, 0]
    for q, pct in enumerate(pcts):
        if not g: break
        c = g[int(pct * len(g))]; pv[q] = c
        window = F(F(0.01) * c)
        sim[q] = sum(1 for x in g if (F(abs(F(x - c))) <= window if variant == "sim_nonstrict" else F(abs(F(x - c))) < window))
    has = len(g) >= need and any(x >= need for x in sim)
    rec.update(n_g=len(g), need=need, pct_bits=[K.to_bits(x) for x in pv], sim=sim, has_euclid=has, base_c=0, weight_sum=None)
    if has:
        pick = pv[[x >= need for x in sim].index(True)]
        centred, tw = centre_base(pick, s, F, prec, K.bias, K.bits)
        rec["base_c"] = K.to_bits(centred); rec["weight_sum"] = float(tw)
        base, inv = snap_to_int_reciprocal(K, centred)
        cands["euclid"] = {"base": base, "inv": inv}
    # -- the float-mult bid (float_mult.rs:338-358): the last maximum of the candidates that save at least 0.5 bits
    fm = None
    for name in ("tz", "euclid"):
        if name not in cands: continue
        c = cands[name]
        c["stage2"] = est_bits_saved(float_mult_savings(K, c["base"], c["inv"], s), variant)
        c["s_int"] = int(c["stage2"]["sum"]); c["s_dbl"] = 0
        c["base_bits"], c["inv_bits"] = K.to_bits(c["base"]), K.to_bits(c["inv"])
        v = c["stage2"]["est"]
        if v >= MULT_REQUIRED and (fm is None or not v < fm[1]): fm = (name, v)
    # -- float quant (float_quant.rs:73-149)
    cum = list(hist); rev = 0
    for i in range(prec, -1, -1): rev += hist[i]; cum[i] = rev
    bk, best = 0, 0.0
    for kk in range(1, prec + 1):
        if cum[kk] == 0: continue
        sv = kk - worst_case_entropy(cum[kk] / float(kept), float((1 << kk) - 1))
        if sv > best: bk, best = kk, sv
        else: break
    q2 = est_bits_saved([(b >> bk, best) for b in s_bits], variant)
    rec.update(bk=bk, best=best, quant_est=q2["est"])
    if best > QUANT_PREFILTER: cands["quant"] = {"bk": bk, "stage2": q2, "s_int": 0, "s_dbl": _f64_bits(q2["sum"])}
    rec["cands"] = cands
    # -- the bids (float.rs:82-98; the chunk compressor takes the last maximum; classic bids 0.0)
    mode, bestv = ("classic", 0), 0.0
    if fm is not None and not fm[1] < bestv:
        mode, bestv = ("float_mult", K.ordered(cands[fm[0]]["base"])), fm[1]
        rec["float_mult_winner"] = fm[0]
    if q2["est"] > QUANT_REQUIRED and not q2["est"] < bestv: mode = ("float_quant", bk)
    return rec, mode


def _f64_bits(x): return int(np.float64(x).view(np.uint64))


def _analyse_int(lat, variant):
    counts, base, score = choose_candidate_base(lat, variant)
    rec = {"gcd": _gcd_table(counts), "cands": {}}
    mode = ("classic", 0)
    if base is not None:                                                # int_mult.rs:215-228
        st = est_bits_saved([(x // base, score) for x in lat], variant)
        rec["cands"]["int"] = {"base": base, "score": score, "stage2": st, "s_int": 0, "s_dbl": _f64_bits(st["sum"])}
        if st["est"] > MULT_REQUIRED: mode = ("int_mult", base)
    return rec, mode


def analyse(arr, variant=None):
    """the record of one chunk"""
    assert variant is None or variant in VARIANTS
    arr = np.ascontiguousarray(arr); n = arr.size; name = arr.dtype.name
    rec = {"n": n, "dtype": name, "sample_n": 0, "route": "none", "mode": ("classic", 0)}
    idx = sample_indices(n)
    if idx is None: return rec
    rec["sample_n"] = len(idx)
    if name in FLOAT_KINDS:
        K = FLOAT_KINDS[name]
        with np.errstate(all="ignore"):
            r, mode = _analyse_float(K, arr[idx], variant)
        rec.update(r)
        if mode is not None: rec["mode"] = mode
        if K.bits < 32 or len(idx) > AUTO_CAP: rec["route"] = "host_size"
        elif rec["kept"] < MIN_SAMPLE: rec["route"] = "none"
        elif rec.get("gcd") and rec["gcd"]["overflow"]: rec["route"] = "host_overflow"
        else: rec["route"] = "dev_float"
    else:
        bits = arr.dtype.itemsize * 8
        if arr.dtype.kind == "i": lat = [int(x) + (1 << (bits - 1)) for x in arr[idx]]      # signed.rs:50-52
        else: lat = [int(x) for x in arr[idx]]
        r, mode = _analyse_int(lat, variant)
        rec.update(r); rec["mode"] = mode
        if len(idx) > AUTO_CAP: rec["route"] = "host_size"
        elif rec["gcd"]["overflow"]: rec["route"] = "host_overflow"
        else: rec["route"] = "dev_int"
    return rec


def hook_view(rec):
    """the fields of a record that pco_gfx_debug_auto_mode reports, as it reports them (host routes: the route alone)"""
    out = {"route": ROUTES.index(rec["route"])}
    if rec["route"] in ("host_size", "host_overflow"): return out
    cands = rec.get("cands", {})
    slots = {"tz": 0, "euclid": 1, "quant": 2, "int": 3}
    if rec["route"] == "none":
        if "kept" in rec and rec["sample_n"] >= MIN_SAMPLE and rec["dtype"] != "float16": out["s_size"] = rec["kept"]
        return out
    g = rec.get("gcd")
    out.update(n_entries=g["n_entries"] if g else 0, overflow=0, cand_mask=sum(1 << slots[c] for c in cands))
    if rec["route"] == "dev_float":
        out.update(s_size=rec["kept"], tz5=rec["tz5"], n_ints=rec["n_ints"], n_gcd=rec["n_g"], sim=list(rec["sim"]), has_euclid=int(rec["has_euclid"]),
                   k=rec["k"], base_c=rec["base_c"])
    for name, c in cands.items():
        q = slots[name]
        out["s_int%d" % q] = c["s_int"]; out["s_dbl%d" % q] = c["s_dbl"]
        if q < 2: out["base%d" % q] = c["base_bits"]; out["inv%d" % q] = c["inv_bits"]
        elif q == 2: out["bk"] = c["bk"]
        else: out["base3"] = c["base"]
    return out
