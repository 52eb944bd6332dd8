"""The ends of the mode-parameter ranges, shared by tests/test_format_limits.py (-m "not gpu") and tests/test_gpu_format_limits.py (-m gpu).

Two things live here:

  * a PLAIN MODEL of the three two-variable splits and their joins (mode/int_mult.rs, float_quant.rs, float_mult.rs) that shares no code with
    the oracle: classic ordering and int-mult on Python integers, float-quant as integer operations on the IEEE pattern, float-mult on numpy
    scalars of the number's own type with one rounding per operation (numpy's float16 computes in f32 and rounds the result to f16, which
    is what the reference's f16 does), rounding half away from zero.  Latents are Python integers in [0, 2^w).
  * the GRID: per number type, the mode parameters at the ends of what the format accepts, the parameters it must refuse, and data that
    carries the values at which those parameters go wrong (the type's extremes, +-0, subnormals, infinities, NaNs with payloads, multiples of
    the base beyond 2^prec).
"""
import numpy as np

INT_TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
FLOAT_TYPES = [np.float16, np.float32, np.float64]
UINT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
PREC = {16: 10, 32: 23, 64: 52}           # Float::PRECISION_BITS: mantissa bits without the implicit one
MODE_CLASSIC, MODE_FLOAT_MULT, MODE_FLOAT_QUANT, MODE_INT_MULT = 1, 2, 3, 4   # ModeSpecKind (include/pco_gfx.h)
INVALID_ARGUMENT = 3                      # ErrorKind::InvalidArgument in both libraries' numbering


def width(dt):
    return np.dtype(dt).itemsize * 8


def patterns(arr):
    """The numbers' bit patterns as Python integers."""
    arr = np.ascontiguousarray(arr)
    return [int(x) for x in arr.view(UINT[width(arr.dtype)])]


def from_patterns(pats, dt):
    return np.array(pats, dtype=UINT[width(dt)]).view(dt)


# ------------------------------------------------------------------------------------------------ the model
def to_ordered(b, w, kind):
    """Number::to_latent_ordered on a bit pattern: unsigned as it is, signed with the top bit flipped, floats with all bits flipped when
    negative and the top bit flipped otherwise."""
    mid = 1 << (w - 1)
    if kind == "u": return b
    if kind == "i": return b ^ mid
    return b ^ ((1 << w) - 1) if b & mid else b ^ mid


def from_ordered(l, w, kind):
    mid = 1 << (w - 1)
    if kind == "u": return l
    if kind == "i": return l ^ mid
    return l ^ mid if l & mid else l ^ ((1 << w) - 1)


def split_classic(arr):
    w, kind = width(arr.dtype), arr.dtype.kind
    return [to_ordered(b, w, kind) for b in patterns(arr)], None


def split_int_mult(arr, base):
    w, kind = width(arr.dtype), arr.dtype.kind
    u = [to_ordered(b, w, kind) for b in patterns(arr)]
    return [x // base for x in u], [x % base for x in u]


def join_int_mult(p, s, base, dt):
    w, kind = width(dt), np.dtype(dt).kind
    return from_patterns([from_ordered((m * base + a) % (1 << w), w, kind) for m, a in zip(p, s)], dt)


def split_float_quant(arr, k):
    w = width(arr.dtype); mid = 1 << (w - 1); lowmax = (1 << k) - 1
    p, s = [], []
    for b in patterns(arr):
        o = to_ordered(b, w, "f")
        p.append(o >> k)
        low = o & lowmax
        s.append(lowmax - low if b & mid else low)
    return p, s


def join_float_quant(p, s, k, dt):
    w = width(dt); mask = (1 << w) - 1; cutoff = (1 << (w - 1)) >> k; lowmax = (1 << k) - 1
    return from_patterns([from_ordered(((y << k) + (m if y >= cutoff else (lowmax - m) & mask)) & mask, w, "f") for y, m in zip(p, s)], dt)


def _bits(x):
    return int(np.array([x]).view(UINT[width(x.dtype)])[0])


def _scalar(b, ft):
    return np.array([b], UINT[width(ft)]).view(ft)[0]


def round_half_away(x):
    """f32::round / f64::round.  x - trunc(x) is exact; beyond 2^prec (and for inf / NaN) x is its own rounding."""
    t = np.trunc(x)
    if abs(x - t) >= 0.5:
        t = t + np.copysign(type(x)(1), x)
    return t


def int_float_to_latent(x):
    """Float::int_float_to_latent (data_types/float.rs): integers below 2^(prec + 1) by value, everything above (inf and NaN too) by the
    distance of its pattern from 2^(prec + 1)'s; the sign bit picks the half of the latent range."""
    ft = type(x); w = width(ft); mid = 1 << (w - 1)
    gpi = 1 << (PREC[w] + 1)
    b = _bits(x); ab = b & (mid - 1)
    a = _scalar(ab, ft)
    abs_int = int(a) if a < ft(gpi) else gpi + (ab - _bits(ft(gpi)))
    return (mid - 1 - abs_int if b & mid else mid + abs_int) % (1 << w)


def int_float_from_latent(l, ft):
    w = width(ft); mid = 1 << (w - 1); gpi = 1 << (PREC[w] + 1)
    neg = l < mid
    abs_int = mid - 1 - l if neg else l - mid
    a = ft(abs_int) if abs_int < gpi else _scalar((_bits(ft(gpi)) + (abs_int - gpi)) % (1 << w), ft)
    return -a if neg else a


def float_mult_config(base_f64, ft):
    """(base, inv_base) as the number type's scalars: the base rounded once from the double, its inverse 1 / base in the type's arithmetic."""
    with np.errstate(all="ignore"):
        base = ft(base_f64)
        return base, ft(1) / base


def split_float_mult(arr, base_f64):
    ft = arr.dtype.type; w = width(ft); mid = 1 << (w - 1); mask = (1 << w) - 1
    base, inv = float_mult_config(base_f64, ft)
    p, s = [], []
    with np.errstate(all="ignore"):
        for x in arr:
            mult = round_half_away(x * inv)
            p.append(int_float_to_latent(mult))
            s.append(((to_ordered(_bits(x), w, "f") - to_ordered(_bits(mult * base), w, "f")) & mask) ^ mid)
    return p, s


def join_float_mult(p, s, base_f64, dt):
    ft = np.dtype(dt).type; w = width(ft); mid = 1 << (w - 1); mask = (1 << w) - 1
    base, _ = float_mult_config(base_f64, ft)
    out = []
    with np.errstate(all="ignore"):
        for m, a in zip(p, s):
            un = int_float_from_latent(m, ft) * base
            out.append(from_ordered(((to_ordered(_bits(un), w, "f") + a) & mask) ^ mid, w, "f"))
    return from_patterns(out, dt)


def model_split(arr, kw):
    """(primary, secondary, mode payload as ChunkMeta carries it) of the model for a config's explicit mode."""
    m = kw["mode"]
    if m == MODE_INT_MULT: return split_int_mult(arr, kw["mode_u64"]) + (kw["mode_u64"],)
    if m == MODE_FLOAT_QUANT: return split_float_quant(arr, kw["mode_u64"]) + (kw["mode_u64"],)
    if m == MODE_FLOAT_MULT:
        base, _ = float_mult_config(kw["mode_f64"], arr.dtype.type)
        return split_float_mult(arr, kw["mode_f64"]) + (to_ordered(_bits(base), width(arr.dtype), "f"),)
    return split_classic(arr) + (0,)


def model_join(p, s, kw, dt):
    m = kw["mode"]
    if m == MODE_INT_MULT: return join_int_mult(p, s, kw["mode_u64"], dt)
    if m == MODE_FLOAT_QUANT: return join_float_quant(p, s, kw["mode_u64"], dt)
    if m == MODE_FLOAT_MULT: return join_float_mult(p, s, kw["mode_f64"], dt)
    w, kind = width(dt), np.dtype(dt).kind
    return from_patterns([from_ordered(l, w, kind) for l in p], dt)


# ------------------------------------------------------------------------------------------------ the grid
def int_mult_bases(w):
    return [1, 2, 3, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << (w - 1)) + 1, (1 << w) - 1]


def float_quant_ks(w):
    return [1, PREC[w] - 1, PREC[w]]


def float_quant_refused(w):
    return [0, PREC[w] + 1]


def float_mult_bases(ft):
    """name -> base (as the double a config carries; every one is exact in `ft`)."""
    fi = np.finfo(ft)
    return {"tiny": float(fi.smallest_subnormal), "min_normal": float(fi.smallest_normal), "max": float(fi.max), "negative": -0.75,
            "negative_tiny": -float(fi.smallest_subnormal),
            "inverse_subnormal": float(np.ldexp(1.5, int(fi.maxexp) - 1))}   # 1.5 * 2^emax: 1 / base lies below the smallest normal


FLOAT_MULT_REFUSED = [float("inf"), float("-inf"), float("nan"), 0.0]


def int_data(dt, n, base, rng):
    """The type's min, max, 0 and -1 first; then random patterns of the whole width, multiples of the base (wrapping) with small
    remainders, and values around the ends of the ordered range."""
    w = width(dt); u = UINT[w]; ii = np.iinfo(dt)
    head = np.array([ii.min, ii.max, 0], dtype=dt)
    minus_one = np.array([(1 << w) - 1], u).view(dt)      # -1 (unsigned: the same pattern, the type's max)
    k = max(n - 4, 0)
    rnd = np.frombuffer(rng.bytes(k * 8), np.uint64)
    full = rnd.astype(u) if w < 64 else rnd
    m = np.where(rng.random(k) < 0.25, rng.integers(0, 1 << min(20, w - 2), k), rng.geometric(0.2, k) - 1).astype(np.uint64)
    mult = (m * np.uint64(base) + rng.integers(0, 3, k).astype(np.uint64)).astype(u)   # wraps modulo 2^w
    ends = (np.where(rng.random(k) < 0.5, np.uint64(0), np.uint64((1 << w) - 8)) + rng.integers(0, 8, k).astype(np.uint64)).astype(u)
    pick = rng.integers(0, 8, k)   # 1/8 full-width patterns, 1/8 the ends of the range, the rest multiples
    body = np.where(pick == 0, full, np.where(pick == 1, ends, mult)).astype(u).view(dt)
    return np.ascontiguousarray(np.concatenate([head, minus_one, body])[:n])


def float_data(ft, n, base_f64, rng):
    """+-0, the smallest and largest subnormals, the largest finite, +-inf first; then random bit patterns of the type's own width (NaNs of
    every payload among them), NaN patterns outright (all-ones exponent, random sign and mantissa), subnormals, small multiples of the base
    with an ulp or two of error, and multiples of the base beyond 2^prec."""
    w = width(ft); u = UINT[w]; prec = PREC[w]; fi = np.finfo(ft)
    exp_mask = ((1 << (w - 1 - prec)) - 1) << prec
    head = np.array([0.0, -0.0, fi.smallest_subnormal, -fi.smallest_subnormal, fi.smallest_normal, fi.max, -fi.max, np.inf, -np.inf], dtype=ft)
    head = np.concatenate([head.view(u), np.array([(1 << prec) - 1, exp_mask | 1, exp_mask | (1 << (prec - 1)), (1 << (w - 1)) | exp_mask | ((1 << prec) - 1)], u)])
    k = max(n - head.size, 0)
    rnd = np.frombuffer(rng.bytes(k * 8), np.uint64)
    full = (rnd >> np.uint64(64 - w)).astype(u)
    nan = (full | u(exp_mask)).astype(u)
    nan = np.where((nan & u((1 << prec) - 1)) == 0, nan | u(1), nan).astype(u)
    sub = (full & u(((1 << prec) - 1) | (1 << (w - 1)))).astype(u)
    with np.errstate(all="ignore"):
        base = ft(base_f64)
        small = (rng.integers(-1000, 1000, k).astype(ft) * base).astype(ft)
        small = (small.view(u) + rng.integers(0, 3, k).astype(u)).astype(u)
        big = (rng.integers(1 << prec, 1 << min(prec + 4, 62), k).astype(np.float64).astype(ft) * base).astype(ft).view(u)
        ints = rng.integers(-(1 << 12), 1 << 12, k).astype(np.float64).astype(ft).view(u)
    pick = rng.integers(0, 16, k)   # 1/16 each: any pattern, NaNs, subnormals, integers; 1/8 large multiples; the rest small multiples
    body = np.choose(np.minimum(pick, 5), [full, nan, sub, ints, big, small]).astype(u)
    body = np.where(pick == 6, big, body).astype(u)
    return np.ascontiguousarray(np.concatenate([head, body])[:n].astype(u).view(ft))


def quant_data(ft, n, k, rng):
    """float_data with, in half of the positions behind the special values, the low k bits cleared (exactly quantised numbers: secondary 0 whatever the sign)."""
    w = width(ft); u = UINT[w]
    x = float_data(ft, n, 0.1, rng).view(u)
    clear = u(((1 << w) - 1) ^ ((1 << k) - 1))
    keep = (rng.random(x.size) >= 0.5) | (np.arange(x.size) < 13)      # (the special values at the front stay as they are)
    return np.ascontiguousarray(np.where(keep, x, x & clear).astype(u).view(ft))


def grid(n, seed=0):
    """Every accepted row of the grid at one size: (id, array, config keywords).  Delta is NoOp unless a row says otherwise; a few rows of each
    mode run under a consecutive delta so that the secondary's path beside a delta'd primary is taken too."""
    rows = []
    for ti, dt in enumerate(INT_TYPES):
        w = width(dt)
        for bi, base in enumerate(int_mult_bases(w)):
            rng = np.random.default_rng([seed, n, ti, bi])
            kw = dict(mode=MODE_INT_MULT, mode_u64=base, delta=1)
            if bi % 3 == 2: kw.update(delta=2, delta_order=1 + bi % 2)
            rows.append((f"{np.dtype(dt).name}-imult-{base:#x}-n{n}", int_data(dt, n, base, rng), kw))
    for ti, ft in enumerate(FLOAT_TYPES):
        w = width(ft)
        for ki, k in enumerate(float_quant_ks(w)):
            rng = np.random.default_rng([seed, n, 100 + ti, ki])
            kw = dict(mode=MODE_FLOAT_QUANT, mode_u64=k, delta=1)
            if ki == 1: kw.update(delta=2, delta_order=1)
            rows.append((f"{np.dtype(ft).name}-fquant-k{k}-n{n}", quant_data(ft, n, k, rng), kw))
        for bi, (name, base) in enumerate(float_mult_bases(ft).items()):
            rng = np.random.default_rng([seed, n, 200 + ti, bi])
            kw = dict(mode=MODE_FLOAT_MULT, mode_f64=base, delta=1)
            if bi == 3: kw.update(delta=2, delta_order=1)
            rows.append((f"{np.dtype(ft).name}-fmult-{name}-n{n}", float_data(ft, n, base, rng), kw))
    return rows


def refused():
    """Every refused row: (id, a small array of the type, config keywords)."""
    rows = []
    for ft in FLOAT_TYPES:
        a = np.arange(1, 40).astype(ft)
        for k in float_quant_refused(width(ft)):
            rows.append((f"{np.dtype(ft).name}-fquant-k{k}", a, dict(mode=MODE_FLOAT_QUANT, mode_u64=k, delta=1)))
        for b in FLOAT_MULT_REFUSED:
            rows.append((f"{np.dtype(ft).name}-fmult-{b}", a, dict(mode=MODE_FLOAT_MULT, mode_f64=b, delta=1)))
    for dt in INT_TYPES:
        rows.append((f"{np.dtype(dt).name}-imult-0", np.arange(1, 40).astype(dt), dict(mode=MODE_INT_MULT, mode_u64=0, delta=1)))
    return rows
