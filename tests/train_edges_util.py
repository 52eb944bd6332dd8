"""The cases of the training-step edge suites (test_train_model.py on the CPU, test_gpu_train_edges.py on the device): chunks whose
histograms put one decision of the bin-partition DP, of its shortcuts, of quantize_weights or of should_fallback exactly on its edge.

What makes a tie of the DP exact: every count, every merged count and the total are powers of two, so log2_approx is exact, every cost
is an integer below 2^24 and two partitions with the same multiset of bins cost the same bit for bit.  The building blocks:

  * a TRIPLE v, v+1, v+2 of equal counts c: {[v, v+1], [v+2]} and {[v], [v+1, v+2]} tie at the step of v+2 between j = i - 1 and j = i;
  * a RUN of r consecutive values of equal counts: every partition into the fewest power-of-two blocks costs the same -- r = 192 ties
    j = i - 63 with j = i - 127 at its last step, r = 129 ties j = i with j = i - 127, r = 1025 ties j = i with j = i - 1023;
  * a run whose first 64 c of mass sit on 32 values two apart with counts 2 c (the same density, half the bins): the 192-run's tie with
    its lower candidate inside the first 64 bins, which a plain run cannot do (its lower candidate is 64 bins behind the run's start);
  * FILLERS, far single values of power-of-two counts, make the total a power of two; in front they shift the bin indices of the
    structure, behind they do not.

A case names the variable its edge is on, the histogram that variable must have, what the model's report must show (`edge`) and the
variant of the model under which its plan must change (`variant`).  Everything a case claims is checked by test_train_model.py."""
import collections
import functools

import numpy as np

import lookback_model as LM
import oracle_lib as O
import train_model as M

DT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
WIDTHS = (8, 16, 32, 64)
MODE_CLASSIC, MODE_INT_MULT = O.MODE_CLASSIC, O.MODE_TRY_INT_MULT
DELTA_NONE, DELTA_CONSECUTIVE, DELTA_LOOKBACK = O.DELTA_NOOP, O.DELTA_TRY_CONSECUTIVE, O.DELTA_TRY_LOOKBACK

# edge: {"ties": {step: [tied js]}} | {"shortcut": name or None} | {"quant": {...}} | {"fallback": worst - baseline} | {"capped": True} |
# {"lookback_triples": [v, ...]}; see check_edge().  bins: the histogram the case's variable must have, None where the case does not design it.
Case = collections.namedtuple("Case", "name section bits kw var bins edge variant")


def variant_set(case):
    return {case.variant} if isinstance(case.variant, str) else set(case.variant)


def classic(level):
    return dict(level=level, mode=MODE_CLASSIC, delta=DELTA_NONE)


def pow2_parts(mass):
    """`mass` as a sum of powers of two, largest first."""
    return [1 << k for k in range(int(mass).bit_length() - 1, -1, -1) if mass >> k & 1]


# ---------------------------------------------------------------------------------------------------------------- bin lists
def layout(bits, front, structure, back):
    """[(count, v, v)] in ascending order: front fillers, the structure [(offset, count)] from a base behind them, back fillers under the
    type's maximum.  None if the type has no room."""
    far, base_gap = {8: (2, 2), 16: (64, 1024), 32: (1000, 1 << 24), 64: (1000, 1 << 24)}[bits]
    base = far * len(front) + base_gap if bits <= 16 else base_gap
    top = (1 << bits) - 1
    vals = [(c, far * k) for k, c in enumerate(front)] + [(c, base + off) for off, c in structure] + \
           [(c, top - far * (len(back) - 1 - k)) for k, c in enumerate(back)]
    lows = [v for _, v in vals]
    if any(b <= a for a, b in zip(lows, lows[1:])) or lows[-1] > top or (bits > 16 and far * len(front) >= base):
        return None
    if len(back) and lows[len(front) + len(structure) - 1] + far > lows[len(front) + len(structure)]:
        return None
    return [(c, v, v) for c, v in vals]


def triple_structure(bits, n_triples, c):
    spacing = {8: 4, 16: 64, 32: 4096, 64: 4096}[bits]
    return [(spacing * t + d, c) for t in range(n_triples) for d in range(3)]


def run_structure(r, c, sparse_prefix=False):
    if not sparse_prefix:
        return [(d, c) for d in range(r)]
    return [(2 * d, 2 * c) for d in range(32)] + [(d, c) for d in range(64, r)]


def numbers_of(bins, bits, seed=0):
    """An array with the histogram `bins`: a bin of one value holds it `count` times, a wider one its two ends half and half."""
    parts = []
    for c, lo, hi in bins:
        parts.append(np.full(c, lo, np.uint64))
        if lo != hi: parts[-1][c // 2:] = hi
    a = np.concatenate(parts).astype(DT[bits])
    np.random.default_rng(seed).shuffle(a)
    return a


def from_differences(latents, bits):
    """Numbers whose order-1 differences, centred as the format stores them, are `latents` (one number more than latents)."""
    mid = 1 << (bits - 1)
    d = (latents.astype(np.uint64) - np.uint64(mid)) & np.uint64((1 << bits) - 1) if bits < 64 else latents.astype(np.uint64) - np.uint64(mid)
    x = np.concatenate([np.zeros(1, np.uint64), np.cumsum(d, dtype=np.uint64)])
    return (x & np.uint64((1 << bits) - 1)).astype(DT[bits]) if bits < 64 else x


# ---------------------------------------------------------------------------------------------------------------- the chunk's variables
def case_latents(case):
    """{variable: latents} of the case's chunk by the format's definitions (unsigned numbers: Classic is the identity, IntMult splits into
    quotient and remainder, order-1 differences are stored centred on the middle of the type and lose their first position)."""
    x = numbers(case.name)
    bits = case.bits
    out = collections.OrderedDict()
    if case.kw["mode"] == MODE_INT_MULT:
        base = DT[bits](case.kw["mode_u64"])
        out["primary"], out["secondary"] = x // base, x % base
    else:
        out["primary"] = x
    if case.kw["delta"] == DELTA_CONSECUTIVE:
        assert case.kw["delta_order"] == 1
        p = out["primary"]
        out["primary"] = (p[1:] - p[:-1]) + DT[bits](1 << (bits - 1))      # (wraps in the type)
    if case.kw["delta"] == DELTA_LOOKBACK:   # the lookbacks, by the plain model of the search, are a 32-bit variable in front of the primary
        lbs = LM.choose_lookbacks(out["primary"], bits, LM.window_log(x.size))
        _, deltas = LM.apply_lookbacks(out["primary"], lbs, bits)
        out = collections.OrderedDict([("delta", np.array(lbs, np.uint32)), ("primary", np.array(deltas, DT[bits]))])
    return out


def var_bits(case, key):
    return 32 if key == "delta" else case.bits


DELTA_NAME = {DELTA_NONE: "none", DELTA_CONSECUTIVE: "consecutive", DELTA_LOOKBACK: "lookback"}
DELTA_SHOWN = {DELTA_NONE: 0, DELTA_CONSECUTIVE: 1, DELTA_LOOKBACK: 2}      # the delta encoding's variant in the ChunkMeta


def model_plans(case, variants=None):
    """The model's prediction of the whole chunk: ({variable: Plan}, fell back, worst, baseline, unoptimized_bins_log).  The histograms
    are the oracle's (its histogram has a suite of its own); everything after them is the model."""
    n = numbers(case.name).size
    ubl = M.choose_unoptimized_bins_log(case.kw["level"], n)
    plans = collections.OrderedDict()
    for key, lat in case_latents(case).items():
        bl = M.var_bins_log(ubl, key, variants)
        plans[key] = M.train(hist(case.name, key, bl), var_bits(case, key), bl, lat.size, variants)
    mode = "int_mult" if case.kw["mode"] == MODE_INT_MULT else "classic"
    # (a lookback chunk of these sizes keeps one latent of state: state_n_log = 0, which the CPU suite reads back from the oracle's chunk)
    fb, worst, baseline = M.should_fallback(plans, n, case.bits, mode, DELTA_NAME[case.kw["delta"]], case.kw.get("delta_order", 0), state_n_log=0, variants=variants)
    return plans, fb, worst, baseline, ubl


@functools.lru_cache(maxsize=None)
def hist(name, key, bins_log):
    h, fell_back = O.histogram(case_latents(BY_NAME()[name])[key], bins_log, rule=1)
    return h


def predicted_chunk(case, variants=None):
    """What inspect_first_chunk must show: (mode kind, delta kind, {variable index: (ans_size_log, [(weight, lower, offset_bits)])}), with
    the variables numbered as the format numbers them (0 delta, 1 primary, 2 secondary)."""
    plans, fb, _, _, _ = model_plans(case, variants)
    if fb:
        return 0, 0, {1: (0, [(1, 0, case.bits)])}
    idx = {"delta": 0, "primary": 1, "secondary": 2}
    return (1 if case.kw["mode"] == MODE_INT_MULT else 0), DELTA_SHOWN[case.kw["delta"]], \
        {idx[k]: (p.ans_size_log, list(zip(p.weights, p.lowers, p.offset_bits))) for k, p in plans.items()}


def shown_chunk(info, bins):
    return int(info.mode_kind), int(info.delta_kind), \
        {v: (int(info.ans_size_log[v]), [tuple(int(x) for x in row) for row in bins[v]]) for v in range(3) if info.var_present[v]}


def check_edge(case, plan, worst=None, baseline=None):
    """None if the model's report of the case's variable shows the edge the case claims, otherwise what it shows instead."""
    e = case.edge
    if "ties" in e:
        got = {i: plan.dp.ties.get(i) for i in e["ties"]}
        if got != e["ties"] or plan.dp.shortcut is not None: return got, plan.dp.shortcut
    if "shortcut" in e:
        if plan.dp.shortcut != e["shortcut"]: return plan.dp.shortcut
        if "holds" in e:   # which of the two comparisons hold, whichever the code took
            holds = (bool(plan.dp.single_cost < plan.dp.threshold), plan.dp.trivial_cost is not None and bool(plan.dp.trivial_cost < plan.dp.threshold))
            if holds != e["holds"]: return holds
        if e.get("single_equal") and plan.dp.single_cost != plan.dp.threshold: return plan.dp.single_cost, plan.dp.threshold
        if e.get("trivial_equal") and plan.dp.trivial_cost != plan.dp.threshold: return plan.dp.trivial_cost, plan.dp.threshold
        if e.get("one_wide") and sum(lo != hi for _, lo, hi in case.bins) != 1: return "bins"
    if "lookback_triples" in e:   # every value of every triple a bin of its own with exactly LOOKBACK_COUNT latents, tied at its last value
        h = hist(case.name, case.var, M.choose_unoptimized_bins_log(case.kw["level"], numbers(case.name).size))
        for v in e["lookback_triples"]:
            if any((LOOKBACK_COUNT, v + d, v + d) not in h for d in range(3)): return v, [b for b in h if v <= b[1] <= v + 2]
            i = h.index((LOOKBACK_COUNT, v + 2, v + 2))
            if plan.dp.ties.get(i) != [i - 1, i] or plan.dp.shortcut is not None: return v, i, plan.dp.ties.get(i), plan.dp.shortcut
    if "capped" in e:   # more distinct values, and more bins at the chunk's own bins_log, than the secondary is allowed
        ubl = M.choose_unoptimized_bins_log(case.kw["level"], numbers(case.name).size)
        sizes = len(hist(case.name, case.var, M.LIMITED_UNOPTIMIZED_BINS_LOG)), len(hist(case.name, case.var, ubl))
        if not (sizes[0] <= 64 < sizes[1] and ubl > M.LIMITED_UNOPTIMIZED_BINS_LOG): return sizes
    if "quant" in e:
        q = e["quant"]
        min_size_log, size_log0, pow2, rep = plan.quant
        show = dict(n_dec=rep.n_dec, n_inc=rep.n_inc, dec_skipped_ones=rep.dec_skipped_ones, pow2=pow2, size_log=plan.ans_size_log, weights=plan.weights,
                    halves=sum(float(f) % 1.0 == 0.5 for f in rep.float_weights), desired_zero=bool(rep.desired_surplus == 0),
                    full=len(plan.weights) == 1 << size_log0, min_over_est=min_size_log > plan.est)
        bad = {k: show[k] for k, want in q.items() if (show[k] < want[1] if isinstance(want, tuple) else show[k] != want)}
        if bad: return bad
    if "est" in e and plan.est != e["est"]: return plan.est
    if "fallback" in e:
        if worst is None or worst - baseline != e["fallback"]: return worst, baseline
    return None


# ---------------------------------------------------------------------------------------------------------------- the cases
def _tie_case(name, section, bits, level, builder, ties, counts=(16, 32, 64, 128), kw=None, var="primary"):
    """The first count per value for which the model says the case works: the histogram holds at most 2^bins_log bins at that level and
    the DP ties at `ties` without a shortcut.  (The count decides whether a triple splits 2 + 1 or merges, and it depends on the width
    through the cost of a bin's metadata.)"""
    kw = kw or classic(level)
    for c in counts:
        bins = builder(c)
        if bins is None: return None
        n = sum(b[0] for b in bins) + (1 if kw["delta"] == DELTA_CONSECUTIVE else 0)
        bl = M.choose_unoptimized_bins_log(level, n)
        a_value_shares_a_slot = (n >> bl) > min(b[0] for b in bins)          # the histogram would not give one bin per value
        wrong_kernel = (bl > 8) != (section in "cd")                        # (c) and (d) are the block kernel's, the rest the one-wave kernel's
        not_the_route_boundary = section == "d" and bl != 9                 # (d): exactly 2^9 histogram bins
        too_small_for_c = section == "c" and n < 1 << 16                    # (c): level 12 at 2^16 numbers or more
        if a_value_shares_a_slot or wrong_kernel or not_the_route_boundary or too_small_for_c: continue
        case = Case(name, section, bits, kw, var, bins, dict(ties=ties), "tie_smallest_j")
        if check_edge(case, M.train(bins, bits, bl, sum(b[0] for b in bins))) is None:
            return case
    return None


def cases_a():
    """(a) adjacent ties of the one-wave kernel, the tied pair on both sides of every slot boundary, inside a slot and at the last bin."""
    out = []
    for bits in WIDTHS:
        if bits == 8:   # 256 values hold 21 triples behind two fillers: the pair {63, 64} at the last bin
            out.append(_tie_case("a-w8-front2-21triples", "a", 8, 8, lambda c: layout(8, [c // 2, c // 2], triple_structure(8, 21, c), []),
                                 {34: [33, 34], 64: [63, 64]}))
            continue
        out.append(_tie_case(f"a-w{bits}-front2-84triples", "a", bits, 8, lambda c: layout(bits, [2 * c, 2 * c], triple_structure(bits, 84, c), []),
                             {34: [33, 34], 64: [63, 64]}))
        out.append(_tie_case(f"a-w{bits}-front0-85triples", "a", bits, 8, lambda c: layout(bits, [], triple_structure(bits, 85, c), [c]),
                             {2: [1, 2], 128: [127, 128]}))
        out.append(_tie_case(f"a-w{bits}-front1-85triples", "a", bits, 8, lambda c: layout(bits, [c], triple_structure(bits, 85, c), []),
                             {192: [191, 192], 255: [254, 255]}))
    return out


def cases_b():
    """(b) ties a slot apart in one lane (the 192-run: slots 1/2, 2/3 and, with the sparse prefix, 0/1) and in different lanes of
    different slots (the 129-run)."""
    out = [_tie_case("b-w8-run192-slots12", "b", 8, 8, lambda c: layout(8, [], run_structure(192, c), [64 * c]), {191: [64, 128]}),
           _tie_case("b-w8-run129-lanes1+0", "b", 8, 8, lambda c: layout(8, [], run_structure(129, c), pow2_parts(127 * c)), {128: [1, 128]})]
    for bits in WIDTHS[1:]:
        out.append(_tie_case(f"b-w{bits}-run192-slots12", "b", bits, 8, lambda c: layout(bits, [], run_structure(192, c), [64 * c]), {191: [64, 128]}))
        out.append(_tie_case(f"b-w{bits}-run192-slots23", "b", bits, 8, lambda c: layout(bits, [c] * 64, run_structure(192, c), []), {255: [128, 192]}))
        out.append(_tie_case(f"b-w{bits}-run192-sparse-slots01", "b", bits, 8, lambda c: layout(bits, [], run_structure(192, c, True), [64 * c]), {159: [32, 96]}))
        out.append(_tie_case(f"b-w{bits}-run129-lanes1+0", "b", bits, 8, lambda c: layout(bits, [], run_structure(129, c), pow2_parts(127 * c)), {128: [1, 128]}))
        out.append(_tie_case(f"b-w{bits}-run129-lanes63+62", "b", bits, 8, lambda c: layout(bits, [c] * 62, run_structure(129, c), pow2_parts(65 * c)), {190: [63, 190]}))
    return out


def _big(name, builder, ties, bits=32, counts=(16, 32, 64, 128)):
    return _tie_case(name, "c", bits, 12, builder, ties, counts)


def cases_c():
    """(c) the block kernel at level 12: the tied pair in one wave (triples), across waves 0 and 1 (the 129-run, and the 192-run by 64),
    across waves 0 and 15 (the 1025-run; the runs at 32 and 64 bits only -- each is a DP of a thousand bins and more in the model, the oracle
    and the exact check, and the widths go through the block kernel with the triples at 1024 bins), with the deciding step below 64 (one active wave; only the triples reach it: a run's last step
    is at least its length), between 64 and 1023 and from 1024 on; histograms of 257, 1023, 1024, 1025, 4095 and 4096 bins."""
    tri = lambda bits, n, c: triple_structure(bits, n, c)
    total = 1 << 16
    rest = lambda c, used: pow2_parts(total - used * c)
    out = [
        _big("c-w64-nb257-85triples", lambda c: layout(64, [], tri(64, 85, c), [c, 256 * c]), {2: [1, 2], 254: [253, 254]}, bits=64),   # (as the 129-run)
        _big("c-nb1023-340triples", lambda c: layout(32, [], tri(32, 340, c), [c, c, 2 * c]), {1019: [1018, 1019]}),
        _big("c-nb1025-341triples", lambda c: layout(32, [c // 2, c // 2], tri(32, 341, c), []), {4: [3, 4], 64: [63, 64], 1024: [1023, 1024]}),
        _big("c-nb4095-1364triples", lambda c: layout(32, [], tri(32, 1364, c), [c, c, 2 * c]), {1025: [1024, 1025], 4091: [4090, 4091]}),
        _big("c-nb4096-1365triples", lambda c: layout(32, [], tri(32, 1365, c), [c]), {2: [1, 2], 1025: [1024, 1025], 4094: [4093, 4094]}),
        # (64-bit: at 32 bits the 127 bins the run saves are worth less than 0.1 bits a number at 2^16 numbers, and the trivial shortcut fires)
        _big("c-w64-run129-step128", lambda c: layout(64, [], run_structure(129, c), rest(c, 129)), {128: [1, 128]}, bits=64, counts=(16,)),
        _big("c-w64-run129-step1028", lambda c: layout(64, [c] * 900, run_structure(129, c), rest(c, 1029)), {1028: [901, 1028]}, bits=64, counts=(16,)),
        _big("c-run192-step191", lambda c: layout(32, [], run_structure(192, c), rest(c, 192)), {191: [64, 128]}, counts=(16,)),
        _big("c-run192-step1091", lambda c: layout(32, [c] * 900, run_structure(192, c), rest(c, 1092)), {1091: [964, 1028]}, counts=(16,)),
        _big("c-run1025-step1024", lambda c: layout(32, [], run_structure(1025, c), rest(c, 1025)), {1024: [1, 1024]}, counts=(16,)),
        _big("c-run1025-step2024", lambda c: layout(32, [c] * 1000, run_structure(1025, c), rest(c, 2025)), {2024: [1001, 2024]}, counts=(16,)),
    ]
    for bits in WIDTHS[1:]:
        out.append(_big(f"c-w{bits}-nb1024-341triples", lambda c: layout(bits, [], tri(bits, 341, c), [c]), {2: [1, 2], 1022: [1021, 1022]}, bits=bits))
    return out


def cases_d():
    """(d) bin lists of (a) and (b), at most 256 bins, through enc_train_big_kernel: level 9 with enough numbers for 2^9 histogram bins."""
    out = []
    for bits in WIDTHS:
        if bits == 8:
            out.append(_tie_case("d-w8-run192-slots12", "d", 8, 9, lambda c: layout(8, [], run_structure(192, c), [64 * c]), {191: [64, 128]}, counts=(32, 64, 128)))
            continue
        out.append(_tie_case(f"d-w{bits}-front1-85triples", "d", bits, 9, lambda c: layout(bits, [c], triple_structure(bits, 85, c), []),
                             {192: [191, 192], 255: [254, 255]}, counts=(32, 64, 128)))
        out.append(_tie_case(f"d-w{bits}-run192-slots23", "d", bits, 9, lambda c: layout(bits, [c] * 64, run_structure(192, c), []), {255: [128, 192]}, counts=(32, 64, 128)))
    return out

def _far(bits, k):
    """The k-th of a few single values far from each other."""
    return {8: 37 * k + 3, 16: 4099 * k + 17}.get(bits, (1 << 24) + (1 << 20) * k)


def _pairs(bits, n_pairs, c, f):
    """n_pairs pairs of adjacent values of count c, far from each other, and one far value of count f: every bin is one value, the best
    partition merges each pair (one offset bit costs what the halved weight saves) and so saves one bin's metadata per pair."""
    return [(c, _far(bits, k) + d, _far(bits, k) + d) for k in range(n_pairs) for d in range(2)] + [(f, (1 << bits) - 1, (1 << bits) - 1)]


SINGLE_EQUAL = {16: (2581, 1209), 32: (4491, 2111), 64: (4387, 1998)}     # (count of v, count of v + 1): single_cost == best + 0.1f * n in f32
TRIVIAL_EQUAL = {16: (47, 588), 32: (200, 210), 64: (46, 2124)}           # (count per pair value, count of the far value): trivial == threshold


def cases_e():
    """(e) the two shortcuts from both sides, at 16, 32 and 64 bits (a bin's metadata, and with it every threshold, depends on the width;
    8 bits has no room for far values).  Each pair is one count apart: on one side the comparison is an EQUALITY in f32 ('<' fails, '<='
    would hold), on the other it holds.  The counts are what sweeps of the model found per width (the single-bin pair: two adjacent
    values, the first swept against the second; the trivial pair: three pairs of adjacent values and a far one, swept at the total for
    which 0.1f * n rounds to three bins' metadata -- 870, 1410 and 2400 numbers -- where exact arithmetic would call the product larger)."""
    out = []
    for bits in (16, 32, 64):
        a = _far(bits, 1)
        two = lambda c1, c2: [(c1, a, a), (c2, a + 1, a + 1)]
        (s1, s2), (tc, tf) = SINGLE_EQUAL[bits], TRIVIAL_EQUAL[bits]
        case = lambda tag, bins, edge, variant: Case(f"e-w{bits}-{tag}", "e", bits, classic(8), "primary", bins, edge, variant)
        out += [
            case("single-equal", two(s1, s2), dict(shortcut="trivial", holds=(False, True), single_equal=True), "single_le"),
            case("single-holds", two(s1 - 1, s2), dict(shortcut="single", holds=(True, True)), "no_shortcuts"),
            case("trivial-equal", _pairs(bits, 3, tc, tf), dict(shortcut=None, holds=(False, False), trivial_equal=True), "trivial_le"),
            case("trivial-holds", _pairs(bits, 3, tc, tf + 1), dict(shortcut="trivial", holds=(False, True)), "no_shortcuts"),
            case("both-hold", two(2048, 2048), dict(shortcut="single", holds=(True, True)), "trivial_first"),
            # the trivial cost would be under the threshold by a wide margin, but the first bin is two values wide
            case("all-trivial-but-one", [(8, 0, 1)] + _pairs(bits, 3, tc, 2 * tf), dict(shortcut=None, holds=(False, False), one_wide=True), "trivial_unchecked"),
        ]
    return out


# (f) count vectors of 2 to 8 bins found by a seeded random search with the model, at level 8 and 16 384 numbers: 2^8 histogram bins of 64
# numbers, a table of 2^10, so that a count c wants c / 16 of it.  Counts of 128 and more are bins of their own; a count under 16 between two
# such is one too (the wide run behind it closes its bin) and wants less than one weight -- its surplus is cut off at zero.
QUANT_VECTORS = collections.OrderedDict([
    ("half", ([584, 3192, 712, 2128, 9768], dict(halves=("min", 1), n_dec=("min", 1)), ("half_even", "truncate"))),
    ("decrement-past-a-one", ([2728, 1, 2128, 4, 1020, 1536, 288, 8679], dict(n_dec=("min", 1), dec_skipped_ones=("min", 1)), ("skip_decrement",))),
    ("increment", ([1632, 1672, 9, 1144, 448, 1568, 9911], dict(n_inc=("min", 1)), ("skip_increment",))),
    ("increment-twice", ([1176, 2984, 884, 1212, 1096, 9, 820, 8203], dict(n_inc=("min", 2)), ("skip_increment",))),
    ("surplus-cut-at-zero", ([500, 3136, 144, 5, 652, 940, 11007], dict(), ("no_surplus_floor",))),
    ("all-even-by-4", ([960, 3144, 12280], dict(pow2=2, size_log=8), ("no_pow2",))),
    ("all-even-down-to-1-1", ([8192, 8192], dict(pow2=9, size_log=1, weights=[1, 1]), ("no_pow2",))),
])


def cases_f():
    """(f) quantize_weights.  min_size_log > estimated_ans_size_log cannot be reached through a chunk: a variable has at most
    min(2^bins_log, n) <= 2^12 bins, and the estimate is min(bins_log + 2, 12, ceil(log2 n)), never below the logarithm of that.  One
    dominant bin beside 255 bins that want less than one weight (weights 1 ... 1, 769 at size 10) cannot either: a bin that wants less than one
    weight holds less than a quarter of a histogram slot and only closes as a bin of its own in front of a run of two slots or more, so
    at most half the bins of a chunk are such; test_train_model.py pins that vector on quantize_weights itself."""
    out = []
    for bits in (16, 32, 64):   # (the quantiser itself does not see the width; the thread that runs it is compiled per width)
        for tag, (counts, quant, variants) in QUANT_VECTORS.items():
            for variant in variants:
                bins = [(c, _far(bits, k), _far(bits, k)) for k, c in enumerate(counts)]
                out.append(Case(f"f-w{bits}-{tag}" + (f"-{variant}" if len(variants) > 1 else ""), "f", bits, classic(8), "primary", bins, dict(quant=quant), variant))
    # the estimate clamped by the number of latents: 300 numbers at level 12 have 2^8 histogram bins, but ceil(log2 300) = 9 < 8 + 2
    out.append(Case("f-estimate-clamped-by-n", "f", 32, classic(12), "primary", [(c, _far(32, k), _far(32, k)) for k, c in enumerate((118, 90, 59, 33))],
                    dict(quant=dict(size_log=9), est=9), "est_no_n_clamp"))
    # desired_surplus == 0 with as many bins as the table has states: 4096 far values 16 times each at level 12 (fewer numbers per value
    # and the DP merges them: a bin's metadata costs more than their offsets)
    out.append(Case("f-zero-surplus-full-table", "f", 32, classic(12), "primary", [(16, k << 20, k << 20) for k in range(4096)],
                    dict(quant=dict(desired_zero=True, full=True, size_log=12)), "no_zero_surplus_guard"))
    return out


def cases_g():
    """(g) the secondary of an int-mult chunk with 200 distinct values, capped at 2^6 histogram bins in both kernels; a tie case as order-1
    differences; lookback chunks of 16, 32 and 64-bit numbers whose DELTA variable -- the lookbacks, 32-bit whatever the numbers are --
    holds five triples (lookback_numbers), through the one-wave kernel (level 8) and the block kernel (level 12: 2^9 histogram bins)."""
    int_mult = lambda level: dict(level=level, mode=MODE_INT_MULT, mode_u64=1000, delta=DELTA_NONE)
    deltas = dict(level=8, mode=MODE_CLASSIC, delta=DELTA_CONSECUTIVE, delta_order=1)
    out = [Case("g-int-mult-secondary-L8", "g", 32, int_mult(8), "secondary", None, dict(capped=True), "secondary_uncapped"),
           Case("g-int-mult-secondary-L12", "g", 32, int_mult(12), "secondary", None, dict(capped=True), "secondary_uncapped")]
    for bits in (16, 32, 64):
        out.append(_tie_case(f"g-w{bits}-order1-85triples", "g", bits, 8, lambda c: layout(bits, [c], triple_structure(bits, 85, c), []),
                             {192: [191, 192], 255: [254, 255]}, kw=deltas))
        for level in (8, 12):
            out.append(Case(f"g-w{bits}-lookback-5triples-L{level}", "g", bits, dict(level=level, mode=MODE_CLASSIC, delta=DELTA_LOOKBACK), "delta", None,
                            dict(lookback_triples=list(LOOKBACK_TRIPLES)), "tie_smallest_j"))
    return out


LOOKBACK_TRIPLES, LOOKBACK_COUNT, LOOKBACK_FILLER, LOOKBACK_N = (70, 80, 90, 100, 110), 64, 131, 2049


@functools.lru_cache(maxsize=None)
def lookback_numbers(bits):
    """2049 numbers whose 2048 lookbacks hold each of 70, 71, 72, 80 ... 112 exactly 64 times: wide random values, then stretches that repeat
    what lies P back (x[i] = x[i - P]: the search's hash proposes P and nothing else comes near) -- first P = 131 as the filler, then the
    fifteen periods in DESCENDING order, so that a switch of period drops a value and never doubles one (a doubled value would make
    lookback 1 exact too).  The few strays (the filler's opening, a period that lingers among the repeating proposals) land on other
    lookbacks; where one lands on a triple's value the stretch lengths are corrected by what the plain model of the search counts, until
    every count is 64.  The total, 2048, is a power of two, and so is every count of a triple: the tie inside a triple is exact in f32
    whatever the strays' bins cost in front of it, as long as the additions stay inside one binade -- which check_edge asks the model."""
    values = sorted((v + d for v in LOOKBACK_TRIPLES for d in range(3)), reverse=True)
    for seed in range(8):      # (a correction moves everything behind it: a seed that does not settle in a few rounds is given up)
        lens = {v: LOOKBACK_COUNT for v in values}
        fresh = LM.wide(np.random.default_rng(seed), LOOKBACK_N, bits)
        for _ in range(6):
            segments = [(LOOKBACK_FILLER, LOOKBACK_N - 1 - sum(lens.values()))] + [(v, lens[v]) for v in values]
            x = [fresh[0]]
            for period, length in segments:
                for _ in range(length):
                    i = len(x)
                    x.append(x[i - period] if i >= period else fresh[i])
            counts = collections.Counter(LM.choose_lookbacks(x, bits, LM.window_log(LOOKBACK_N)))
            if all(counts[v] == LOOKBACK_COUNT for v in values):
                return np.array(x, DT[bits])
            for v in values:
                lens[v] = max(lens[v] + LOOKBACK_COUNT - counts[v], 1)
    raise AssertionError("the lookbacks could not be steered")


def int_mult_numbers(level):
    """1000 q + r: four quotients, 200 remainders of almost equal counts."""
    n = 1 << (13 if level == 8 else 16)
    rng = np.random.default_rng(level)
    r = rng.permutation(n) % 200
    q = rng.integers(0, 4, n) * 7 + 1
    return (q * 1000 + r).astype(np.uint32)


FALLBACK_REPEATS = 64


def fallback_latents(c_wide):
    """The family of (h): order-1 differences of a u16 -- c_wide values spread evenly over 60 000 (one bin of 16 offset bits, which costs a bit
    more than it saves) and 64 times the type's maximum (a bin without offsets): every further wide value adds one bit to worst - baseline."""
    return np.concatenate([(np.arange(c_wide, dtype=np.uint64) * 60000 // c_wide).astype(np.uint16), np.full(FALLBACK_REPEATS, 65535, np.uint16)])


def _fallback_case(c_wide, d, variant):
    return Case(f"h-fallback-{d:+d}-wide{c_wide}", "h", 16, dict(level=8, mode=MODE_CLASSIC, delta=DELTA_CONSECUTIVE, delta_order=1), "primary", None,
                dict(fallback=d), variant)


@functools.lru_cache(maxsize=None)
def fallback_sweep():
    """{worst - baseline: [c_wide, ...]} over the family, by the model."""
    out = collections.defaultdict(list)
    for c_wide in range(640, 740):
        lat = fallback_latents(c_wide)
        n = lat.size + 1
        ubl = M.choose_unoptimized_bins_log(8, n)
        h, _ = O.histogram(lat, ubl, rule=1)
        _, worst, baseline = M.should_fallback({"primary": M.train(h, 16, ubl, lat.size)}, n, 16, "classic", "consecutive", 1)
        out[worst - baseline].append(c_wide)
    return out


def cases_h():
    """(h) should_fallback one byte under, at, and one byte over equality: the last size of the sweep with worst - baseline = -1, the first
    and the last with 0, the first with +1."""
    s = fallback_sweep()
    return [_fallback_case(s[-1][-1], -1, ("worst_one_byte_more", "fallback_ge")), _fallback_case(s[0][0], 0, "fallback_ge"), _fallback_case(s[0][-1], 0, "fallback_ge"),
            _fallback_case(s[1][0], 1, "worst_one_byte_less")]


SECTIONS = collections.OrderedDict([("a", cases_a), ("b", cases_b), ("c", cases_c), ("d", cases_d), ("e", cases_e), ("f", cases_f), ("g", cases_g), ("h", cases_h)])


@functools.lru_cache(maxsize=None)
def section(s):
    return tuple(SECTIONS[s]())


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(c for s in SECTIONS for c in section(s) if c is not None)


@functools.lru_cache(maxsize=None)
def BY_NAME():
    return {c.name: c for c in all_cases()}


@functools.lru_cache(maxsize=None)
def numbers(name):
    """The case's numbers (read-only: the tests share them)."""
    c = BY_NAME()[name]
    if c.kw["delta"] == DELTA_LOOKBACK:
        lat = lookback_numbers(c.bits)
    elif c.section == "g" and c.bins is None:
        lat = int_mult_numbers(c.kw["level"])
    elif c.section == "h":
        lat = fallback_latents(int(name.split("wide")[1]))
        np.random.default_rng(lat.size).shuffle(lat)
    else:
        lat = numbers_of(c.bins, c.bits, seed=len(name))
    if c.kw["delta"] == DELTA_CONSECUTIVE:
        lat = from_differences(lat, c.bits)
    lat.setflags(write=False)
    return lat
