"""A plain model of the encoder's training step, written from the reference's text: bin_optimization.rs (log2_approx, bin_cost, the
partition DP, its two shortcuts, the rewind), ans/encoding.rs (quantize_weights_to, quantize_weights) and wrapped/chunk_compressor.rs
(choose_unoptimized_bins_log, train_infos' estimated_ans_size_log, the secondary's bin cap, should_fallback).

Arithmetic is NumPy float32, one rounded operation at a time, nothing fused.  The DP is vectorised over j inside a step (the reference
scans j = i .. 0 with '<': the LARGEST j among the candidates of minimal cost wins; the model takes the minimum and then that j).

Besides the answer every function returns a report of what a test needs to certify that a case sits on an edge: per DP step the set of
candidates that tie for the minimum, which shortcut fired, each float weight before rounding, what the repair loops did, the power-of-two
reduction.  `variants` (a set of names from VARIANTS) switches one rule to a plausible wrong one; the tests use them ONLY to prove that a
case discriminates -- a case whose answer does not change under its variant tests nothing.

exact=True runs the DP in integers instead: every log2_approx value of an integer >= 2 is a multiple of 2^-23, so costs scaled by 2^23
are exact in int64 (the thresholds are compared as Fractions, 0.1f being the rational it is).  On a case built from powers of two the f32
run has to agree with it; quantize_weights_to has the same switch, in Fractions."""
import collections
from fractions import Fraction

import numpy as np

f32 = np.float32
VARIANTS = ("tie_smallest_j", "single_le", "trivial_le", "no_shortcuts", "half_even", "truncate", "skip_decrement", "skip_increment",
            "no_pow2", "est_no_n_clamp", "secondary_uncapped", "fallback_ge",
            # beyond the issue's list, for the cases none of the above can move:
            "trivial_first", "trivial_unchecked", "no_surplus_floor", "no_zero_surplus_guard", "worst_one_byte_more", "worst_one_byte_less")

MAX_COMPRESSION_LEVEL = 12
LIMITED_UNOPTIMIZED_BINS_LOG = 6
BITS_TO_ENCODE_ANS_SIZE_LOG, BITS_TO_ENCODE_N_BINS, BITS_TO_ENCODE_MODE_VARIANT, BITS_TO_ENCODE_QUANTIZE_K = 4, 15, 4, 8
DELTA_MAX_BIT_SIZE = 4 + 5 + 5 + 64 + 32 * 32
ANS_INTERLEAVING = 4
SCALE_LOG = 23

# log2_approx's constants, each one f32 operation
_Z = f32(0.674)
_SIGNIF_MASK = np.uint32(0x7FFFFF)
_Z_SIGNIF = np.array(_Z).view(np.uint32) & _SIGNIF_MASK
_B = f32(2.0) / _Z
_C = -_B / (f32(6.0) * _Z)
_A = -_B - _C
_POW2 = np.array([1 << k for k in range(64)], np.uint64)


def _variants(variants):
    v = frozenset(variants or ())
    assert v <= set(VARIANTS), v - set(VARIANTS)
    return v


def log2_approx(x):
    """bin_optimization.rs:19-43 on a float32 scalar or array."""
    x = np.asarray(x, f32)
    bits = x.view(np.uint32)
    exp = bits >> np.uint32(23)
    signif = bits & _SIGNIF_MASK
    high_bit = (signif > _Z_SIGNIF).astype(np.uint32)
    log_int = (exp + high_bit).astype(np.int64) - 127
    normalized = (((np.uint32(0x7F) ^ high_bit) << np.uint32(23)) | signif).view(f32)
    inner = _B + _C * normalized
    return (log_int.astype(f32) + _A) + normalized * inner


def bits_to_encode_offset(max_offset):
    """bits.rs:20: the bit length of upper - lower (Python ints or a uint64 array)."""
    if isinstance(max_offset, np.ndarray):
        return np.searchsorted(_POW2, max_offset.astype(np.uint64), side="right")
    return int(max_offset).bit_length()


def bits_to_encode_offset_bits(latent_bits):
    return int(latent_bits).bit_length()


def bin_meta_cost(latent_bits, ans_size_log):
    """Bin::exact_bit_size"""
    return ans_size_log + latent_bits + bits_to_encode_offset_bits(latent_bits)


def bin_cost(meta, lower, upper, count, total_log2):
    """bin_optimization.rs:46-57; count and the bounds may be arrays."""
    count_f = np.asarray(count).astype(f32)
    ans_cost = f32(total_log2) - log2_approx(count_f)
    offset_cost = np.asarray(bits_to_encode_offset(np.asarray(upper, np.uint64) - np.asarray(lower, np.uint64))).astype(f32)
    return f32(meta) + (ans_cost + offset_cost) * count_f


def _log2_scaled(count):
    """log2_approx(count) * 2^23 as exact integers (count: integer array, every entry >= 1)."""
    v = log2_approx(np.asarray(count).astype(f32)).astype(np.float64) * float(1 << SCALE_LOG)
    assert (v == np.floor(v)).all()
    return v.astype(np.int64)


def _bin_cost_scaled(meta, lower, upper, count, total_log2_s):
    count = np.asarray(count, np.int64)
    ob = np.asarray(bits_to_encode_offset(np.asarray(upper, np.uint64) - np.asarray(lower, np.uint64))).astype(np.int64)
    return (np.int64(meta) << SCALE_LOG) + ((total_log2_s - _log2_scaled(count)) + (ob << SCALE_LOG)) * count


DpReport = collections.namedtuple("DpReport", "best_js ties best_cost single_cost trivial_cost threshold shortcut partitioning")


def choose_optimized_partitioning(bins, latent_bits, ans_size_log, variants=None, exact=False):
    """bin_optimization.rs:104-178.  bins: [(count, lower, upper)].  ties: {i: [every j whose cost equals the step's minimum]} for the steps
    with more than one such j.  With exact=True the costs are integers scaled by 2^23."""
    v = _variants(variants)
    nb = len(bins)
    counts = np.array([b[0] for b in bins], np.int64)
    lowers = np.array([b[1] for b in bins], np.uint64)
    uppers = np.array([b[2] for b in bins], np.uint64)
    cc = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(cc[-1])
    assert total < 1 << 24
    meta = bin_meta_cost(latent_bits, ans_size_log)
    if exact:
        tl = int(_log2_scaled(np.array([total]))[0])
        cost_fn = lambda lo, up, c: _bin_cost_scaled(meta, lo, up, c, tl)
        best = np.zeros(nb + 1, np.int64)
    else:
        tl = log2_approx(f32(total))
        cost_fn = lambda lo, up, c: bin_cost(f32(meta), lo, up, c, tl)
        best = np.zeros(nb + 1, f32)
    best_js = np.zeros(nb, np.int64)
    ties = {}
    for i in range(nb):
        cost = best[:i + 1] + cost_fn(lowers[:i + 1], uppers[i], cc[i + 1] - cc[:i + 1])
        m = cost.min()
        js = np.flatnonzero(cost == m)
        best[i + 1] = m
        best_js[i] = js[0] if "tie_smallest_j" in v else js[-1]
        if js.size > 1:
            ties[i] = js.tolist()
    best_cost = best[nb]
    single = cost_fn(lowers[0], uppers[nb - 1], total)
    all_trivial = bool((lowers == uppers).all()) or "trivial_unchecked" in v
    if exact:
        tenth = Fraction(float(f32(0.1)))
        threshold = Fraction(int(best_cost), 1 << SCALE_LOG) + tenth * total
        single_c = Fraction(int(single), 1 << SCALE_LOG)
        trivial_c = Fraction(int(sum(int(x) for x in cost_fn(lowers, uppers, counts))), 1 << SCALE_LOG) if all_trivial else None
    else:
        threshold = best_cost + f32(0.1) * f32(total)
        single_c = f32(single)
        trivial_c = None
        if all_trivial:
            trivial_c = f32(0.0)
            for x in cost_fn(lowers, uppers, counts):       # the reference sums in order
                trivial_c = trivial_c + x
    shortcut = None
    if "no_shortcuts" not in v:
        single_holds = single_c <= threshold if "single_le" in v else single_c < threshold
        trivial_holds = all_trivial and (trivial_c <= threshold if "trivial_le" in v else trivial_c < threshold)
        if "trivial_first" in v and trivial_holds:
            shortcut = "trivial"
        elif single_holds:
            shortcut = "single"
        elif trivial_holds:
            shortcut = "trivial"
    if shortcut == "single":
        part = [(0, nb - 1)]
    elif shortcut == "trivial":
        part = [(i, i) for i in range(nb)]
    else:
        part = rewind_best_partitioning(best_js, nb)
    return part, DpReport(best_js, ties, best_cost, single_c, trivial_c, threshold, shortcut, part)


def rewind_best_partitioning(best_js, n_bins):
    part = []
    i = n_bins - 1
    while True:
        j = int(best_js[i])
        part.append((j, i))
        if j > 0:
            i = j - 1
        else:
            break
    part.reverse()
    return part


def optimize_bins(bins, latent_bits, ans_size_log, variants=None, exact=False):
    """bin_optimization.rs:180-198: ([(weight, lower, upper, offset_bits)], DpReport)."""
    part, rep = choose_optimized_partitioning(bins, latent_bits, ans_size_log, variants, exact)
    out = []
    for j, i in part:
        count = sum(int(b[0]) for b in bins[j:i + 1])
        out.append((count, int(bins[j][1]), int(bins[i][2]), bits_to_encode_offset(int(bins[i][2]) - int(bins[j][1]))))
    return out, rep


def _round(x, v):
    """f32::round (half away from zero), or a variant's rounding, of a non-negative float32 / Fraction."""
    fl = int(x)
    frac = x - fl
    half = Fraction(1, 2) if isinstance(x, Fraction) else 0.5
    if "truncate" in v:
        return fl
    if "half_even" in v and frac == half:
        return fl + (fl & 1)
    return fl + (1 if frac >= half else 0)


QuantReport = collections.namedtuple("QuantReport", "float_weights rounded n_dec n_inc dec_skipped_ones desired_surplus sum_ok")


def quantize_weights_to(counts, total_count, size_log, variants=None, exact=False):
    """ans/encoding.rs:95-151.  dec_skipped_ones: bins of weight 1 the decrement loop passed on its way -- it may not take from them.  sum_ok: the weights add up to 2^size_log (always, without a variant)."""
    v = _variants(variants)
    if size_log == 0:
        return [1], QuantReport([], [1], 0, 0, 0, 0, True)
    required = 1 << size_log
    if exact:
        num = lambda x: Fraction(x)
        one, zero = Fraction(1), Fraction(0)
    else:
        num = lambda x: f32(x)
        one, zero = f32(1.0), f32(0.0)
    multiplier = num(required) / num(total_count)
    surplus = [num(c) * multiplier - one for c in counts]
    if "no_surplus_floor" not in v:
        surplus = [max(x, zero) for x in surplus]
    desired = zero
    for s in surplus:
        desired = desired + s
    required_surplus = required - len(counts)
    if desired == 0 and "no_zero_surplus_guard" in v:      # 0 / 0: every float weight is NaN, which casts to 0 and compares false
        return [0] * len(counts), QuantReport([float("nan")] * len(counts), [0] * len(counts), 0, 0, 0, desired, False)
    surplus_mult = zero if desired == 0 else num(required_surplus) / desired
    fw = [one + s * surplus_mult for s in surplus]
    weights = [max(_round(x, v), 0) if x > 0 else 0 for x in fw]
    rounded = list(weights)
    weight_sum = sum(weights)
    n_dec = n_inc = skipped = 0
    i = 0
    while weight_sum > required and i < len(weights) and "skip_decrement" not in v:
        if weights[i] > 1 and num(weights[i]) > fw[i]:
            weights[i] -= 1; weight_sum -= 1; n_dec += 1
        elif weights[i] == 1:
            skipped += 1
        i += 1
    i = 0
    while weight_sum < required and i < len(weights) and "skip_increment" not in v:
        if num(weights[i]) < fw[i]:
            weights[i] += 1; weight_sum += 1; n_inc += 1
        i += 1
    return weights, QuantReport(fw, rounded, n_dec, n_inc, skipped, desired, weight_sum == required)


def quantize_weights(counts, total_count, max_size_log, variants=None, exact=False):
    """ans/encoding.rs:156-175: (size_log, weights, (min_size_log, size_log before the reduction, power_of_2, QuantReport))."""
    v = _variants(variants)
    if len(counts) == 1:
        return 0, [1], (0, 0, 0, None)
    min_size_log = (len(counts) - 1).bit_length()
    size_log = max(min_size_log, max_size_log)
    weights, rep = quantize_weights_to(counts, total_count, size_log, v, exact)
    power_of_2 = 0 if "no_pow2" in v else min(((w & -w).bit_length() - 1) if w else 32 for w in weights)
    return size_log - power_of_2, [w >> power_of_2 for w in weights], (min_size_log, size_log, power_of_2, rep)


def choose_unoptimized_bins_log(level, n):
    """chunk_compressor.rs:362-371"""
    log_n = int(n).bit_length() - 1
    fast = max(log_n - 4, 0)
    return level if level <= fast else fast + max(level - fast, 0) // 2


def var_bins_log(unoptimized_bins_log, key, variants=None):
    """new_candidate: the secondary is trained on at most 2^6 histogram bins."""
    if key == "secondary" and "secondary_uncapped" not in _variants(variants):
        return min(unoptimized_bins_log, LIMITED_UNOPTIMIZED_BINS_LOG)
    return unoptimized_bins_log


def estimated_ans_size_log(bins_log, n_latents, variants=None):
    """train_infos: min(bins_log + 2, 12, ceil(log2(n_latents)))"""
    est = min(bins_log + 2, MAX_COMPRESSION_LEVEL)
    if "est_no_n_clamp" in _variants(variants):
        return est
    return min(est, 0 if n_latents <= 1 else (n_latents - 1).bit_length())


Plan = collections.namedtuple("Plan", "latent_bits ans_size_log weights lowers offset_bits counts est dp quant")


def train(bins, latent_bits, bins_log, n_latents, variants=None, exact=False):
    """train_infos after the histogram: `bins` is the histogram of the variable's n_latents latents at `bins_log` (its own, capped for a
    secondary by var_bins_log)."""
    est = estimated_ans_size_log(bins_log, n_latents, variants)
    infos, dp = optimize_bins(bins, latent_bits, est, variants, exact)
    counts = [b[0] for b in infos]
    size_log, weights, quant = quantize_weights(counts, n_latents, est, variants, exact)
    return Plan(latent_bits, size_log, weights, [b[1] for b in infos], [b[3] for b in infos], counts, est, dp, quant)


def should_fallback(plans, n, number_bits, mode="classic", delta="none", delta_order=0, state_n_log=0, n_pages=1, variants=None):
    """chunk_compressor.rs:502-541.  plans: {"delta" | "primary" | "secondary": Plan}; mode: classic, int_mult, float_mult, float_quant;
    delta: none, consecutive, lookback.  Returns (fallback, worst, baseline) with both sizes in bytes; a Classic chunk without delta is
    never compared: (False, None, None)."""
    if mode == "classic" and delta == "none":
        return False, None, None
    worst_bits = 7 * n_pages
    meta_bits = BITS_TO_ENCODE_MODE_VARIANT + {"classic": 0, "int_mult": number_bits, "float_mult": number_bits,
                                               "float_quant": BITS_TO_ENCODE_QUANTIZE_K}[mode] + DELTA_MAX_BIT_SIZE
    page_meta_bits = 0
    for key, p in plans.items():
        for w, ob, c in zip(p.weights, p.offset_bits, p.counts):
            worst_bits += c * (ob + p.ans_size_log - (w.bit_length() - 1))
        meta_bits += BITS_TO_ENCODE_ANS_SIZE_LOG + BITS_TO_ENCODE_N_BINS + len(p.weights) * bin_meta_cost(p.latent_bits, p.ans_size_log)
        per_state = 0
        if key == "primary":
            per_state = {"none": 0, "consecutive": delta_order, "lookback": 1 << state_n_log}[delta]
        page_meta_bits += p.ans_size_log * ANS_INTERLEAVING + p.latent_bits * per_state
    worst = -(-meta_bits // 8) + n_pages * -(-page_meta_bits // 8) + -(-worst_bits // 8)
    worst += ("worst_one_byte_more" in _variants(variants)) - ("worst_one_byte_less" in _variants(variants))
    base_bits = BITS_TO_ENCODE_MODE_VARIANT + DELTA_MAX_BIT_SIZE + BITS_TO_ENCODE_ANS_SIZE_LOG + BITS_TO_ENCODE_N_BINS + bin_meta_cost(number_bits, 0)
    baseline = -(-base_bits // 8) + -(-(n * number_bits) // 8)
    return (worst >= baseline if "fallback_ge" in _variants(variants) else worst > baseline), worst, baseline
