"""A plain model of DeltaSpec::Auto (wrapped/chunk_compressor.rs:289-360, sampling.rs:27-60, delta/mod.rs:37-48), written from the reference's
text.  It shares no code with the oracle or the product and knows nothing of how a trial is encoded: its inputs are a chunk's length and
the nine size estimates of its sample -- candidate 0 no delta, 1 lookback WITHOUT its penalty, 1 + k consecutive order k -- as float32.

  sample_positions(n)       where the delta sample lies in a chunk of n numbers
  decide(costs, n)          the reference's sequential decision: (kind, order, window_n_log), kind 0 none / 1 consecutive / 2 lookback
  schedule(costs, n)        the bit mask of candidates the device's wave schedule trial-encodes: {0, 1, 2, 3} always, then {4, 5}, {6, 7}, {8},
                            a wave only while every order of the one before was an improvement
  batch(chunks)             one call of several chunks replayed the way the device lays it out: per wave a sub-list of the chunks that go on,
                            the wave's estimates candidate-major at [j * stride + k]; the decision and mask of every chunk

Every function takes the name of a wrong reading (VARIANTS); test_auto_delta_model.py shows that each one changes the rows that name it.
A reading under which the reference's arithmetic has no value (a division by zero, an index beyond the wave's list) gives UNDEFINED."""
import numpy as np

NONE, CONSECUTIVE, LOOKBACK = 0, 1, 2
MIN_SAMPLE, SAMPLE_RATIO, GROUP_N, MAX_ORDER = 10, 40, 200, 7
UNDEFINED = "undefined"
VARIANTS = ("global_minimum", "non_strict", "lookback_without_penalty", "window_from_sample", "stride_without_max", "raw_bits", "first_wave_stride")
F = np.float32


def sample_n(n):
    """the length of the delta sample: whole groups, so usually more than the target of 10 + (n - 10) / 40"""
    if n < MIN_SAMPLE: return 0
    target = MIN_SAMPLE + (n - MIN_SAMPLE) // SAMPLE_RATIO
    return -(-target // GROUP_N) * min(GROUP_N, n)


def sample_positions(n, variant=None):
    """the positions of the sample's latents in the chunk, in sample order"""
    if n < MIN_SAMPLE: return np.zeros(0, np.int64)
    target = MIN_SAMPLE + (n - MIN_SAMPLE) // SAMPLE_RATIO
    group_n = min(GROUP_N, n)
    n_groups = -(-target // GROUP_N)
    spare = max(n - n_groups * group_n, 0)
    gaps = n_groups - 1 if variant == "stride_without_max" else max(n_groups, 2) - 1
    if gaps == 0: return UNDEFINED
    stride = group_n + spare // gaps
    return (np.arange(n_groups, dtype=np.int64)[:, None] * stride + np.arange(group_n, dtype=np.int64)[None, :]).reshape(-1)


def window_log(n):
    """new_lookback: the bits of n - 1, kept within 4..15"""
    return min(max(int(n - 1).bit_length(), 4), 15)


def _better(cost, best, variant): return cost <= best if variant == "non_strict" else cost < best


def decide(costs, n, variant=None):
    sn = sample_n(n)
    if sn == 0: return (NONE, 0, 0)
    c = [F(x) for x in costs]
    penalty = F(0.25) * F(sn)
    lookback = c[1] if variant == "lookback_without_penalty" else F(c[1] + penalty)
    w = window_log(sn if variant == "window_from_sample" else n)
    if variant == "global_minimum":                                            # the cheapest of all nine, the first of equals
        all_costs = [c[0], lookback] + c[2:]
        j = int(np.argmin(np.array(all_costs, dtype=np.float64)))
        return (NONE, 0, 0) if j == 0 else (LOOKBACK, 0, w) if j == 1 else (CONSECUTIVE, j - 1, 0)
    best, best_cost = (NONE, 0, 0), c[0]
    if best_cost > penalty and _better(lookback, best_cost, variant): best, best_cost = (LOOKBACK, 0, w), lookback
    for order in range(1, MAX_ORDER + 1):
        if not _better(c[1 + order], best_cost, variant): break
        best, best_cost = (CONSECUTIVE, order, 0), c[1 + order]
    return best


WAVES = ((0, 1, 2, 3), (4, 5), (6, 7), (8,))                                   # candidates per wave


def schedule(costs, n):
    if sample_n(n) == 0: return 0
    stop = decide(costs, n)
    reached = stop[1] if stop[0] == CONSECUTIVE else 0                         # the last order that was an improvement
    mask = 0
    for wave in WAVES:
        mask |= sum(1 << c for c in wave)
        if reached < wave[-1] - 1: break                                       # the wave's last order was no improvement: nothing deeper
    return mask


def batch(chunks, variant=None):
    """chunks: [(costs or None, n)] of one call.  Replays the call wave by wave over flat candidate-major lists, the way the device holds the
    estimates: [(decision, mask)] per chunk.  `first_wave_stride` reads every wave with the first wave's stride."""
    k_all = len(chunks)
    out = [[(NONE, 0, 0), 0, None] for _ in range(k_all)]                      # decision, mask, best cost
    live = [i for i, (c, n) in enumerate(chunks) if sample_n(n)]
    first_stride = len(live)
    for w, wave in enumerate(WAVES):
        if not live: break
        flat = [F(chunks[i][0][c]) for c in wave for i in live]                # trial j of the wave's k-th chunk at [j * len(live) + k]
        stride = first_stride if variant == "first_wave_stride" else len(live)
        go_on = []
        for k, i in enumerate(live):
            n = chunks[i][1]; sn = sample_n(n); o = out[i]
            o[1] |= sum(1 << c for c in wave)
            idx = [j * stride + k for j in range(len(wave))]
            if max(idx) >= len(flat): o[0] = UNDEFINED; continue
            got = [flat[x] for x in idx]
            if w == 0:
                o[2] = got[0]
                penalty = F(0.25) * F(sn)
                lookback = F(got[1] + penalty)
                if o[2] > penalty and lookback < o[2]: o[0], o[2] = (LOOKBACK, 0, window_log(n)), lookback
                got = got[2:]; orders = (1, 2)
            else: orders = tuple(c - 1 for c in wave)
            more = True
            for order, cost in zip(orders, got):
                if not cost < o[2]: more = False; break
                o[0], o[2] = (CONSECUTIVE, order, 0), cost
            if more: go_on.append(i)
        live = go_on
    return [(o[0], o[1]) for o in out]
