"""The rows of the bit packers' edge suites (test_pack_layout_model.py on the CPU, test_gpu_pack_edges.py on the device).

Every byte the encoder emits passes through one of five packers: pack_run / pack_item_t ("general"), the shifted-copy branch of pack_run
("copy"), pack1_run / pack1_item ("lean<mask>", "lean<mask, wide>"), the packing waves of enc_walkp_kernel with enc_place_kernel ("walkp") and
the BitSink of enc_page_kernel ("page").  A row is a small array built so that the page the reference encoder writes for it sits on a branch
point or a shared word of the packer it is routed to; what a row claims is evaluated by pack_layout_model on the oracle's chunk, never taken
from the device.  Families:

  W  field widths: the widest offset of a batch decides between one, two and four puts per lane (16 / 32), recomputed per batch;
  S  staging: PackSink::reserve against its threshold, flushes ending on dword residues 0, 1 and 31;
  J  run joins: runs of 64 batches packed by separate waves that share their first and last dword, runs shorter than a dword;
  T  tails: a last batch of 1 .. 255 latents behind full ones, on every route;
  C  the shifted copy at sizes around its 16-byte steps, its four-step unroll and its run length;
  P  walk-and-pack, then place: bodies of 0, 1 and 31 bits modulo 32, bodies shorter than a dword, head ends on every byte residue;
  H  the bin table of the head at 63 .. 256 bins.

REQUIRED lists what the rows of a family must show between them; a row's `claims` are the conditions it is there for, and every one of
them must hold.  UNREACHABLE names the conditions no input can meet, with the reason."""
import collections
import functools

import numpy as np

import oracle_lib as O
import pack_layout_model as P

Row = collections.namedtuple("Row", "name family kw make route compact claims")
UINT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
CLASSIC = dict(level=8, mode=1, delta=1)
TAILS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255)
W64 = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 58, 59, 2, 3, 4)
W32 = (0, 1, 15, 16, 17, 26, 27, 2, 3, 4, 5, 6, 7, 8, 9, 10)
WSEC64 = (0, 1, 15, 16, 17, 31, 32, 33, 34, 35, 38, 39, 2, 3, 4, 5)     # secondaries under a base near 2^44: sixteen clusters 2^40 apart
WSEC32 = (0, 1, 15, 16, 17, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)         # ... under a base near 2^22: 2^18 apart
WPAGE = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 52, 53, 2, 3, 4)     # 512 clusters 2^55 apart have no room for 58 and 59 bits
NONE, PRIMARY, BOTH, LB_PRIMARY, LB_ONLY = (False, False, False), (False, True, False), (False, True, True), (True, True, False), (True, False, False)   # which variables hold 16-bit latents


# ---------------------------------------------------------------------------------------------------------------- building blocks
def clusters(bits, widths, per, sep, seed, order=None, base0=0):
    """len(widths) clusters of `per` numbers: cluster i spans exactly 2^widths[i] values from base0 + i << sep (both ends present).  `order`:
    None cluster after cluster (every batch of 256 has one width), else the seed of a permutation (every lane mixes widths)."""
    rng = np.random.default_rng(seed); parts = []
    for i, w in enumerate(widths):
        base = base0 + (i << sep)
        x = rng.integers(0, 1 << w, per, dtype=np.uint64) + np.uint64(base) if w else np.full(per, base, np.uint64)
        if w: x[0] = base; x[-1] = base + (1 << w) - 1; rng.shuffle(x)
        parts.append(x)
    a = np.concatenate(parts)
    if order is not None: a = a[np.random.default_rng(order).permutation(a.size)]
    return a.astype(UINT[bits])


def outliers(bits, seed, batches=(3, 17, 30), n=8192):
    """A heavy constant 0 and rare outliers over the whole type (one bin of full-width offsets), at positions 4 lane + k, k = 0..3, of
    lanes 0 and 63 of a few batches."""
    a = np.zeros(n, UINT[bits]); rng = np.random.default_rng(seed); top = (1 << bits) - 1
    for b in batches:
        for pos in (0, 1, 2, 3, 252, 253, 254, 255):
            a[b * 256 + pos] = rng.integers(1, top, dtype=np.uint64)
    a[batches[0] * 256] = 1; a[batches[0] * 256 + 255] = top
    return a


def uniform(bits, k, n, seed, base=0):
    """n numbers uniform in [base, base + 2^k), both ends present: one bin of k offset bits, no tANS."""
    a = np.random.default_rng(seed).integers(0, 1 << k, n, dtype=np.uint64) + np.uint64(base)
    a[0] = base
    if n > 1: a[n - 1] = base + (1 << k) - 1
    return a.astype(UINT[bits])


def spikes(bits, n, seed, base=5, out=77, k=30, span=16384):
    """`base` everywhere but for k positions among the first `span` and k among the last `span` numbers, which hold `out`: two bins without
    offset bits, runs of 64 batches a few dozen bits long between a first and a last run of a few hundred."""
    rng = np.random.default_rng(seed)
    a = np.full(n, base, UINT[bits])
    a[rng.choice(min(span, n), k, replace=False)] = out
    a[n - 1 - rng.choice(min(span, n), k, replace=False)] = out
    return a


def skewed(bits, n, seed, scale=1, top=16):
    """A few bins of unequal weight with narrow offsets (what enc_walkp_kernel qualifies)."""
    return ((np.random.default_rng(seed).geometric(0.3, n) % top) * scale).astype(UINT[bits])


def two_far(bits, n, seed, lo_span, far):
    """Two clusters `far` apart: several bins, full-width latents (the value range is beyond the 16-bit window)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, lo_span, n) + rng.integers(0, 2, n) * far).astype(UINT[bits])


def int_mult(bits, n, seed, base, q_top=16, r_top=3):
    rng = np.random.default_rng(seed)
    return ((rng.geometric(0.3, n) % q_top).astype(np.uint64) * np.uint64(base) + rng.integers(0, r_top, n).astype(np.uint64)).astype(UINT[bits])


def periodic(bits, n, seed, period=37, noise=3, top=1 << 12):
    """A period with a little noise: under a lookback delta, a lookback variable of a few bins and narrow differences."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, top, period)[np.arange(n) % period] + rng.integers(0, noise, n)).astype(UINT[bits])


def many_spikes(bits, n, seed, k=300, shift=30):
    rng = np.random.default_rng(seed); w = rng.random(k) + 0.2
    return (rng.choice(k, n, p=w / w.sum()).astype(np.uint64) << np.uint64(shift)).astype(UINT[bits])


def three_vars(bits, seed, order=None):
    """Lookback delta on an int-mult chunk (three variables: the general kernel at 32 and 64 bits): quotients with a period of 37, remainders
    clustered like the W pages under a base near 2^44 (2^22 at 32 bits)."""
    n = 8192; rng = np.random.default_rng(seed)
    base, sep, ws, q_top = ((1 << 44) + 1, 40, WSEC64, 1 << 18) if bits == 64 else ((1 << 22) + 1, 18, WSEC32, 1 << 9)
    r = clusters(64, ws, 512, sep, seed + 1, order).astype(np.uint64)
    q = (rng.integers(0, q_top, 37)[np.arange(n) % 37] + rng.integers(0, 2, n)).astype(np.uint64)
    return (q * np.uint64(base) + r).astype(UINT[bits]), base


# ---------------------------------------------------------------------------------------------------------------- the rows
def _rows():
    rows = []
    def add(name, family, kw, make, route, compact, *claims):
        rows.append(Row(name, family, dict(kw), make, route, compact, tuple(claims)))

    # ---- W: field widths
    for bits, ws, sep in ((64, W64, 60), (32, W32, 28)):
        wide = "lean<2, wide>"
        cls = ["bmax_in=0..0", "bmax_in=1..16", "bmax_in=17..32", "bmax=16", "bmax=17", "one_width_per_batch"] + \
              (["bmax_in=33..63", "bmax=32", "bmax=33", "maxob>32,bmax<=16"] if bits == 64 else [])
        add(f"W-u{bits}-clusters", "W", CLASSIC, functools.partial(clusters, bits, ws, 512, sep, 7), wide, NONE, *cls)
        add(f"W-u{bits}-permuted", "W", CLASSIC, functools.partial(clusters, bits, ws, 512, sep, 7, 3), wide, NONE, "lanes_mix_widths", f"bmax={max(ws)}")
        add(f"W-u{bits}-outliers", "W", CLASSIC, functools.partial(outliers, bits, 5), wide, NONE, f"bmax={bits}", "bmax_in=0..0", "outliers_at_lanes_0_63",
            *(["bmax_in=64..64", "maxob>32,bmax<=16"] if bits == 64 else ["bmax=32"]))
        kw3 = dict(level=8, mode=4, mode_u64=three_vars(bits, 11)[1], delta=3)
        cls3 = ["vars=3", "sec:one_width_per_batch", "sec:bmax_in=0..0", "sec:bmax_in=1..16", "sec:bmax_in=17..32", "sec:bmax=16", "sec:bmax=17"] + \
               (["sec:bmax_in=33..63", "sec:bmax=32", "sec:bmax=33", "sec:maxob>32,bmax<=16"] if bits == 64 else [])
        add(f"W-u{bits}-three-clusters", "W", kw3, lambda bits=bits: three_vars(bits, 11)[0], "general", LB_ONLY if bits == 64 else LB_PRIMARY, *cls3)   # (the quotients' first period: differences of 18 bits at 64 bits, of 9 at 32)
        add(f"W-u{bits}-three-permuted", "W", kw3, lambda bits=bits: three_vars(bits, 11, 3)[0], "general", LB_ONLY if bits == 64 else LB_PRIMARY, "vars=3", "sec:lanes_mix_widths")
    # 16-bit latents: widths 0, 1 and 15 in one batch (16 cannot be: see UNREACHABLE)
    add("W-u16-lean2", "W", CLASSIC, functools.partial(narrow16, 16, 1), "lean<2>", PRIMARY, "widths_in_batch=0,1,15")
    add("W-u32-lean6", "W", dict(level=8, mode=4, mode_u64=40000, delta=1),
        lambda: (narrow16(32, 2).astype(np.uint64) * np.uint64(40000) + narrow16(32, 3).astype(np.uint64)).astype(np.uint32), "lean<6>", BOTH, "widths_in_batch=0,1,15", "sec:widths_in_batch=0,1,15")
    add("W-u32-lean3", "W", dict(level=8, mode=1, delta=3), functools.partial(lookback_steps, 5), "lean<3>", LB_PRIMARY, "widths_in_batch=0,1,15")
    # more than 256 bins: enc_page_kernel's BitSink
    add("W-u64-page", "W", dict(level=9, mode=1, delta=1), functools.partial(clusters, 64, WPAGE * 32, 16, 55, 9), "page", NONE,
        "put_end=32", "put_end=33", "put_end=64", "put_end=65", "bins>256")

    # ---- S: staging (the 16-bit lean rows first: in the Classic call they share enc_walkp_kernel's first block with rows that kernel refuses)
    for name, spec, claims in S_COMPACT:
        add(name, "S", S_COMPACT_KW[spec[0]], functools.partial(s_compact, *spec), spec[0], {"lean<2>": PRIMARY, "lean<6>": BOTH, "lean<3>": LB_PRIMARY}[spec[0]], *claims)
    for k in (43, 44):
        add(f"S-u64-ob{k}", "S", CLASSIC, functools.partial(uniform, 64, k, 1280, k), "lean<2, wide>", NONE, "reserve_passes<512" if k == 43 else "reserve_flushes<512", "flush_end=8")
    add("S-u64-ob44-511", "S", CLASSIC, functools.partial(uniform, 64, 44, 511, 45), "lean<2, wide>", NONE, "reach_decides")   # (8 + 256 x 44 + 255 x 44 + 96 = 22 588: 60 bits beyond)
    add("S-u64-full-after-narrow", "S", CLASSIC, lambda: np.concatenate([uniform(64, 8, 256, 1), uniform(64, 64, 256, 2)[::-1].copy() | np.uint64(256)]), "lean<2, wide>", NONE, "full64_after_pending")
    for name, seed, claims in S_SEARCHED:
        add(name, "S", CLASSIC, functools.partial(s_two_bins, *seed), s_route(seed), NONE, *claims)

    # ---- J: run joins
    for name, spec, claims in J_SEARCHED:
        add(name, "J", j_kw(spec), functools.partial(j_make, spec), spec[0], j_compact(spec[0]), "runs=6", *claims)

    # ---- T: tails
    for t in TAILS:
        n = 256 + t
        add(f"T-lean2-{t}", "T", CLASSIC, functools.partial(skewed, 32, n, 100 + t), "lean<2>", PRIMARY, f"tail={t}")
        add(f"T-wide32-{t}", "T", CLASSIC, functools.partial(two_far, 32, n, 200 + t, 1000, 1 << 24), "lean<2, wide>", NONE, f"tail={t}")
        add(f"T-wide64-{t}", "T", CLASSIC, functools.partial(two_far, 64, 512 + t, 300 + t, 1 << 20, 1 << 50), "lean<2, wide>", NONE, f"tail={t}")
        add(f"T-general-{t}", "T", CLASSIC, functools.partial(two_far, 16, n, 400 + t, 100, 40000), "general", NONE, f"tail={t}")
        add(f"T-copy-{t}", "T", CLASSIC, functools.partial(uniform, 32, 32, n, 500 + t), "copy", NONE, f"tail={t}")
        add(f"T-walkp-{t}", "T", CLASSIC, functools.partial(skewed, 16, n, 600 + t), "walkp", PRIMARY, f"tail={t}")
        add(f"T-lean6-{t}", "T", dict(level=8, mode=4, mode_u64=1000, delta=1), functools.partial(int_mult, 32, n, 700 + t, 1000), "lean<6>", BOTH, f"tail={t}", f"sec:tail={t}")
        add(f"T-lean3-{t}", "T", dict(level=8, mode=1, delta=3), functools.partial(periodic, 32, n + 1, 800 + t, 37, 3, 1 << 10), "lean<3>", LB_PRIMARY, f"tail={t}")
        add(f"T-page-{t}", "T", dict(level=9, mode=1, delta=1), functools.partial(many_spikes, 64, 8192 + t, 900 + t), "page", NONE, f"tail={t}", "bins>256")
    for order, n in ((1, 513), (7, 517)):
        add(f"T-lean6-order{order}", "T", dict(level=8, mode=4, mode_u64=1000, delta=2, delta_order=order),
            lambda n=n, order=order: (np.cumsum(int_mult(32, n, 50 + order, 1000, q_top=4).astype(np.uint64) // 1000 % 3) * 1000 + np.random.default_rng(order).integers(0, 3, n)).astype(np.uint32),
            "lean<6>", BOTH, "primary_one_batch_shorter")

    # ---- C: the shifted copy
    for bits in (16, 32, 64):
        per = 16 // (bits // 8)
        sizes = [2, 3, 4, 5, 64 * per - 1, 64 * per, 64 * per + 1, 256 * per - 1, 256 * per + 1, 16383, 16384, 16385, 16384 + 255, 32768 + 3]
        for n in sizes:
            # (a handful of numbers is cheaper as one bin per number than as one bin of full-width offsets: those rows are no copies)
            single = (bits == 16 and n <= 2) or (bits == 32 and n <= 3) or (bits == 64 and n <= 5)
            add(f"C-u{bits}-{n}", "C", CLASSIC, functools.partial(uniform, bits, bits, n, n + bits), ("general" if bits == 16 else "lean<2, wide>") if single else "copy", NONE,
                f"bins={n}" if single else f"copy_n={n}")
    for bits in (16, 32, 64):   # (one number: one bin without offset bits, nothing in the body; the general kernel writes the head)
        add(f"C-u{bits}-1", "C", CLASSIC, functools.partial(uniform, bits, bits, 1, 1), "general", PRIMARY, "writes_nothing")

    # ---- P: walk-and-pack, then place
    for name, spec, claims in P_SEARCHED:
        add(name, "P", CLASSIC, functools.partial(p_make, spec), "walkp" if spec[0] != "constant" else "general", PRIMARY, *claims)
    for i in range(3):
        add(f"P-u8-long-{i}", "P8", CLASSIC, functools.partial(skewed, 8, 32768, 40 + i, 1, 5 + 4 * i), "walkp", PRIMARY, "batches=128")

    # ---- H: the bin table of the head
    for bits, step, wide in ((64, 1 << 40, True), (8, 3, False)):
        for b in (63, 64, 65, 255, 256):
            if bits == 8 and b > 65: continue
            add(f"H-u{bits}-{b}", "H", CLASSIC, functools.partial(h_make, bits, b, step), "lean<2, wide>" if wide else "lean<2>", NONE if wide else PRIMARY, f"bins={b}")
    for b, rare in ((255, 128), (256, 64)):
        add(f"H-u8-{b}", "H", CLASSIC, functools.partial(h_make_u8, b, rare), "lean<2>", PRIMARY, f"bins={b}")
    return rows


def narrow16(bits, seed, n=16384, rare=24):
    """A few numbers over 16 401 values in batch 3 (too few for the partition to split their bin of 15 offset bits), a heavy pair (1 bit),
    two heavy single values: 16-bit latents (fewer than 32 768 values apart)."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(1, 4, n)
    a = np.where(pick == 1, 20000 + rng.integers(0, 2, n), np.where(pick == 2, 25000, 30000))
    at = 3 * 256 + rng.choice(256, rare, replace=False)
    a[at] = rng.integers(100, 16501, rare); a[at[:2]] = (100, 16500)
    return a.astype(UINT[bits])


def lookback_steps(seed, n=16384):
    """Steps drawn like narrow16 from the number before (the lookback search finds 1: every other candidate is further away), but for
    an exact copy of the number two back behind some of the long steps (it finds 2): a lookback variable of two bins, differences that are
    the steps."""
    rng = np.random.default_rng(seed)
    d = narrow16(32, seed + 1, n).astype(np.int64)
    d[d == 30000] = 25000                                # (differences of -5000 turn up too: all of them within 32 768 values)
    keep = np.arange(n) // 256 == 3                      # (the batch with the rare wide steps stays as narrow16 made it)
    d[(rng.random(n) < 0.4) & ~keep] = 0
    back = (rng.random(n) < 0.3) & ~keep
    a = np.zeros(n, np.int64); a[0] = 1 << 20; a[1] = a[0] + 25000
    for i in range(2, n):
        a[i] = a[i - 2] if back[i] and a[i - 1] - a[i - 2] >= 20000 else a[i - 1] + d[i]
    return a.astype(np.uint32)


def h_make(bits, b, step):
    """b values `step` apart, 32 (33 for every third) of each."""
    a = np.repeat(np.arange(b, dtype=np.uint64) * np.uint64(step), np.where(np.arange(b) % 3 == 0, 33, 32))
    np.random.default_rng(b).shuffle(a)
    return a.astype(UINT[bits])


def h_make_u8(b, rare):
    """Every value below b of a byte, 384 and `rare` of them by turns: bins the partition does not merge once there are enough numbers."""
    a = np.repeat(np.arange(b).astype(np.uint8), np.where(np.arange(b) % 2 == 0, 384, rare))
    np.random.default_rng(b).shuffle(a)
    return a


# S rows found by a search over widths, lengths and seeds, recorded here: two clusters `far` apart at widths (k0, k1), n numbers, seed
def s_two_bins(bits, k0, k1, n, seed):
    rng = np.random.default_rng(seed)
    far = 40000 if bits == 16 else 1 << (bits - 2)   # (beyond the 16-bit window either way)
    pick = rng.random(n) < 0.7
    a = np.where(pick, rng.integers(0, 1 << k0, n, dtype=np.uint64), np.uint64(far) + rng.integers(0, 1 << k1, n, dtype=np.uint64))
    a[0] = 0; a[1] = (1 << k0) - 1; a[2] = far; a[3] = far + (1 << k1) - 1
    return a.astype(UINT[bits])


def s_compact(rt, k0, k1, n, seed):
    """The staging rows of the lean kernels over 16-bit latents (values fewer than 4096 apart): two clusters of k0 and k1 offset bits for
    `lean<2>`; quotient and remainder of that kind under the base 4096 for `lean<6>`; a period of 37 with 2^k0 values of noise under a
    lookback delta for `lean<3>`."""
    def two(seed):
        rng = np.random.default_rng(seed)
        a = np.where(rng.random(n) < 0.7, rng.integers(0, 1 << k0, n), 2048 + rng.integers(0, 1 << k1, n))
        a[:4] = (0, (1 << k0) - 1, 2048, 2048 + (1 << k1) - 1)
        return a.astype(np.uint64)
    if rt == "lean<2>": return two(seed).astype(np.uint32)
    if rt == "lean<6>": return (two(seed) * np.uint64(4096) + two(seed + 500)).astype(np.uint32)
    return periodic(32, n, seed, 37, 1 << k0, 1 << 9)


S_COMPACT_KW = {"lean<2>": CLASSIC, "lean<6>": dict(level=8, mode=4, mode_u64=4096, delta=1), "lean<3>": dict(level=8, mode=1, delta=3)}
# (route, k0, k1, n, seed), found by a search over widths, lengths and seeds
S_COMPACT = [
    ("S-lean2-10-9-4096a", ("lean<2>", 10, 9, 4096, 5), ["flush_end=0"]), ("S-lean2-10-9-4096b", ("lean<2>", 10, 9, 4096, 7), ["flush_end=31"]),
    ("S-lean2-10-9-5120", ("lean<2>", 10, 9, 5120, 6), ["flush_end=1"]), ("S-lean2-10-6-4096a", ("lean<2>", 10, 6, 4096, 0), ["reserve_flushes<512"]),
    ("S-lean2-10-6-4096b", ("lean<2>", 10, 6, 4096, 2), ["reserve_passes<512"]),
    ("S-lean6-10-9-4096a", ("lean<6>", 10, 9, 4096, 0), ["flush_end=0"]), ("S-lean6-10-9-4096b", ("lean<6>", 10, 9, 4096, 1), ["reserve_passes<512"]),
    ("S-lean6-10-9-5120", ("lean<6>", 10, 9, 5120, 0), ["flush_end=1"]), ("S-lean6-10-9-6144", ("lean<6>", 10, 9, 6144, 1), ["flush_end=31"]),
    ("S-lean6-10-6-4096", ("lean<6>", 10, 6, 4096, 0), ["reserve_flushes<512"]),
    ("S-lean3-10-4096a", ("lean<3>", 10, 0, 4096, 2), ["flush_end=0"]), ("S-lean3-10-4096b", ("lean<3>", 10, 0, 4096, 5), ["reserve_passes<512"]),
    ("S-lean3-10-5120a", ("lean<3>", 10, 0, 5120, 0), ["flush_end=31"]), ("S-lean3-10-5120b", ("lean<3>", 10, 0, 5120, 3), ["flush_end=1"]),
    ("S-lean3-9-4096", ("lean<3>", 9, 0, 4096, 4), ["reserve_flushes<512"]),
]


def s_route(spec):
    return "general" if spec[0] == 16 else "lean<2, wide>"


S_SEARCHED = [
    ("S-u64-two-23-19-1536", (64, 23, 19, 1536, 4), ["flush_end=1"]),
    ("S-u64-two-23-19-2048", (64, 23, 19, 2048, 4), ["flush_end=0"]),
    ("S-u64-two-37-19-1536", (64, 37, 19, 1536, 3), ["flush_end=31", "field_ends=14,19,45,30"]),
    ("S-u16-two-7-9-2048", (16, 7, 9, 2048, 2), ["reserve_passes<512"]),
    ("S-u16-two-7-9-2304", (16, 7, 9, 2304, 2), ["flush_end=1"]),
    ("S-u16-two-11-5-2048", (16, 11, 5, 2048, 5), ["flush_end=31", "reserve_flushes<512"]),
    ("S-u16-two-11-9-2304", (16, 11, 9, 2304, 1), ["flush_end=0"]),
]
# (route, n, seed, outliers per end)
_J_ONE = [((0, 30), ["run_in_dword", "two_starts_in_dword"]), ((1, 30), ["run_residue=0"]), ((1, 29), ["run_residue=1"]), ((3, 29), ["run_residue=31"])]
J_SEARCHED = [(f"J-{rt}-{seed}-{k}", (rt, 98304, seed, k), claims) for rt in ("lean<2>", "lean<2, wide>", "general") for (seed, k), claims in _J_ONE] + \
             [(f"J-{rt}-partial", (rt, 5 * 16384 + 77, 1, 30), ["last_run_one_partial_batch"]) for rt in ("lean<2>", "lean<2, wide>", "general", "lean<6>", "lean<3>")] + [
    ("J-lean<6>-0-30", ("lean<6>", 98304, 0, 30), ["run_residue=1"]), ("J-lean<6>-3-30", ("lean<6>", 98304, 3, 30), ["run_residue=0"]),
    ("J-lean<6>-7-30", ("lean<6>", 98304, 7, 30), ["run_residue=31"]),
    ("J-lean<3>-0-30", ("lean<3>", 98304, 0, 30), ["run_residue=1"]), ("J-lean<3>-3-30", ("lean<3>", 98304, 3, 30), ["run_residue=0"]),
    ("J-lean<3>-5-30", ("lean<3>", 98304, 5, 30), ["run_residue=31"]),
]
# (kind, bits, n, seed, top): the first rows by search, the rest fill the call to 40 pages of 1, 2, 3 and 5 batches and partial last batches; items
# 2 k and 2 k + 1 share a packing wave of enc_walkp_kernel: a long page beside a short one in both orders, a constant page among them
P_SEARCHED = [
    ("P-head24", ("skew", 16, 257, 0, 3), ["head_end=24"]), ("P-body0", ("skew", 16, 257, 0, 16), ["body%32=0", "scratch_first=0"]),
    ("P-body1", ("skew", 16, 257, 1, 16), ["body%32=1", "head_end=16", "scratch_first=31"]), ("P-body31", ("skew", 16, 257, 3, 5), ["body%32=31"]),
    ("P-head8", ("skew", 16, 300, 0, 5), ["head_end=8"]), ("P-head0", ("skew", 16, 1280, 0, 5), ["head_end=0", "batches=5"]),
    ("P-tiny-one-dword", ("rare", 16, 257, 0, 4), ["body<32_one_dword"]), ("P-long-a", ("skew", 32, 1281, 7, 9), ["batches=6"]),
    ("P-tiny-two-dwords", ("rare", 16, 257, 3, 2), ["body<32_two_dwords"]), ("P-constant", ("constant", 16, 700, 0, 0), ["writes_nothing"]),
    ("P-long-b", ("skew", 64, 1300, 9, 16), ["batches=6"]), ("P-short-b", ("skew", 8, 256, 8, 5), ["batches=1"]),
] + [(f"P-fill-{i}", ("skew", (16, 32, 8, 64)[i % 4], (256, 1280, 300, 512, 768, 700, 513, 769, 257, 1279)[i % 10], 20 + i, (5, 9, 16, 3)[i % 4]),
      [f"batches={((256, 1280, 300, 512, 768, 700, 513, 769, 257, 1279)[i % 10] + 255) // 256}"]) for i in range(28)]


def j_kw(spec):
    return {"lean<2>": CLASSIC, "lean<2, wide>": CLASSIC, "general": CLASSIC, "lean<6>": dict(level=8, mode=4, mode_u64=1000, delta=1),
            "lean<3>": dict(level=8, mode=1, delta=3)}[spec[0]]


def j_compact(rt):
    return {"lean<2>": PRIMARY, "lean<2, wide>": NONE, "general": NONE, "lean<6>": BOTH, "lean<3>": LB_PRIMARY}[rt]


def j_make(spec):
    """(route, n, seed, k): the six-run page of a route."""
    rt, n, seed, k = spec
    if rt == "lean<2>": return spikes(32, n, seed, k=k)
    if rt == "lean<2, wide>": return spikes(64, n, seed, out=1 << 40, k=k)
    if rt == "general": return spikes(16, n, seed, out=40000, k=k)
    if rt == "lean<6>": return (spikes(32, n, seed, k=k).astype(np.uint64) * np.uint64(1000) + spikes(32, n, seed + 1000, base=0, out=3, k=k)).astype(np.uint32)
    a = np.random.default_rng(9).integers(0, 1 << 12, 37)[np.arange(n) % 37].astype(np.uint32)   # lean<3>: a period, a few numbers off it
    rng = np.random.default_rng(seed)
    a[rng.choice(16384, k, replace=False)] += 1
    a[n - 1 - rng.choice(16384, k, replace=False)] += 1
    return a


def p_make(spec):
    """(kind, bits, n, seed, top)"""
    kind, bits, n, seed, top = spec
    if kind == "constant": return np.full(n, 123, UINT[bits])
    if kind == "rare": return np.where(np.random.default_rng(seed).random(n) < top / 1000.0, 6, 5).astype(UINT[bits])
    return skewed(bits, n, seed, 1, top)


@functools.lru_cache(maxsize=None)
def ROWS():
    rows = _rows()
    assert len({r.name for r in rows}) == len(rows)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def BY_NAME():
    return {r.name: r for r in ROWS()}


@functools.lru_cache(maxsize=None)
def numbers(name):
    a = np.ascontiguousarray(BY_NAME()[name].make())
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_file(name):
    return O.simple_compress(numbers(name), O.make_config(**BY_NAME()[name].kw))


@functools.lru_cache(maxsize=None)
def oracle_chunk(name):
    """The standalone chunk the oracle writes for the row."""
    a = numbers(name)
    f = oracle_file(name)
    header = 4 + 1 + 1 + (6 + max(int(a.size).bit_length(), 1) + 7) // 8 + 2   # magic, version, uniform type byte, the varint n_hint, the wrapped format's two bytes
    return f[header:-1]                                                          # ... and the terminator behind the chunk


@functools.lru_cache(maxsize=None)
def layout(name):
    return P.parse_chunk(oracle_chunk(name))


# ---------------------------------------------------------------------------------------------------------------- conditions
def holds(row, cond, variants=()):
    """Whether `cond` holds of the row's page, by the model on the oracle's chunk.  A "sec:" prefix speaks of the secondary, else the primary.
    `variants`: the wrong restatements of pack_layout_model.VARIANTS to evaluate it under."""
    L = layout(row.name)
    v = 1
    if cond.startswith("sec:"): v, cond = 2, cond[4:]
    key, _, val = cond.partition("=")
    per_batch = [row_[v].widths for row_ in L.batches if v in row_]
    bmaxes = [max(w, default=0) for w in per_batch]
    body = L.body_last - L.body_first
    if key == "bmax": return int(val) in bmaxes
    if key == "bmax_in":
        a, b = (int(x) for x in val.split("..")); return any(a <= m <= b for m in bmaxes)
    if cond == "maxob>32,bmax<=16": return P.max_ob(L, v) > 32 and any(m <= 16 for m in bmaxes)
    if cond == "one_width_per_batch": return all(len(set(w)) == 1 for w in per_batch)
    if cond == "lanes_mix_widths": return any(len(set(w[i:i + 4])) > 1 for w in per_batch for i in range(0, len(w), 4))
    if cond == "outliers_at_lanes_0_63":
        return any(len(w) == 256 and set(w[:4]) | set(w[252:]) == {L.latent_bits} and max(w[4:252]) <= 16 for w in per_batch)
    if cond == "vars=3": return all(L.present[u] and not P.trivial(L, u) for u in range(3))
    if key == "widths_in_batch": return any({int(x) for x in val.split(",")} <= set(w) for w in per_batch)
    if key == "field_ends":   # how many offset fields end 32, 33, 64 and 65 bits past the start of their first dword (put's second and third dword)
        ends = collections.Counter((pos & 31) + w for pos, w in P.fields(L, variants))
        return [ends[k] for k in (32, 33, 64, 65)] == [int(x) for x in val.split(",")]
    if key == "put_end": return any((pos & 31) + w == int(val) for pos, w in P.fields(L, variants))
    if cond == "bins>256": return len(L.bins[1]) > 256
    if key == "bins": return len(L.bins[1]) == int(val)
    if key == "tail": return len(per_batch) >= 2 and len(per_batch[-1]) == int(val) and len(per_batch[-2]) == 256
    if cond == "primary_one_batch_shorter": return sum(1 in r for r in L.batches) + 1 == sum(2 in r for r in L.batches)
    if key == "copy_n": return L.n == int(val) and len(L.bins[1]) == 1 and L.bins[1][0][2] == L.latent_bits
    if cond == "writes_nothing": return body == 0
    if key == "batches": return len(L.batches) == int(val)
    # the stages of the page's runs
    if cond in ("reserve_passes<512", "reserve_flushes<512", "full64_after_pending", "reach_decides") or key == "flush_end":
        for _, flushes, dist, pends, tags in P.run_schedules(L, row.route, variants):
            if cond == "reserve_passes<512" and any(0 <= d < 512 for d in dist): return True
            if cond == "reserve_flushes<512" and any(-512 <= d < 0 for d in dist): return True
            if cond == "reach_decides" and any(-P.kPutReach <= d < 0 for d in dist): return True   # (a reserve that flushes only for the reach of a put)
            if key == "flush_end" and any(f % 32 == int(val) for f in flushes): return True
            if cond == "full64_after_pending" and any(t != "head" and p > 0 and L.batches[t[1]][t[0]].widths == [64] * 256 for t, p in zip(tags, pends)): return True
        return False
    # run joins
    st, en = P.runs(L, variants), P.run_ends(L, variants)
    if key == "runs": return len(st) == int(val)
    if key == "run_residue": return any(s % 32 == int(val) for s in st[1:])
    if cond == "run_in_dword": return any(e > s and s >> 5 == (e - 1) >> 5 and 0 < k < len(st) - 1 for k, (s, e) in enumerate(zip(st, en)))
    if cond == "two_starts_in_dword": return len({s >> 5 for s in st}) < len(st)
    if cond == "last_run_one_partial_batch": return len(L.batches) % (32 if "runs32" in variants else P.kRunBatches) == 1 and L.n % 256 != 0
    # walk-and-pack, then place
    if key == "body%32": return body % 32 == int(val)
    if cond == "body<32_one_dword": return 0 < body < 32 and L.head_bits >> 5 == (L.head_bits + body - 1) >> 5
    if cond == "body<32_two_dwords": return 0 < body < 32 and L.head_bits >> 5 != (L.head_bits + body - 1) >> 5
    if key == "head_end": return L.head_bits % 32 == int(val)
    if key == "scratch_first": return (reg_bits_of(L.n_lat[1]) - body) % 32 == int(val)
    raise KeyError(cond)


def reg_bits_of(n_lat):
    """enc_walkp_kernel: the bits of a page's body region in the field scratch; the body is written downwards from its end."""
    return ((2 * n_lat + 8) & ~3) * 8 if n_lat else 0


W_WIDE64 = ["bmax_in=0..0", "bmax_in=1..16", "bmax_in=17..32", "bmax_in=33..63", "bmax_in=64..64", "bmax=16", "bmax=17", "bmax=32", "bmax=33", "maxob>32,bmax<=16",
            "one_width_per_batch", "lanes_mix_widths", "outliers_at_lanes_0_63"]
W_WIDE32 = ["bmax_in=0..0", "bmax_in=1..16", "bmax_in=17..32", "bmax=16", "bmax=17", "bmax=32", "one_width_per_batch", "lanes_mix_widths", "outliers_at_lanes_0_63"]
J_ALL = ["runs=6", "run_residue=0", "run_residue=1", "run_residue=31", "run_in_dword", "two_starts_in_dword", "last_run_one_partial_batch"]
S_ALL = ["reserve_passes<512", "reserve_flushes<512", "flush_end=0", "flush_end=1", "flush_end=31", "full64_after_pending"]
LEAN16 = ("lean<2>", "lean<6>", "lean<3>")          # the lean kernels over 16-bit latents
LEAN_TWO = ("lean<6>", "lean<3>")                   # ... with two variables
# (family, routes, latent bits or None for any) -> what the rows of that family on those routes must show between them
REQUIRED = {
    ("W", ("lean<2, wide>",), 64): W_WIDE64, ("W", ("lean<2, wide>",), 32): W_WIDE32,
    ("W", ("general",), 64): ["vars=3"] + ["sec:" + c for c in W_WIDE64], ("W", ("general",), 32): ["vars=3"] + ["sec:" + c for c in W_WIDE32],
    ("W", ("page",), None): ["put_end=32", "put_end=33", "put_end=64", "put_end=65", "bins>256"],
    ("W", LEAN16, None): ["widths_in_batch=0,1,15,16"],
    ("S", ("lean<2, wide>",), None): S_ALL + ["reach_decides", "field_ends=14,19,45,30"], ("S", ("general",), None): S_ALL,
    ("S", ("lean<2>",), None): S_ALL, ("S", ("lean<6>",), None): S_ALL, ("S", ("lean<3>",), None): S_ALL,
    ("J", LEAN_TWO, None): ["run_in_dword", "two_starts_in_dword"],
    ("P", ("walkp",), None): ["body%32=0", "body%32=1", "body%32=31", "body<32_one_dword", "body<32_two_dwords", "head_end=0", "head_end=8", "head_end=16", "head_end=24",
                              "scratch_first=0", "scratch_first=31", "batches=1", "batches=2", "batches=3", "batches=5"],
    ("P", ("general",), None): ["writes_nothing"],
    ("H", ("lean<2, wide>",), None): [f"bins={b}" for b in (63, 64, 65, 255, 256)], ("H", ("lean<2>",), None): [f"bins={b}" for b in (63, 64, 65, 255, 256)],
}
for _rt in LEAN16:
    REQUIRED[("W", (_rt,), None)] = ["widths_in_batch=0,1,15"]
for _rt in ("lean<2>", "lean<2, wide>", "general", "lean<6>", "lean<3>"):
    REQUIRED[("J", (_rt,), None)] = [c for c in J_ALL if _rt not in LEAN_TWO or c not in ("run_in_dword", "two_starts_in_dword")]
for _rt in ("lean<2>", "lean<2, wide>", "general", "copy", "walkp", "lean<6>", "lean<3>", "page"):
    REQUIRED[("T", (_rt,), None)] = [f"tail={t}" for t in TAILS] + (["primary_one_batch_shorter"] if _rt == "lean<6>" else [])
for _bits in (16, 32, 64):
    _per = 16 // (_bits // 8)
    REQUIRED[("C", ("copy",), _bits)] = [f"copy_n={n}" for n in (64 * _per - 1, 64 * _per, 64 * _per + 1, 256 * _per - 1, 256 * _per + 1, 16383, 16384, 16385, 16384 + 255, 32768 + 3)]

# conditions no input can meet: (family, routes, bits, condition) -> why.  At most three.
UNREACHABLE = {
    ("W", LEAN16, None, "widths_in_batch=0,1,15,16"): "the lean kernels without `wide` pack 16-bit latents only, and those span fewer than 2^15 values (kC16KeyRange, kWideHistRange): no bin of such a variable has more than 15 offset bits",
    ("J", LEAN_TWO, None, "run_in_dword"): "two variables that write anything each cost a run of 64 batches 22 bits or more (16 384 symbols of a 2^10 table's heaviest weight, 1023): a middle run is 44 bits or longer",
    ("J", LEAN_TWO, None, "two_starts_in_dword"): "as run_in_dword: runs of 44 bits or more put at most one start into a dword",
}
assert len(UNREACHABLE) <= 3

# Conditions that ask for an offset as wide as a 32- or 64-bit type on a route whose variables are narrower ("where the width allows"): carried
# here, one by one and with the reason, so that the coverage test counts them.  (family, routes, bits, condition) -> why
_SEC_BASE = "the three-variable page is the one the general kernel packs at 32 and 64 bits, and its remainders lie under the int-mult base (2^44 + 1, 2^22 + 1): no bin of the secondary is as wide as the type, so neither is a heavy constant's outlier bin (the quotients stay below 2^20 resp. 2^10, and so do their differences under the lookback delta)"
_LATENT16 = "16-bit latents: no offset of such a variable has more than 15 bits, and a batch of 256 x 64 offset bits needs a 64-bit variable"
WIDTH_LIMITED = {
    ("W", ("general",), 64, "sec:bmax_in=64..64"): _SEC_BASE, ("W", ("general",), 64, "sec:outliers_at_lanes_0_63"): _SEC_BASE,
    ("W", ("general",), 32, "sec:bmax=32"): _SEC_BASE, ("W", ("general",), 32, "sec:outliers_at_lanes_0_63"): _SEC_BASE,
    ("S", ("general",), None, "full64_after_pending"): "one- and two-variable pages reach the general kernel only with full-width latents of an 8- or 16-bit type: no 64-bit offsets",
    ("S", ("lean<2>",), None, "full64_after_pending"): _LATENT16, ("S", ("lean<6>",), None, "full64_after_pending"): _LATENT16,
    ("S", ("lean<3>",), None, "full64_after_pending"): _LATENT16,
}


def coverage(family, routes, bits):
    """The conditions claimed by the rows of (family, routes[, latent bits])."""
    return {c for r in ROWS() if r.family == family and r.route in routes and (bits is None or layout(r.name).latent_bits == bits) for c in r.claims}


# ---------------------------------------------------------------------------------------------------------------- calls
Call = collections.namedtuple("Call", "name kw rows shifts")


@functools.lru_cache(maxsize=None)
def CALLS():
    """The batched calls of the device suite: the rows of a family that share a config, those meant for enc_walkp_kernel in a call of their
    own (a block of that kernel qualifies only as a whole).  shifts: the destination offsets modulo 16 the call is run at."""
    groups = collections.OrderedDict()
    for r in ROWS():
        if r.family == "P8": continue
        key = (r.family + ("-walkp" if r.route == "walkp" and r.family != "P" else ""), tuple(sorted(r.kw.items())))
        groups.setdefault(key, []).append(r.name)
    out = []
    for (fam, kw), names in groups.items():
        tag = "-".join(f"{k}{v}" for k, v in kw if (k, v) not in (("mode", 1), ("delta", 1), ("level", 8)))
        out.append(Call(fam + ("-" + tag if tag else ""), dict(kw), tuple(names), (0, 8) if fam[0] in "JTC" else (8,) if fam[0] == "P" else (0,)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def predicted_routes(call):
    """The model's route for every row of a call: {row name: route}."""
    Ls = [layout(n) for n in call.rows]; cs = [BY_NAME()[n].compact for n in call.rows]
    walkp = P.call_walkp(Ls, cs, P.call_slots([call.kw]))
    return {n: P.route(l, c, w) for n, l, c, w in zip(call.rows, Ls, cs, walkp)}
