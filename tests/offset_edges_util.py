"""The rows of the offset-reader suites (test_offset_reader_model.py on the CPU, test_gpu_offset_edges.py on the device): valid chunks from
the TEST-ONLY generator (oracle/pco_oracle_testenc.hpp) in which every bin of the forced variable carries exactly k offset bits
(TBL_OB_ALL) with the lowers moved down (tbl_lower_wrap), on few-valued data -- so the trained bins need fewer bits than k, the section of
every batch fills the dwords its reader reserves, and the fields are populated up to their top bit.

rows(width) -> [(label, array, test_encode kwargs)]; built(width) adds the file, the chunk inside it, its pack_layout_model.Layout and the
row's group.  Seeds come from deterministic searches from fixed starts (the first seed whose layout has the wanted residue / nd / byte
position), cached per process: what a row covers is certified by the layout model in coverage(), not by luck, and missing(width, ...) lists
what a set of rows fails to cover -- the CPU suite asserts it is empty, and that it is not once a group of rows is taken away.

Groups: "res" (k x every start residue of a full batch), "last" (k x last batches of 1 .. 256 latents, batches of delta state only), "nd"
(the one / two / three register seams of trail_section), "bins" (2, 63, 64 bins; 65 is a refusal), "one16" (TBL_OB_ONE: a section far
shorter than its reserve), "two" (two latent variables on either side of kFlFast2 / kFlTriv2), "wide" (k beyond 16: dec_expand_kernel's
per-field path; k = 17 is the expanders' refusal where the latent has 17 bits), "2048" (need_bytes 2048 / 2052 / beyond), "lb" (Lookback:
dec_expand_lb_kernel), "tail" (the safe-load tail), "general" (257 bins: pco_decode_kernel)."""
import collections
import functools

import numpy as np

import gpu_util as U
import offset_reader_model as M
import oracle_lib as O
import pack_layout_model as P

WIDTHS = (8, 16, 32, 64)
UINT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
SINT = {8: np.int8, 16: np.int16, 32: np.int32, 64: np.int64}
K_TRAIL = (1, 7, 8, 15, 16)
K_WIDE = (17, 31, 32, 33, 57, 63, 64)
K_GENERAL = (1, 8, 32, 57, 58, 59, 60, 61, 62, 63, 64)
LAST_BATCHES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256)
ND_SEAMS = {8: (64, 65), 16: (64, 65, 128, 129)}     # k -> the nd a last batch must take
WINDOW_ENDS = {8: (63,), 16: (64, 128)}               # ... and where some lane's window must end in those rows: its last dword is the last of the
                                                      # first register (k = 8), the first of the second (k = 16) and the first of the third.  (With
                                                      # every field 16 bits wide a lane's window starts on an even dword and ends on one: no row of
                                                      # this generator has a window that ends at dword 127.)
GROUPS = ("res", "last", "nd", "bins", "one16", "two", "wide", "2048", "lb", "tail", "general")

# the decoders' selection, as far as these rows need it (decode_fast.hip; test_offset_reader_model.py reads the numbers from the sources)
kFastMaxBins, kFastMaxAns, kTrailMaxBins, kTrailMaxOb = 256, 12, 64, 16
K8_TABLE_BYTES, K4_TABLE_BYTES = 4272, 9264
kTrailMinChunks = 1024    # pco_gfx.hip: a width group of at least this many chunks decodes with the expanders under the walk

Row = collections.namedtuple("Row", "label array kw")
Built = collections.namedtuple("Built", "row group file chunk layout")
CLASSIC = dict(mode=O.MODE_CLASSIC)
TWO_VAR = {8: [("imult", np.uint8, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=5))],
           16: [("imult", np.int16, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=7)), ("fmult", np.float16, dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.5)),
                ("fquant", np.float16, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=4))],
           32: [("imult", np.int32, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=7)), ("fmult", np.float32, dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.25)),
                ("fquant", np.float32, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=12))],
           64: [("imult", np.int64, dict(mode=O.MODE_TRY_INT_MULT, mode_u64=1000)), ("fmult", np.float64, dict(mode=O.MODE_TRY_FLOAT_MULT, mode_f64=0.01)),
                ("fquant", np.float64, dict(mode=O.MODE_TRY_FLOAT_QUANT, mode_u64=30))]}


def ks(width, pool):
    return tuple(k for k in pool if k <= width)


# ---------------------------------------------------------------------------------------------------------------- data
def few(dt, n, seed, order=0, m=4):
    """n numbers of m far-apart values with unequal counts, summed `order` times (wrapping): under a consecutive delta of that order the
    latents are the m values again, one trained bin each, none needing an offset bit."""
    rng = np.random.default_rng(seed); dt = np.dtype(dt); bits = 8 * dt.itemsize
    vals = (np.arange(m, dtype=np.uint64) * np.uint64((((1 << bits) - 1) // (m + 1)) | 1)).astype(UINT[bits])
    p = rng.random(m) ** 2 + 0.05
    x = vals[rng.choice(m, n, p=p / p.sum())]
    for _ in range(order): x = np.cumsum(x, dtype=UINT[bits])
    return np.ascontiguousarray(x.view(dt))


def two_data(kind, dt, kw, n, seed, order, sec):
    """Two latent variables: a few-valued primary (summed `order` times) beside a secondary that is constant (sec 0) or takes sec values."""
    rng = np.random.default_rng(seed); dt = np.dtype(dt); bits = 8 * dt.itemsize
    q = rng.choice(np.array([1, 2, 4, 7, 11]), n, p=[0.4, 0.25, 0.2, 0.1, 0.05])
    for _ in range(order): q = np.cumsum(q) % (40 if bits == 8 else 3000)
    r = rng.integers(0, sec, n) if sec else np.zeros(n, np.int64)
    if kind == "imult":
        return np.ascontiguousarray((q * kw["mode_u64"] + r).astype(dt))
    u = UINT[bits]
    if kind == "fmult":
        x = ((q + 16) * kw["mode_f64"]).astype(dt)
        return np.ascontiguousarray((x.view(u) + r.astype(u)).view(dt))
    sh = kw["mode_u64"]
    one = np.ones(1, dt).view(u)[0]           # float-quant: the primary is the bits above the low `sh`; q counted up from 1.0's
    return np.ascontiguousarray((one + (q.astype(u) << u(sh)) + r.astype(u)).view(dt))


def forced(k, vars_=O.TBL_PRIMARY, seed=1, **more):
    return dict(tbl_vars=vars_, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=k, tbl_lower_wrap=True, tbl_seed=seed, **more)


def consecutive(order):
    return dict(delta=O.TE_DELTA_CONSECUTIVE, order=order) if order else {}


# ---------------------------------------------------------------------------------------------------------------- building a row
def build(row, group):
    f = O.test_encode(row.array, **row.kw)
    chunk = f[U.standalone_header_len(row.array.size):-1]
    return Built(row, group, f, chunk, P.parse_chunk(chunk))


def exact(b, v, k):
    """Every bin of variable v carries exactly k offset bits."""
    return len(b.layout.bins[v]) > 0 and all(x[2] == k for x in b.layout.bins[v])


def starts(layout, v, full_only=False):
    """[(batch, first bit of the offset section, latents)] of variable v."""
    out = []
    for bi, r in enumerate(layout.batches):
        if v in r and (not full_only or len(r[v].widths) == 256):
            out.append((bi, r[v].pos + r[v].ans_bits, len(r[v].widths)))
    return out


def populated(b):
    """At least half of the chunk's non-empty fields have their top bit set (a condition on every row: a cut one bit short cannot pass).
    The lookback variable's lowers cannot be moved down, so its wide fields hold small numbers: the "lb" rows are the exception."""
    return b.group == "lb" or M.top_bit_share(b.chunk, b.layout) >= 0.5


def search(make, accept, start, limit=400):
    """The first seed from `start` whose built row `accept`s (deterministic: the generator, numpy's generators and the search order are)."""
    for seed in range(start, start + limit):
        b = make(seed)
        if b is not None and accept(b) and populated(b): return b
    raise AssertionError(f"no seed in [{start}, {start + limit}) gives the wanted row")


def classic_row(width, group, label, k, n, seed, order=0, m=4, signed=False, **tbl):
    dt = (SINT if signed else UINT)[width]
    kw = dict(CLASSIC, **consecutive(order), **forced(k, seed=seed % 7 + 1, **tbl))
    return build(Row(f"{label} k={k} n={n} order={order} seed={seed}", few(dt, n, seed, order, m), kw), group)


# ---------------------------------------------------------------------------------------------------------------- the groups
def g_res(width):
    """Per k: rows of seven full batches, kept while they add a start residue, until every residue 0..31 starts a full batch."""
    out = []
    for k in ks(width, K_TRAIL):
        seen = set()
        for seed in range(1000, 1400):
            b = classic_row(width, "res", "res", k, 7 * 256 + 1 + seed * 37 % 200, seed, order=seed % 3, m=3 + seed % 4, signed=seed % 2 == 1)
            if not exact(b, 1, k) or not populated(b): continue
            new = {s & 31 for _, s, _ in starts(b.layout, 1, True)} - seen
            if new: out.append(b); seen |= new
            if len(seen) == 32: break
        assert len(seen) == 32, (width, k, sorted(seen))
    return out


def g_last(width):
    """Per k: last batches of 1 .. 256 latents behind one full batch, orders 0..2 in turn; a chunk of 70 numbers (it ends before its wave's
    other chunk has begun its second batch); under orders 1 and 2 a last batch that holds only delta state (numbers, but no latent)."""
    out = []
    for k in ks(width, K_TRAIL):
        for i, last in enumerate(LAST_BATCHES):
            order = (i + k) % 3
            out.append(search(lambda s: classic_row(width, "last", f"last={last}", k, 256 + last + order, s, order, signed=i % 2 == 1),
                              lambda b: exact(b, 1, k) and starts(b.layout, 1)[-1][2] == last, 2000 + 10 * i))
        out.append(search(lambda s: classic_row(width, "last", "short", k, 70, s, order=k % 3), lambda b: exact(b, 1, k) and len(b.layout.bins[1]) > 1, 2100))
        for order in (1, 2):
            for extra in range(1, order + 1):
                out.append(search(lambda s: classic_row(width, "last", f"state-only+{extra}", k, 512 + extra, s, order),
                                  lambda b: exact(b, 1, k) and b.layout.batches[-1] == {} and len(b.layout.batches) == 3, 2200))
    return out


def g_nd(width):
    """Last batches whose section takes exactly 64 / 65 (one register | two) and 128 / 129 (two | three) dwords with the reach."""
    out = []
    for k, seams in ND_SEAMS.items():
        if k > width: continue
        for nd in seams:
            cnts = {(8, 64): (244, 247, 248), (8, 65): (247, 248), (16, 64): (122, 123, 124), (16, 65): (123, 124, 125), (16, 128): (250, 251), (16, 129): (253,)}[(k, nd)]
            def accept(b):
                _, s, cnt = starts(b.layout, 1)[-1]
                return exact(b, 1, k) and M.trail_nd(s, cnt, k) == nd
            out.append(search(lambda s: classic_row(width, "nd", f"nd={nd}", k, 256 + cnts[s % len(cnts)], s, m=3 + s % 3), accept, 3000))
    return out


def g_bins(width):
    """2, 63 and 64 bins (lane 63 holds a bin); 65 bins: the expanders refuse the chunk."""
    out = []
    for k in ks(width, (7, 16)):
        out.append(search(lambda s: classic_row(width, "bins", "bins=2", k, 700, s, m=2), lambda b: exact(b, 1, k) and len(b.layout.bins[1]) == 2, 4000))
        for nb in (63, 64, 65):
            out.append(search(lambda s: classic_row(width, "bins", f"bins={nb}", k, 900, s, order=s % 2, m=5, tbl_n_bins=nb, tbl_ans_size_log=O.TBL_ANS_MIN),
                              lambda b: exact(b, 1, k) and len(b.layout.bins[1]) == nb, 4100))
    return out


def clamp_run(b):
    """Dwords the fetch of the chunk's last batch asks for beyond the clamp (each of them reads the dword at the clamp instead)."""
    bi, s, cnt = starts(b.layout, 1)[-1]
    return (s >> 5) + M.trail_nd(s, cnt, P.max_ob(b.layout, 1)) - ((len(b.chunk) + M.kTrailClamp) >> 2)


def g_one16(width):
    """ONE bin at min(16, width) bits, the others tight: max_ob says 16 where almost no field has a bit, so the fetch of every batch runs
    far past the section, and in the last batches past the chunk's end into the clamp."""
    k = min(16, width)
    def make(s):
        kw = dict(CLASSIC, tbl_vars=O.TBL_PRIMARY, tbl_ob_mode=O.TBL_OB_ONE, tbl_ob_value=k, tbl_lower_wrap=True, tbl_seed=s)
        return build(Row(f"one bin at {k} seed={s}", few(UINT[width], 4 * 256 + 255, s, m=5), kw), "one16")
    def accept(b):
        obs = sorted(x[2] for x in b.layout.bins[1])
        return obs[-1] == k and obs[-2] == 0 and any(w == k for r in b.layout.batches for w in r[1].widths) and clamp_run(b) >= 60
    return [search(make, accept, 6000)]


def g_two(width):
    """Two latent variables.  Primary forced to kA / kB (15 / 16: either side of kFlFast2; the top two widths at 8 bits) beside a narrow
    trained secondary; secondary forced to 7 and 8 (either side of kFlFast2's other limit) beside a trained primary; a constant secondary
    with the primary at 1, kA, kB (either side of kFlTriv2); a one-bin secondary that carries offset bits; a one-bin primary beside a
    several-bin secondary; orders 0..2 on the primary."""
    out = []
    kA, kB = (15, 16) if width >= 16 else (7, 8)
    for kind, dt, mkw in TWO_VAR[width]:
        orders = (0, 1, 2) if kind != "fquant" else (0,)
        def row(label, order, sec, seed, tbl, n=3 * 256 + 77):
            kw = dict(mkw, **consecutive(order), **dict(tbl, tbl_seed=seed % 11 + 1))
            return build(Row(f"{kind} {label} order={order} seed={seed}", two_data(kind, dt, mkw, n, seed, order, sec), kw), "two")
        for i, k in enumerate((kA, kB)):
            for order in orders[:2]:
                out.append(search(lambda s: row(f"primary k={k}, narrow secondary", order, 3, s, forced(k)),
                                  lambda b: exact(b, 1, k) and len(b.layout.bins[2]) > 1, 7000 + i))
        for k in (7, 8):
            out.append(search(lambda s: row(f"secondary k={k}, trained primary", 0, 3, s, forced(k, O.TBL_SECONDARY)), lambda b: exact(b, 2, k), 7100))
        for i, k in enumerate((1, kA, kB)):
            order = orders[i % len(orders)]
            out.append(search(lambda s: row(f"constant secondary, primary k={k}", order, 0, s, forced(k)),
                              lambda b: exact(b, 1, k) and P.trivial(b.layout, 2) and len(b.layout.bins[1]) > 1, 7200 + i))
        out.append(search(lambda s: row("one-bin secondary with offset bits", 0, 4, s, forced(3, O.TBL_SECONDARY, tbl_n_bins=1)),
                          lambda b: len(b.layout.bins[2]) == 1 and b.layout.bins[2][0][2] == 3 and len(b.layout.bins[1]) > 1, 7300))
        out.append(search(lambda s: row("one-bin primary, several-bin secondary", 0, 3, s, forced(7, tbl_n_bins=1)),
                          lambda b: len(b.layout.bins[1]) == 1 and b.layout.bins[1][0][2] == 7 and len(b.layout.bins[2]) > 1, 7400))
    return out


def g_wide(width):
    """k beyond 16: dec_expand_kernel's per-field path, two dwords a field at 32 bits and three at 64."""
    return [search(lambda s: classic_row(width, "wide", "wide", k, 256 + 200 + s % 50, s, order=s % 3, signed=s % 2 == 1), lambda b: exact(b, 1, k), 8000 + k)
            for k in ks(width, K_WIDE)]


def g_2048(width):
    """64-bit fields at 64 bits: a last batch of 255 latents starting on residue 0 (need_bytes 2048: the stage's first 512 dwords) and on
    another (2052: dwords 512.. fetched), and full batches off residue 0, whose last field lies in dword 512."""
    if width < 64: return []
    out = []
    for name, ok in (("2048", lambda s: s & 31 == 0), ("2052", lambda s: s & 31 != 0)):
        out.append(search(lambda s: classic_row(64, "2048", f"need_bytes={name}", 64, 256 + 255, s, m=3 + s % 4),
                          lambda b: exact(b, 1, 64) and starts(b.layout, 1)[-1][2] == 255 and ok(starts(b.layout, 1)[-1][1]), 9000, 2000))
    out.append(search(lambda s: classic_row(64, "2048", "last=256", 64, 512, s), lambda b: exact(b, 1, 64) and any(s & 31 for _, s, _ in starts(b.layout, 1)), 9100))
    return out


def g_lb(width):
    """Lookback (dec_expand_lb_kernel): the delta variable's bins at 1 and 16 bits at least (its lowers cannot be moved: the fields of this
    variable are small numbers in wide fields, the one group whose top bits are clear)."""
    out = []
    for k in (1, 16):
        def make(s):
            x = few(UINT[width], 700, s, m=6)
            kw = dict(CLASSIC, delta=O.TE_DELTA_LOOKBACK, window_n_log=4, lookback_seed=s, tbl_vars=O.TBL_DELTA, tbl_ob_mode=O.TBL_OB_ALL, tbl_ob_value=k, tbl_seed=s)
            return build(Row(f"lookback, delta variable at {k} seed={s}", x, kw), "lb")
        out.append(search(make, lambda b: b.layout.present[0] and min(x[2] for x in b.layout.bins[0]) >= k and P.max_ob(b.layout, 0) == max(k, 3 if k == 1 else k), 9500))
    return out


def tail_kind(b):
    """Where the first lane of the safe-load tail stands in the last item of the chunk: "in" (its slice starts inside the chunk and
    straddles src_len + 16), "beyond" (wholly beyond src_len), or None (no lane takes the safe path)."""
    lay = b.layout
    v = max(lay.batches[-1]) if lay.batches and lay.batches[-1] else None
    if v is None: return None
    s, widths = M.item(lay, v, len(lay.batches) - 1)
    safe = [first for _, how, first in M.expand_tail(M.Mem(b.chunk, 0), s, len(widths), P.max_ob(lay, v)) if how == "safe"]
    if not safe: return None
    return "in" if safe[0] < len(b.chunk) else "beyond"


def g_tail(width):
    k = min(width, 24)
    return [search(lambda s: classic_row(width, "tail", f"tail {kind}", k, 300 + s % 64, s), lambda b: exact(b, 1, k) and tail_kind(b) == kind, 9700)
            for kind in ("in", "beyond")]


def general_fields(b):
    """{(sh, ob)} over the fields of a chunk as unpack_offsets meets them."""
    return {(pos & 7, w) for pos, w in P.fields(b.layout) if w}


def g_general(width):
    """257 bins: pco_decode_kernel.  k up to the full width; fields with sh + ob = 64 and 65; 64-bit fields at sh 0 and 7."""
    out = []
    for k in ks(width, K_GENERAL):
        def accept(b):
            f = general_fields(b)
            return exact(b, 1, k) and len(b.layout.bins[1]) == 257 and (k < 57 or ((64 - k, k) in f and (min(65 - k, 7), k) in f)) and (k < 64 or (0, 64) in f)
        out.append(search(lambda s: classic_row(width, "general", "257 bins", k, 600 + s % 100, s, order=s % 2, m=6, tbl_n_bins=257, tbl_ans_size_log=O.TBL_ANS_MIN), accept, 9900 + k))
    return out


MAKERS = dict(zip(GROUPS, (g_res, g_last, g_nd, g_bins, g_one16, g_two, g_wide, g_2048, g_lb, g_tail, g_general)))


@functools.lru_cache(maxsize=None)
def built(width):
    out = []
    for g in GROUPS: out += MAKERS[g](width)
    labels = [b.row.label for b in out]
    assert len(set(labels)) == len(labels), [l for l in labels if labels.count(l) > 1]
    return tuple(out)


def rows(width):
    return [tuple(b.row) for b in built(width)]


# ---------------------------------------------------------------------------------------------------------------- where a row goes
def walker(layout):
    """decode_fast.hip's selection: "k8" / "k4" (the walkers, then dec_expand_kernel) or "general" (pco_decode_kernel)."""
    pres = [v for v in range(3) if layout.present[v]]
    t = sum((4 << layout.asl[v]) + 8 for v in pres)
    if (max(len(layout.bins[v]) for v in pres) > kFastMaxBins or max(layout.asl[v] for v in pres) > kFastMaxAns or t > K4_TABLE_BYTES
            or (layout.delta == P.DELTA_LOOKBACK and layout.mode != P.MODE_CLASSIC)):
        return "general"
    return "k4" if t > K8_TABLE_BYTES else "k8"


def path(layout):
    """"trail1" / "trail2" (a candidate of dec_trail_kernel<L, false> / <L, true> in a call of kTrailMinChunks chunks), "expand", "expand_lb",
    "general"."""
    w = walker(layout)
    if w == "general": return "general"
    if layout.delta == P.DELTA_LOOKBACK: return "expand_lb"
    nb, mo = [len(x) for x in layout.bins], [P.max_ob(layout, v) for v in range(3)]
    prim = w == "k8" and layout.order <= 2 and 1 <= nb[1] <= kTrailMaxBins and mo[1] <= kTrailMaxOb
    if not layout.present[2]:
        return "trail1" if layout.mode == P.MODE_CLASSIC and prim and nb[1] > 1 else "expand"
    if prim and 1 <= nb[2] <= kTrailMaxBins and mo[2] <= kTrailMaxOb and (nb[1] > 1 or nb[2] > 1): return "trail2"
    return "expand"


# ---------------------------------------------------------------------------------------------------------------- coverage
def coverage(bs):
    """Everything the issue asks of a width's rows, computed from their layouts alone."""
    c = dict(residues=collections.defaultdict(set), lasts=collections.defaultdict(set), state_only=set(), nd=collections.defaultdict(set), window_ends=set(),
             bins=collections.defaultdict(set), refusals=set(), clamp_run=0, two=set(), bodies=set(), wide=set(), need_bytes=set(), dword512=False,
             lb=set(), tails=set(), general_k=set(), general_fields=set(), paths=collections.Counter())
    for b in bs:
        lay = b.layout; p = path(lay); c["paths"][p] += 1
        nb, mo = [len(x) for x in lay.bins], [P.max_ob(lay, v) for v in range(3)]
        uniform = exact(b, 1, mo[1])
        if p == "trail1" and uniform:
            k = mo[1]
            c["residues"][k] |= {s & 31 for _, s, _ in starts(lay, 1, True)}
            c["lasts"][k].add(starts(lay, 1)[-1][2])
            if lay.order and lay.batches[-1] == {}: c["state_only"].add(lay.order)
            c["bins"][k].add(nb[1])
            for bi, s, cnt in starts(lay, 1):
                nd = M.trail_nd(s, cnt, k); c["nd"][k].add(nd)
                if nd in (64, 65, 128, 129):
                    _, excl = M._lanes(lay.batches[bi][1].widths)
                    c["window_ends"] |= {(((s & 31) + excl[l]) >> 5) + 2 for l in range((cnt + 3) // 4)}
        if p == "trail1" and not uniform:   # (TBL_OB_ONE) dwords the last batch's fetch asks for beyond the clamp
            c["clamp_run"] = max(c["clamp_run"], clamp_run(b))
        if p == "expand" and not lay.present[2] and lay.mode == P.MODE_CLASSIC:
            if nb[1] > kTrailMaxBins: c["refusals"].add("65 bins")
            if mo[1] == kTrailMaxOb + 1: c["refusals"].add("k=17")
            if mo[1] > kTrailMaxOb and uniform: c["wide"].add(mo[1])
            if mo[1] == 64:
                for bi, s, cnt in starts(lay, 1):
                    c["need_bytes"].add(M.expand_need_bytes(s, cnt, 64))
                    if ((s & 31) + 64 * cnt + 31) // 32 > 512: c["dword512"] = True
        if p == "trail2":
            c["two"].add((lay.mode, lay.order, mo[1], nb[1], mo[2], nb[2])); c["bodies"] |= set(M.fast_bodies(lay)) or {"none"}
        if p == "trail1": c["bodies"] |= set(M.fast_bodies(lay)) or {"none1"}
        if p == "expand_lb": c["lb"].add(min(x[2] for x in lay.bins[0]))
        if p != "general": c["tails"].add(tail_kind(b))
        if p == "general" and uniform:
            c["general_k"].add(mo[1]); c["general_fields"] |= general_fields(b)
    return c


def missing(width, bs):
    """What the rows `bs` of a width leave uncovered (empty: they cover what the issue asks)."""
    c = coverage(bs); out = []
    def need(ok, what):
        if not ok: out.append(f"u{width}: {what}")
    for k in ks(width, K_TRAIL):
        need(c["residues"][k] == set(range(32)), f"k={k}: start residues of full batches {sorted(set(range(32)) - c['residues'][k])} missing")
        need(set(LAST_BATCHES) <= c["lasts"][k], f"k={k}: last batches {sorted(set(LAST_BATCHES) - c['lasts'][k])} missing")
    need({1, 2} <= c["state_only"], "a last batch of delta state only, orders 1 and 2")
    for k, seams in ND_SEAMS.items():
        if k <= width: need(set(seams) <= c["nd"][k], f"k={k}: nd {sorted(set(seams) - c['nd'][k])} missing")
    ends = {e for k, es in WINDOW_ENDS.items() if k <= width for e in es}
    need(ends <= c["window_ends"], f"a lane whose window ends at dword {sorted(ends - c['window_ends'])}")
    need({2, 63, 64} <= set().union(*c["bins"].values()), "2, 63 and 64 bins")
    need("65 bins" in c["refusals"], "65 bins (a refusal)")
    if width >= 32: need("k=17" in c["refusals"], "k=17 (a refusal)")
    need(c["clamp_run"] >= 60, f"TBL_OB_ONE: a last batch whose fetch runs a register past the clamp (it runs {c['clamp_run']} dwords)")
    kA, kB = (15, 16) if width >= 16 else (7, 8)
    two = c["two"]
    for mode in {P.MODE_INT_MULT} | ({P.MODE_FLOAT_MULT, P.MODE_FLOAT_QUANT} if width >= 16 else set()):
        mine = [t for t in two if t[0] == mode]
        for k in (kA, kB):
            need(any(t[2] == k and t[5] > 1 for t in mine), f"mode {mode}: primary k={k} beside a several-bin secondary")
            need(any(t[2] == k and t[5] == 1 and t[4] == 0 for t in mine), f"mode {mode}: primary k={k} beside a constant secondary")
        need(any(t[2] == 1 and t[5] == 1 and t[4] == 0 for t in mine), f"mode {mode}: primary k=1 beside a constant secondary")
        need({7, 8} <= {t[4] for t in mine}, f"mode {mode}: secondary k=7 and k=8")
        need(any(t[5] == 1 and t[4] > 0 for t in mine), f"mode {mode}: a one-bin secondary with offset bits")
        need(any(t[3] == 1 and t[5] > 1 for t in mine), f"mode {mode}: a one-bin primary beside a several-bin secondary")
        need({t[1] for t in mine} >= ({0, 1, 2} if mode != P.MODE_FLOAT_QUANT else {0}), f"mode {mode}: orders on the primary")
    need({"pair", "pair2t", "pair2", "none", "none1"} <= c["bodies"], f"candidates of every straight-line body and of none: {sorted(c['bodies'])}")
    need(set(ks(width, K_WIDE)) <= c["wide"], f"wide k {sorted(set(ks(width, K_WIDE)) - c['wide'])} missing")
    if width == 64:
        need({2048, 2052} <= c["need_bytes"], f"need_bytes 2048 and 2052 (have {sorted(c['need_bytes'])})")
        need(c["dword512"], "a 64-bit section whose last field lies in dword 512")
    need({1, 16} <= c["lb"], "Lookback rows with the delta variable at 1 and at 16 bits")
    need({"in", "beyond"} <= c["tails"], f"safe-load tails starting inside and beyond the chunk (have {sorted(map(str, c['tails']))})")
    need(set(ks(width, K_GENERAL)) <= c["general_k"], f"general-kernel k {sorted(set(ks(width, K_GENERAL)) - c['general_k'])} missing")
    gf = c["general_fields"]
    if width == 64:
        need(any(sh + ob == 64 for sh, ob in gf) and any(sh + ob == 65 for sh, ob in gf), "general-kernel fields with sh + ob = 64 and 65")
        need((0, 64) in gf and (7, 64) in gf, "general-kernel 64-bit fields at sh 0 and 7")
    return out


def readers(b):
    """The model functions that apply to a row: [(name, variable, batch, function of (mem, mutants))] -- the expanders' general bodies for
    every item of a trail candidate and their straight-line bodies for its full batches, dec_expand_kernel's reader for every chunk a walker
    takes (a small call sends the trail candidates there too), pco_decode_kernel's for the others."""
    lay = b.layout; p = path(lay); out = []
    for bi, r in enumerate(lay.batches):
        for v in sorted(r):
            if p == "general":
                out.append(("general", v, bi, lambda mem, mu, v=v, bi=bi: M.general(mem, lay, v, bi, mu))); continue
            out.append(("expand", v, bi, lambda mem, mu, v=v, bi=bi: M.expand(mem, lay, v, bi, mu)))
            if p not in ("trail1", "trail2"): continue
            out.append(("trail_general", v, bi, lambda mem, mu, v=v, bi=bi: M.trail_general(mem, lay, v, bi, mu)))
            if len(r[v].widths) == 256 and M.fast_batch(lay, bi):
                for body in M.fast_bodies(lay):
                    if body == "pair2t" and v == 2: continue
                    out.append((f"trail_fast[{body}]", v, bi, lambda mem, mu, v=v, bi=bi, body=body: M.trail_fast(mem, lay, v, bi, body, mu)))
    return out
