"""Where every bit of a page lies: a pure-Python layout model of one standalone chunk, and the encoder's pack arithmetic restated over it.

Written from the format description and the reference's text -- metadata/chunk.rs (mode, delta encoding, per-variable
bin tables), page_latent_var.rs (delta state, four final tANS states per variable), chunk_latent_compressor.rs:134-169, 272-329 (batch after
batch, variable after variable: the tANS fields of the batch, then its offsets; a variable with delta state stores that many latents fewer;
a single bin without offset bits writes nothing, one with offset bits writes offsets only).  It shares tans_model's table construction
(decoder_nodes) and nothing with the oracle: the oracle writes a chunk, this file re-derives its length, its padding and the position of
every section of every batch from the chunk's bytes alone.  Values are skipped; only the tANS chains are followed (their bits decide where
everything else lies).

The second half restates, as plain arithmetic, what the encoder's bit packers decide from those positions (encode_fast.hip,
encode_walkpack.hip, encode_kernels.hip): which kernel packs a page (route), where a page is cut into runs (runs), when the LDS stage of a
run is flushed (sink_schedule) and how wide the widest offset of each batch is (bmax_of).  VARIANTS names three wrong restatements; the
CPU suite shows that each changes at least one row's answer."""
import collections

from tans_model import BATCH_N, INTERLEAVING, decoder_nodes

DTYPE_BITS = {1: 32, 2: 64, 3: 32, 4: 64, 5: 32, 6: 64, 7: 16, 8: 16, 9: 16, 10: 8, 11: 8}
OB_BITS = {8: 4, 16: 5, 32: 6, 64: 7}                  # bits of a bin's offset_bits field: enough for 0 .. latent width
MODE_CLASSIC, MODE_INT_MULT, MODE_FLOAT_MULT, MODE_FLOAT_QUANT = range(4)   # the ChunkMeta's mode variants
DELTA_NONE, DELTA_CONSECUTIVE, DELTA_LOOKBACK = range(3)                    # ... and delta variants
VAR_NAMES = ("delta", "primary", "secondary")
VARIANTS = ("offsets_first", "runs32", "no_reach")     # offsets before tANS bits | runs of 32 batches | a reserve without the + 96

kRunBatches = 64           # encode_fast.hip: batches per pack run
kStgDwords = 704           # encode_kernels.hip: dwords of a run's LDS stage
kPutReach = 96             # PackSink::reserve: room for the three dwords a 64-bit put may touch
kFastEncMaxAsl = 10        # larger tANS tables take enc_page_kernel
kMaxFastBins = 256
kDirectHistRange = 4096    # enc_walkp_kernel looks bins up by value: 16-bit latents spanning fewer values than this
kWsMinBatches, kWsMaxItems = 64, 4096   # long pages of small calls are walked in segments: enc_walkp_kernel is off for such a call
kWpQ = 16                  # items per enc_walkp_kernel block
kWpSymOff = 2928           # encode_walkpack.hip: where the tables of an item must end in its LDS slot

Section = collections.namedtuple("Section", "var batch pos ans_bits off_bits widths")   # pos: first bit, relative to the chunk's first byte
Layout = collections.namedtuple("Layout", "latent_bits n mode delta order state_n present asl bins n_lat meta_end head_bits body_first body_last end_bits batches")


class Reader:
    """Bit i of the stream is bit (i mod 8) of byte i // 8, fields are little-endian (tans_model.Bits on bytes: no whole-stream shifts)."""

    def __init__(self, data):
        self.d = bytes(data); self.n = 8 * len(self.d); self.pos = 0

    def read(self, bits):
        p = self.pos; b = p >> 3
        self.pos = p + bits
        assert self.pos <= self.n, "read past the end"
        return (int.from_bytes(self.d[b:b + 10], "little") >> (p & 7)) & ((1 << bits) - 1)

    def skip(self, bits):
        self.pos += bits
        assert self.pos <= self.n, "skipped past the end"

    def align(self):
        assert self.read(-self.pos % 8) == 0, "non-zero padding"


def parse_chunk(chunk):
    """One standalone chunk (number type byte, 24 bits of n - 1, ChunkMeta, one page) -> Layout.  Fails if the chunk does not end, zero-padded,
    exactly where the last batch does."""
    r = Reader(chunk)
    lb = DTYPE_BITS[r.read(8)]
    n = r.read(24) + 1
    mode = r.read(4)
    assert mode in (MODE_CLASSIC, MODE_INT_MULT, MODE_FLOAT_MULT, MODE_FLOAT_QUANT), mode
    if mode in (MODE_INT_MULT, MODE_FLOAT_MULT): r.skip(lb)
    elif mode == MODE_FLOAT_QUANT: r.skip(8)
    delta = r.read(4); order = 0; state_n = 0
    assert delta in (DELTA_NONE, DELTA_CONSECUTIVE, DELTA_LOOKBACK), delta
    if delta == DELTA_CONSECUTIVE:
        order = r.read(3); assert r.read(1) == 0, "a delta'd secondary"
        state_n = order
    elif delta == DELTA_LOOKBACK:
        r.skip(5); state_n = 1 << r.read(4); assert r.read(1) == 0, "a delta'd secondary"
    present = (delta == DELTA_LOOKBACK, True, mode != MODE_CLASSIC)
    asl = [0, 0, 0]; bins = [[], [], []]
    for v in range(3):
        if not present[v]: continue
        vb = 32 if v == 0 else lb                   # the lookback variable is 32 bits wide whatever the type
        asl[v] = r.read(4); nb = r.read(15)
        assert asl[v] <= 14 and nb <= 1 << asl[v] and not (nb == 1 and asl[v] > 0), (v, asl[v], nb)
        for _ in range(nb):
            w = r.read(asl[v]) + 1; lower = r.read(vb); ob = r.read(OB_BITS[vb])
            assert ob <= vb
            bins[v].append((w, lower, ob))
    r.align()
    meta_end = r.pos
    # the page: per variable its delta state (the primary's), then four final tANS states
    state = [None, None, None]
    for v in range(3):
        if not present[v]: continue
        if v == 1: r.skip(lb * state_n)
        state[v] = [r.read(asl[v]) for _ in range(INTERLEAVING)]
    r.align()
    head_bits = r.pos
    n_lat = [0, 0, 0]
    for v in range(3):
        if present[v]: n_lat[v] = n if v == 2 else max(n - state_n, 0)
    nodes = [decoder_nodes(asl[v], [b[0] for b in bins[v]]) if present[v] and len(bins[v]) > 1 else None for v in range(3)]
    writes = [present[v] and len(bins[v]) >= 1 and not (len(bins[v]) == 1 and bins[v][0][2] == 0) for v in range(3)]
    data = r.d
    batches = []
    for b in range((n + BATCH_N - 1) // BATCH_N):
        row = {}
        for v in range(3):
            base = b * BATCH_N
            if not writes[v] or base >= n_lat[v]: continue
            cnt = min(BATCH_N, n_lat[v] - base)
            start = r.pos
            if nodes[v] is None:
                widths = [bins[v][0][2]] * cnt; ans = 0
            else:
                nd = nodes[v]; st = state[v]; obs = [x[2] for x in bins[v]]; widths = []
                pos = r.pos
                for i in range(cnt):
                    j = i & 3
                    s, bits, nxt = nd[st[j]]
                    widths.append(obs[s])
                    q = pos >> 3
                    st[j] = nxt + ((int.from_bytes(data[q:q + 4], "little") >> (pos & 7)) & ((1 << bits) - 1))
                    pos += bits
                assert pos <= r.n, "read past the end"
                ans = pos - r.pos
                r.pos = pos
            off = sum(widths)
            r.skip(off)
            row[v] = Section(v, b, start, ans, off, widths)
        batches.append(row)
    body_last = r.pos
    r.align()
    assert r.pos == r.n, ("the chunk does not end where its last batch does", r.pos, r.n)
    return Layout(lb, n, mode, delta, order, state_n, present, tuple(asl), tuple(tuple(b) for b in bins), tuple(n_lat), meta_end, head_bits,
                  head_bits, body_last, r.pos, batches)


# ---------------------------------------------------------------------------------------------------------------- views of a layout
def sections(layout, variants=()):
    """Every section in stream order: (var, batch, kind "ans" | "off", first bit, bits).  Under "offsets_first" the two sections of a
    (variable, batch) swap places."""
    out = []
    for row in layout.batches:
        for v in sorted(row):
            s = row[v]
            if "offsets_first" in variants:
                out.append((v, s.batch, "off", s.pos, s.off_bits)); out.append((v, s.batch, "ans", s.pos + s.off_bits, s.ans_bits))
            else:
                out.append((v, s.batch, "ans", s.pos, s.ans_bits)); out.append((v, s.batch, "off", s.pos + s.ans_bits, s.off_bits))
    return out


def fields(layout, variants=()):
    """Every offset field of the body in stream order: (first bit, width)."""
    out = []
    for v, b, kind, pos, bits in sections(layout, variants):
        if kind != "off": continue
        for w in layout.batches[b][v].widths:
            out.append((pos, w)); pos += w
    return out


def what_lies_at(layout, bit):
    """For a failure report: which part of the chunk holds `bit`."""
    if bit < layout.meta_end: return "chunk meta"
    if bit < layout.head_bits: return "page meta"
    for v, b, kind, pos, bits in sections(layout):
        if pos <= bit < pos + bits:
            return f"{VAR_NAMES[v]} batch {b} {'tANS' if kind == 'ans' else 'offset'} section, bit {bit - pos} of {bits}"
    return "final padding" if bit < layout.end_bits else "beyond the chunk"


def batch_start(layout, b):
    row = layout.batches[b]
    return row[min(row)].pos if row else None


def runs(layout, variants=()):
    """First bit of every run of kRunBatches batches (enc_scan_kernel's run_start; run 0 starts behind the head).  A page whose variables
    write nothing has one run of no bits."""
    per = 32 if "runs32" in variants else kRunBatches
    out = []
    pos = layout.body_first
    for b, row in enumerate(layout.batches):
        if row: pos = row[min(row)].pos
        elif b and layout.batches[b - 1]:
            last = layout.batches[b - 1]; s = last[max(last)]; pos = s.pos + s.ans_bits + s.off_bits
        if b % per == 0: out.append(pos)
    return out or [layout.body_first]


def run_ends(layout, variants=()):
    st = runs(layout, variants)
    return st[1:] + [layout.body_last]


def bmax_of(layout, v, b):
    """The widest offset of batch b of variable v: what pack_item_t / pack1_item choose their puts by when the variable's widest is above 16."""
    return max(layout.batches[b][v].widths, default=0)


def max_ob(layout, v):
    return max((x[2] for x in layout.bins[v]), default=0)


def trivial(layout, v):
    return len(layout.bins[v]) == 0 or (len(layout.bins[v]) == 1 and layout.bins[v][0][2] == 0)


# ---------------------------------------------------------------------------------------------------------------- the stage of a run
def sink_schedule(start_bit, secs, variants=()):
    """PackSink::reserve / commit / flush restated.  `secs`: [(reserve, commit)] -- what a packer asks room for, and what it then commits
    (reserve None: a commit without a reserve, as finish_byte's).  Returns (flushes, distances, pends): the bit at which the stage was
    flushed, per flush; per reserve the bits left below the threshold (negative: it flushed) and the bits staged when it was made."""
    reach = 0 if "no_reach" in variants else kPutReach
    outbit, pend = start_bit, 0
    flushes, dist, pends = [], [], []
    for sec in secs:
        reserve, commit = sec[0], sec[1]
        if reserve is not None:
            d = kStgDwords * 32 - ((outbit & 31) + pend + reserve + reach)
            dist.append(d); pends.append(pend)
            if d < 0:
                outbit += pend; pend = 0
                flushes.append(outbit)
        pend += commit
    return flushes, dist, pends


def head_sections(layout):
    """pack_run's head of run 0: put_uniform reserves 64 per field, the bin tables 64 entries at a time."""
    lb = layout.latent_bits
    secs = [(64, 8), (64, 24), (64, 4)]
    if layout.mode in (MODE_INT_MULT, MODE_FLOAT_MULT): secs.append((64, lb))
    elif layout.mode == MODE_FLOAT_QUANT: secs.append((64, 8))
    secs.append((64, 4))
    if layout.delta == DELTA_CONSECUTIVE: secs += [(64, 3), (64, 1)]
    elif layout.delta == DELTA_LOOKBACK: secs += [(64, 5), (64, 4), (64, 1)]
    pos = sum(c for _, c in secs)
    for v in range(3):
        if not layout.present[v]: continue
        vb = 32 if v == 0 else lb
        secs += [(64, 4), (64, 15)]; pos += 19
        bin_bits = layout.asl[v] + vb + OB_BITS[vb]
        nb = len(layout.bins[v])
        for b0 in range(0, nb, 64):
            secs.append((64 * bin_bits, min(64, nb - b0) * bin_bits)); pos += min(64, nb - b0) * bin_bits
    secs.append((None, -pos % 8)); pos += -pos % 8
    assert pos == layout.meta_end, (pos, layout.meta_end)
    for v in range(3):
        if not layout.present[v]: continue
        if v == 1: secs += [(64, lb)] * layout.state_n; pos += lb * layout.state_n
        secs += [(64, layout.asl[v])] * 4; pos += 4 * layout.asl[v]
    secs.append((None, -pos % 8)); pos += -pos % 8
    assert pos == layout.head_bits, (pos, layout.head_bits)
    return secs


def body_sections(layout, first, last, exact):
    """The reserves of batches [first, last): pack1_item (exact) reserves a variable's batch as it is, pack_item_t its latents times the
    table's width plus its latents times the variable's widest offset."""
    secs = []
    for b in range(first, min(last, len(layout.batches))):
        for v in sorted(layout.batches[b]):
            s = layout.batches[b][v]; cnt = len(s.widths)
            if exact: secs.append((s.ans_bits + s.off_bits, s.ans_bits + s.off_bits, (v, b)))
            else: secs.append(((cnt * layout.asl[v] if len(layout.bins[v]) > 1 else 0) + cnt * max_ob(layout, v), s.ans_bits + s.off_bits, (v, b)))
    return secs


def run_schedules(layout, rt, variants=()):
    """sink_schedule of every stage a routed page goes through: [(what, flushes, distances, pends, tags)], `tags` naming each reserve
    ("head", or (variable, batch)).  A lean page's head is a stage of its own (enc_pack_kernel stops behind it); a general page's run 0
    carries the head's stage on into the body; "copy" stores its body without a stage; "walkp" and "page" do not use PackSink."""
    def stage(what, start, secs):
        return (what,) + sink_schedule(start, secs, variants) + ([x[2] if len(x) > 2 else "head" for x in secs if x[0] is not None],)
    if rt == "page": return []
    head = head_sections(layout)
    if rt in ("copy", "walkp"): return [stage("head", 0, head)]
    per = 32 if "runs32" in variants else kRunBatches
    out = []
    for k, start in enumerate(runs(layout, variants)):
        body = body_sections(layout, k * per, (k + 1) * per, rt != "general")
        if k == 0 and rt == "general": out.append(stage("head+run0", 0, head + body))
        elif k == 0: out += [stage("head", 0, head), stage("run0", start, body)]
        else: out.append(stage(f"run{k}", start, body))
    return out


# ---------------------------------------------------------------------------------------------------------------- routes
def fast_ok(layout):
    """enc_train_kernel: a chunk takes the fast kernels unless a variable's table is larger than 2^10 or has more than 256 bins.  (A chunk the
    encoder fell back on -- should_fallback -- is not fast either: such a chunk is Classic with one full-width bin, and no row here is one.)"""
    return all(not layout.present[v] or (layout.asl[v] <= kFastEncMaxAsl and len(layout.bins[v]) <= kMaxFastBins) for v in range(3))


def pack1_mask(layout, compact):
    """encode_fast.hip pack1_mask: 0, or the mask of the one or two variables a lean kernel packs."""
    mask = 0; n_on = 0
    for v in range(3):
        if not layout.present[v] or trivial(layout, v): continue
        mask |= 1 << v; n_on += 1
        if len(layout.bins[v]) > 256: return 0
        if not compact[v] and layout.latent_bits < 32: return 0
    if not (mask & 2) or n_on > 2: return 0
    if is_copy(layout, compact): return 0
    return mask


def is_copy(layout, compact):
    """pack_run's shifted copy: the primary alone, one bin, no tANS, offsets as wide as the latent, full-width latents."""
    on = [layout.present[v] and not trivial(layout, v) for v in range(3)]
    return on[1] and not on[0] and not on[2] and len(layout.bins[1]) == 1 and layout.bins[1][0][2] == layout.latent_bits and not compact[1]


def worst_bits(asl, bins):
    """Most tANS + offset bits one latent of a variable can take (enc_walkp_kernel: at most 16)."""
    return max(asl - (int(2 * w - 1).bit_length() - 1) + 1 + int(ob) for w, _, ob in bins)


def wp_fits(asl, n_bins):
    """encode_walkpack.hip wp_fits: next states u16[2^asl], then twelve bytes per bin, below the slot's symbol area."""
    return (((2 << asl) + 7) & ~7) + 12 * n_bins <= kWpSymOff


def walkp_primary(asl, bins):
    """The block test's word on a primary variable that writes something, as far as its bin table shows: something to walk (two bins or more),
    at most 256 bins, bins spanning fewer than 4096 latents (their span stands for the variable's range), no latent of more than 16 tANS +
    offset bits."""
    span = max(lo + (1 << ob) - 1 for _, lo, ob in bins) - min(lo for _, lo, _ in bins)
    return 2 <= len(bins) <= 256 and span < kDirectHistRange and worst_bits(asl, bins) <= 16


def walkp_item(mode, present, asl, bins):
    """What enc_walkp_kernel's block test (encode_walkpack.hip, pass 1) makes of a ONE-variable chunk with 16-bit latents, as far as its
    ChunkMeta shows: "trivial" (one bin without offset bits: nothing of it reaches the page body, it never breaks a block), "refuse" (more
    than one variable, or walkp_primary says no), else "ok".  (Whether the tables fit the block's LDS slot is not checked here; chunks of at
    most a few dozen bins always do.  walkp_verdict is the test for any page of any call.)"""
    if mode != MODE_CLASSIC or present[0] or present[2]:
        return "refuse"
    if len(bins[1]) == 1 and bins[1][0][2] == 0:
        return "trivial"
    return "ok" if walkp_primary(asl[1], bins[1]) else "refuse"


def walkp_verdict(layout, compact, v):
    """Pass 1 of enc_walkp_kernel for the item (page, variable v): "idle" (nothing of it reaches the body), "ok", or "bad" (it breaks its
    block): the item must be the page's primary, the only variable of the page that writes, held as 16-bit latents, with tables that fit
    the slot, and pass walkp_primary."""
    def writes(u): return fast_ok(layout) and layout.present[u] and not trivial(layout, u)
    if not writes(v): return "idle"
    if v != 1 or writes(0) or writes(2) or layout.n_lat[1] == 0 or not compact[1] or not wp_fits(layout.asl[1], len(layout.bins[1])): return "bad"
    return "ok" if walkp_primary(layout.asl[1], layout.bins[1]) else "bad"


def call_slots(kws):
    """The variables that have a latent slot in a call of chunks with these configs, in slot order (pco_gfx_encode_api.inc: the lookback
    variable when a chunk asks for lookback, the primary, the secondary when a chunk asks for a mode other than Classic)."""
    return ((0,) if any(kw.get("delta") == 3 for kw in kws) else ()) + (1,) + ((2,) if any(kw.get("mode") != 1 for kw in kws) else ())


def call_walkp(layouts, compacts, slots=(1,)):
    """Per page of ONE call (one page per chunk): whether enc_walkp_kernel packs it -- the kernel runs, the page's primary writes and every
    item of its block of sixteen (page, variable) items is "ok" or "idle".  The kernel is off when the call is walked in segments (a page of
    64 batches or more among at most 4096 items)."""
    n_items = len(layouts) * len(slots)
    assert n_items <= 8192 or len(slots) == 1, "more than 8192 items of several variables: the 16-per-wave walker takes part, not modelled"
    if max(l.n for l in layouts) >= kWsMinBatches * BATCH_N and n_items <= kWsMaxItems:
        return [False] * len(layouts)
    verdicts = [walkp_verdict(layouts[i // len(slots)], compacts[i // len(slots)], slots[i % len(slots)]) for i in range(n_items)]
    out = []
    for p in range(len(layouts)):
        item = p * len(slots) + slots.index(1)
        blk = verdicts[item // kWpQ * kWpQ: item // kWpQ * kWpQ + kWpQ]
        out.append(verdicts[item] == "ok" and "bad" not in blk)
    return out


def route(layout, compact, walkp=False):
    """Which kernel packs the page: "page" (enc_page_kernel), "walkp" (enc_walkp_kernel + enc_place_kernel; `walkp`: call_walkp's word for
    the page), "copy" (the general kernel's shifted copy), "lean<mask>" / "lean<mask, wide>" (enc_pack1_kernel), "general"."""
    if not fast_ok(layout): return "page"
    if walkp: return "walkp"
    if is_copy(layout, compact): return "copy"
    mask = pack1_mask(layout, compact)
    if not mask: return "general"
    wide = any((mask >> v) & 1 and not compact[v] for v in range(3))
    return f"lean<{mask}, wide>" if wide else f"lean<{mask}>"


# what pco_gfx_debug_pack_routes reports for a route ("copy" is a branch of the general kernel: the device does not tell the two apart)
ROUTE_BYTE = {"page": 0xff, "walkp": 15, "general": 0, "copy": 0, "lean<2>": 2, "lean<6>": 6, "lean<3>": 3, "lean<2, wide>": 10, "lean<6, wide>": 14, "lean<3, wide>": 11}
