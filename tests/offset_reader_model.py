"""The decoders' offset readers restated in plain Python: which dwords and bytes of a page body each of them fetches, where it clamps, which
window a lane gets and how the fields are cut from it.

Three pieces of device code cut offset fields out of a page body:

  * the trailing expanders (decode_trail.hip): trail_section / trail_stage_a / trail_stage_b (`trail_general`) and the straight-line bodies
    trail_fast_pair, trail_fast_pair2t and trail_fast_pair2 (`trail_fast`): a batch's section in one to three registers across the wave
    (lane l of register j: dword 64 j + l from the dword the section starts in, clamped at last = (src_len + 12) >> 2), a lane's three-dword
    window through the crossbar, four fields cut from the window;
  * expand_prefetch / expand_item of dec_expand_kernel (decode_fast.hip; the range, resume and index decoders share them): 32-byte lane
    slices staged in LDS, the dwords 512.. fetched only when need_bytes > 2048, a safe-load tail, a window path for max_ob <= 16 and a
    per-field path (`expand`);
  * unpack_offsets of pco_decode_kernel (decode_kernel.hip): two safe 64-bit loads per field, the second iff sh + ob > 64 (`general`).

Every function takes the chunk's bytes with what stands in the 16 bytes behind them (Mem), the chunk's pack_layout_model.Layout and a
(variable, batch), and returns the offsets a wave would extract for that item -- by the kernel's own dword / byte indices, clamps and masks,
never by a bit-stream reader.  `true_fields` is the bit-stream reader they are compared with.  Bits the kernels fetch but no field uses
(the lanes past a one-register section wrap round, the stage holds a previous item's dwords, ...) are modelled as they are: stale LDS is
POISON, the slack is the caller's fill byte, and a correct reader gives the same fields whatever they hold.

MUTANTS names one-place wrong readings; the CPU suite shows that each changes the answer of at least one row of offset_edges_util.py.
HARMLESS names two that cannot: they only move a bound that lies in bits no field uses (see the notes at each), and the suite pins that they
change nothing -- the day one of them does, a reader has begun to depend on its slack."""
import pack_layout_model as P

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
LANES = 64
POISON = 0xA5C3965A            # an LDS dword nobody wrote for this item
kExpStgDwords = 528            # decode_fast.hip: dwords of an item's LDS stage
kSlack = 16                    # readable bytes behind a chunk
kTrailReach = 2                # decode_trail.hip: nd = section dwords + 2 (the dwords a lane's window may reach into)
kTrailClamp = 12               # ... last = (src_len + 12) >> 2
kExpReach = 8                  # decode_fast.hip: need_bytes = section dwords * 4 + 8
kWindowMaxOb = 16              # four fields of up to 16 bits fit one 64-bit window
kFastMaxOb, kFast2MaxOb, kFast2MaxOb2 = 7, 15, 7   # kFlFast: primary 1..7; kFlFast2 / kFlTriv2: primary up to 15; kFlFast2: secondary up to 7
kTrailMaxBins = 64

MUTANTS = ("window_two_dwords", "one_register_up_to_65", "two_registers_up_to_129", "clamp_one_short", "residue_dropped",
           "stage_one_lane_short", "no_fetch_beyond_2048", "bfe_width_mod_32", "window_path_at_17", "no_second_word", "mask_at_64")
# clamp_at_len (last = src_len >> 2): the last dword that holds a bit of the chunk is (src_len - 1) >> 2 <= src_len >> 2, so no field's bits
#   move; only what the lanes past the chunk's end hold does.  clamp_one_short (last = (src_len >> 2) - 1) is the nearest clamp that matters.
# need_bytes_without_reach (no + 8): the section's own dwords are all below need_bytes - 8, so every dword that holds a field's bit is still
#   staged; the reach only keeps the dwords a window touches BEHIND the last field out of stale LDS.  stage_one_lane_short (the last staging
#   lane left out) is the nearest gate that matters.
HARMLESS = ("clamp_at_len", "need_bytes_without_reach")


class Mem:
    """A chunk as a decoder sees it: src_len bytes, then kSlack readable bytes of `fill`."""

    def __init__(self, chunk, fill):
        self.len = len(chunk); self.b = bytes(chunk) + bytes([fill]) * kSlack

    def u32(self, byte):
        """load_u32_le: a plain load, which must stay inside the chunk and its slack."""
        assert 0 <= byte and byte + 4 <= self.len + kSlack, ("a load beyond the slack", byte, self.len)
        return int.from_bytes(self.b[byte:byte + 4], "little")

    def u64_safe(self, byte):
        """load_u64_le_safe(src, byte, src_len + 16): bytes at or beyond src_len + 16 read as zero."""
        return int.from_bytes(self.b[byte:byte + 8], "little")   # (a short slice is the zero extension)


def item(layout, v, b):
    """(first bit of the offset section, widths) of variable v in batch b; None when the variable writes nothing there."""
    s = layout.batches[b].get(v) if b < len(layout.batches) else None
    return None if s is None else (s.pos + s.ans_bits, list(s.widths))


def true_fields(chunk, layout, v, b):
    """The item's offsets read as a bit stream: field i is the next widths[i] bits, little-endian."""
    start, widths = item(layout, v, b)
    whole = int.from_bytes(bytes(chunk), "little"); out = []
    for w in widths:
        out.append((whole >> start) & ((1 << w) - 1)); start += w
    return out


def _lanes(widths):
    """Per lane: its four offset-bit counts (zero past the batch's latents) and the bits of the section before its first field."""
    w = list(widths) + [0] * (4 * LANES - len(widths))
    obs = [w[4 * l:4 * l + 4] for l in range(LANES)]
    excl, acc = [], 0
    for l in range(LANES):
        excl.append(acc); acc += sum(obs[l])
    return obs, excl


def _window(w0, w1, w2, sh):
    """v_alignbit twice: 64 bits from bit sh (0..31) of the three dwords."""
    return ((w0 | (w1 << 32) | (w2 << 64)) >> (sh & 31)) & M64


def _ubfe(x, width):
    """v_bfe_u32 from bit 0: the width operand counts modulo 32."""
    return x & M32 & ((1 << (width & 31)) - 1)


def _cut4(v64, obs, cnt_left):
    out = []
    for k in range(4):
        if k < cnt_left: out.append(_ubfe(v64, obs[k]))
        v64 >>= obs[k]
    return out


def trail_nd(start, cnt, max_ob):
    """Dwords trail_section reserves for a batch: those its cnt * max_ob bits may touch, plus the reach."""
    return (((start & 31) + cnt * max_ob + 31) >> 5) + kTrailReach


def _trail_last(mem, mutants):
    if "clamp_at_len" in mutants: return mem.len >> 2
    if "clamp_one_short" in mutants: return max((mem.len >> 2) - 1, 0)
    return (mem.len + kTrailClamp) >> 2


def trail_general(mem, layout, v, b, mutants=()):
    """trail_section + trail_stage_a + trail_stage_b for one (variable, batch) of a chunk the expanders take (max_ob <= 16)."""
    start, widths = item(layout, v, b)
    cnt, max_ob = len(widths), P.max_ob(layout, v)
    if max_ob == 0: return [0] * cnt
    assert max_ob <= kWindowMaxOb, "the walker leaves wider offsets to dec_expand_kernel"
    obs, excl = _lanes(widths)
    d0, nd, last = start >> 5, trail_nd(start, cnt, max_ob), _trail_last(mem, mutants)
    reg = lambda j: [mem.u32(4 * min(d0 + 64 * j + l, last)) for l in range(LANES)]
    s0 = reg(0); s1 = reg(1) if nd > 64 else [0] * LANES; s2 = reg(2) if nd > 128 else [0] * LANES
    seam1 = 65 if "one_register_up_to_65" in mutants else 64
    seam2 = 129 if "two_registers_up_to_129" in mutants else 128
    if nd <= 64: fetch = lambda i: s0[i & 63]          # (indices past lane 63 wrap: only bits no field uses come from there)
    else: fetch = lambda i: s0[i & 63] if i < seam1 else (s1[i & 63] if i < seam2 else s2[i & 63])
    out = []
    for l in range(LANES):
        rel = (0 if "residue_dropped" in mutants else start & 31) + excl[l]; di, sh = rel >> 5, rel & 31
        w2 = 0 if "window_two_dwords" in mutants else fetch(di + 2)
        out += _cut4(_window(fetch(di), fetch(di + 1), w2, sh), obs[l], cnt - 4 * l)
    return out


def fast_bodies(layout):
    """Which straight-line body the flags of dec_trail_kernel allow a chunk with a 16-byte aligned destination: "pair" (kFlFast),
    "pair2t" (kFlTriv2), "pair2" (kFlFast2) -- what the lockstep loop tries in this order -- or none."""
    nb1, mo1 = len(layout.bins[1]), P.max_ob(layout, 1)
    if not layout.present[2]:
        return ("pair",) if nb1 > 1 and 1 <= mo1 <= kFastMaxOb else ()
    nb2, mo2 = len(layout.bins[2]), P.max_ob(layout, 2)
    out = ()
    if nb1 > 1 and 1 <= mo1 <= kFast2MaxOb and nb2 <= 1 and mo2 == 0: out += ("pair2t",)
    if mo1 <= kFast2MaxOb and mo2 <= kFast2MaxOb2: out += ("pair2",)
    return out


def fast_batch(layout, b):
    """The straight-line bodies take full batches only: 256 numbers and the delta state behind them."""
    return layout.n - b * 256 >= 256 + layout.state_n


def trail_fast(mem, layout, v, b, body, mutants=()):
    """The section fetch and window of trail_fast_pair ("pair": one register), trail_fast_pair2t ("pair2t": two) and trail_fast_pair2
    ("pair2": two for the primary, one for the secondary) for a full batch.  Crossbar indices wrap modulo 64 lanes, as ds_bpermute does."""
    start, widths = item(layout, v, b)
    assert len(widths) == 256 and fast_batch(layout, b)
    if P.max_ob(layout, v) == 0: return [0] * 256
    obs, excl = _lanes(widths)
    d0, last = start >> 5, _trail_last(mem, mutants)
    reg = lambda j: [mem.u32(4 * min(d0 + 64 * j + l, last)) for l in range(LANES)]
    sec = reg(0)
    if body == "pair" or (body == "pair2" and v == 2):
        fetch = lambda i: sec[i & 63]
    else:
        assert body in ("pair2t", "pair2") and v == 1
        hi = reg(1); seam = 65 if "one_register_up_to_65" in mutants else 64
        fetch = lambda i: sec[i & 63] if i < seam else hi[i & 63]
    out = []
    for l in range(LANES):
        rel = (0 if "residue_dropped" in mutants else start & 31) + excl[l]; di, sh = rel >> 5, rel & 31
        w2 = 0 if "window_two_dwords" in mutants else fetch(di + 2)
        out += _cut4(_window(fetch(di), fetch(di + 1), w2, sh), obs[l], 4)
    return out


def expand_need_bytes(start, cnt, max_ob, mutants=()):
    need_bits = cnt * max_ob
    if need_bits == 0: return 0
    return (((start & 31) + need_bits + 31) // 32) * 4 + (0 if "need_bytes_without_reach" in mutants else kExpReach)


def expand_tail(mem, start, cnt, max_ob):
    """How the staging lanes of an item fetch their slices: [(lane, "direct" | "safe", first byte)] for the lanes below need_bytes."""
    byte0, need = (start >> 5) * 4, expand_need_bytes(start, cnt, max_ob)
    return [(l, "direct" if byte0 + 32 * l + 32 <= mem.len + kSlack else "safe", byte0 + 32 * l) for l in range(LANES) if 32 * l < need]


def expand(mem, layout, v, b, mutants=()):
    """expand_prefetch + expand_item for one (variable, batch).  The lookback variable's latents are 32 bits wide whatever the type."""
    start, widths = item(layout, v, b)
    cnt, max_ob = len(widths), P.max_ob(layout, v)
    lv_bits = 32 if v == 0 else max(layout.latent_bits, 32)     # (8 and 16-bit latents are cut as 32-bit ones)
    if cnt * max_ob == 0: return [0] * cnt
    byte0, need = (start >> 5) * 4, expand_need_bytes(start, cnt, max_ob, mutants)
    stg = [POISON] * kExpStgDwords
    for l in range(LANES):
        off = 32 * l
        gate = off + 32 < need if "stage_one_lane_short" in mutants else off < need
        if not gate: continue
        if byte0 + off + 32 <= mem.len + kSlack:
            sl = [mem.u32(byte0 + off + 4 * k) for k in range(8)]
        else:
            sl = []
            for k in range(4):
                w = mem.u64_safe(byte0 + off + 8 * k); sl += [w & M32, w >> 32]
        stg[8 * l:8 * l + 8] = sl
    if need > 2048 and "no_fetch_beyond_2048" not in mutants:
        for l in range(2):
            w = mem.u64_safe(byte0 + 2048 + 8 * l); stg[512 + 2 * l] = w & M32; stg[513 + 2 * l] = w >> 32
    obs, excl = _lanes(widths)
    window_max = 17 if "window_path_at_17" in mutants else kWindowMaxOb
    out = []
    for l in range(LANES):
        r = (0 if "residue_dropped" in mutants else start & 31) + excl[l]
        left = cnt - 4 * l
        if max_ob <= window_max:
            d = r >> 5
            w2 = 0 if "window_two_dwords" in mutants else stg[d + 2]
            out += _cut4(_window(stg[d], stg[d + 1], w2, r), obs[l], left)
            continue
        for k in range(4):
            ob = obs[l][k]; d = r >> 5
            if lv_bits == 64:
                v64 = _window(stg[d], stg[d + 1], stg[d + 2], r)
                val = v64 if ob >= 64 else v64 & ((1 << ob) - 1)
            else:
                x = _window(stg[d], stg[d + 1], 0, r) & M32
                val = _ubfe(x, ob)
                if ob >= 32 and "bfe_width_mod_32" not in mutants: val = x
            if k < left: out.append(val)
            r += ob
    return out


def general(mem, layout, v, b, mutants=()):
    """unpack_offsets of pco_decode_kernel: per field two safe 64-bit loads from its byte, the second iff sh + ob > 64, masked iff ob < 64."""
    start, widths = item(layout, v, b)
    out = []; bit = start
    for ob in widths:
        val = 0
        if ob != 0:
            byte, sh = bit >> 3, bit & 7
            val = mem.u64_safe(byte) >> sh
            if sh + ob > 64 and "no_second_word" not in mutants: val |= (mem.u64_safe(byte + 8) << (64 - sh)) & M64
            if "mask_at_64" in mutants: val &= (1 << (ob & 63)) - 1          # (a 64-bit shift counts modulo 64)
            elif ob < 64: val &= (1 << ob) - 1
        out.append(val); bit += ob
    return out


def top_bit_share(chunk, layout):
    """Share of the chunk's non-empty offset fields whose top bit is set (a cut one bit short cannot pass where this is high)."""
    n = top = 0
    for b, row in enumerate(layout.batches):
        for v in row:
            for w, x in zip(row[v].widths, true_fields(chunk, layout, v, b)):
                if w: n += 1; top += x >> (w - 1)
    return top / n if n else 1.0
