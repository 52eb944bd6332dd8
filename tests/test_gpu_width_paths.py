"""-m gpu: every decode walk / expander arrangement and every encode walk arrangement, at every number width.

The batched calls pick their kernels from the shape of the call (pco_gfx.hip: the decode width groups and kTrailMinChunks; pco_gfx_encode_api.inc:
the encode walks), and the kernels behind those choices are instantiated per latent width.  Each row below forces one arrangement with the
SHIPPED thresholds (no test switches), proves from the profile / the trail counters that the arrangement really ran, and checks

  * the bytes of every encoded chunk against the oracle (one oracle run per distinct array, its copies spread through the call),
  * every decoded number bit for bit, with a guard byte behind every chunk's numbers,
  * (decode rows) that a chunk cut short in the middle of a walker block fails alone,
  * (E-walkp) that all copies of a chunk are byte-identical wherever they sit, half of them at destinations 8 but not 16 bytes aligned.

If a threshold moves and a row no longer reaches its kernel, the row fails instead of quietly testing something else."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as U
import oracle_lib as O
import pack_layout_model as PM
from pcodec_amd import _lib as G
from test_gpu_parity import O_header_len

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 32, 64)
UINT = {8: np.uint8, 16: np.uint16, 32: np.uint32, 64: np.uint64}
SINT = {8: np.int8, 16: np.int16, 32: np.int32, 64: np.int64}
FLOAT = {16: np.float16, 32: np.float32, 64: np.float64}
NAME = {8: "u8", 16: "u16", 32: "u32", 64: "u64"}
SIZES = [700, 1, 2, 255, 256, 257, 4096, 4097, 3, 513, 1000, 70000]
TRAIL_MIN_CHUNKS = 1024   # pco_gfx.hip kTrailMinChunks: a width group of at least this many chunks decodes with the expanders under the walk
GUARD = 0xAB


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def oracle_chunk(a, kw):
    f = O.simple_compress(a, O.make_config(**kw))
    return f, U.chunk_of_file(f, len(f) - O_header_len(f) - 1)


def ints(x, dt):
    """int64 values -> dt, wrapping like the type's arithmetic."""
    return np.ascontiguousarray(np.asarray(x, np.int64).astype(dt))


# ------------------------------------------------------------------------------------------------ call helpers
def _slots(sizes, align=16, extra=0):
    offs, pos = [], 0
    for s in sizes:
        offs.append(pos); pos += (s + extra + align - 1) // align * align
    return offs, pos


def decode_call(blobs, want, damaged=()):
    """One pco_gfx_decompress_chunks call over `blobs` (one device buffer, 16 readable bytes behind each chunk) into one output buffer filled
    with GUARD.  Checks every chunk: the damaged ones report ST_INSUFFICIENT_DATA, every other one is bit-exact and writes nothing past its
    numbers."""
    import torch
    k = len(blobs)
    s_offs, s_total = _slots([len(b) for b in blobs], extra=16)
    host_src = np.zeros(s_total, np.uint8)
    for o, b in zip(s_offs, blobs):
        host_src[o:o + len(b)] = np.frombuffer(b, np.uint8)
    src = torch.from_numpy(host_src).cuda()
    d_offs, d_total = _slots([a.nbytes for a in want], extra=16)
    out = torch.full((d_total,), GUARD, dtype=torch.uint8, device="cuda")
    tasks = (G.DecodeTask * k)(*[G.DecodeTask(src.data_ptr() + s_offs[i], len(blobs[i]), out.data_ptr() + d_offs[i], want[i].size,
                                              G.DTYPE_BYTE[want[i].dtype.name], 0) for i in range(k)])
    res = (G.TaskResult * k)()
    rc = G.lib().pco_gfx_decompress_chunks(k, tasks, res, None, None)
    assert (rc != 0) == bool(damaged), rc
    host = out.cpu().numpy()
    for i, a in enumerate(want):
        if i in damaged:
            assert res[i].status == G.ST_INSUFFICIENT_DATA, (i, res[i].status)
        else:
            assert res[i].status == 0 and res[i].n_out == a.size and res[i].consumed == len(blobs[i]), (i, a.dtype, a.size, res[i].status, res[i].n_out)
            assert U.bits_equal(host[d_offs[i]:d_offs[i] + a.nbytes].view(a.dtype), a), (i, a.dtype, a.size)
        end = d_offs[i + 1] if i + 1 < k else d_total
        assert (host[d_offs[i] + a.nbytes:end] == GUARD).all(), ("written past the chunk's numbers", i, a.dtype, a.size)


def encode_call(arrays, cfg, misalign=False):
    """One pco_gfx_compress_chunks call over `arrays` (sources and destinations in one device buffer each); with `misalign`, every odd
    chunk's destination lies 8 bytes past a 16-byte boundary.  Returns (chunk bytes, profiled kernel names)."""
    import torch
    L = G.lib()
    k = len(arrays)
    s_offs, s_total = _slots([a.nbytes for a in arrays])
    host_src = np.zeros(s_total, np.uint8)
    for o, a in zip(s_offs, arrays):
        host_src[o:o + a.nbytes] = a.view(np.uint8)
    src = torch.from_numpy(host_src).cuda()
    caps = [L.pco_gfx_guarantee_chunk_size(a.size, G.DTYPE_BYTE[a.dtype.name]) + 64 for a in arrays]
    d_offs, d_total = _slots(caps, extra=16)
    if misalign:
        d_offs = [o + 8 if i % 2 else o for i, o in enumerate(d_offs)]
    comp = torch.zeros(d_total + 16, dtype=torch.uint8, device="cuda")
    tasks = (G.EncodeTask * k)(*[G.EncodeTask(src.data_ptr() + s_offs[i], arrays[i].size, comp.data_ptr() + d_offs[i], caps[i],
                                              G.DTYPE_BYTE[arrays[i].dtype.name], 0) for i in range(k)])
    assert all((t.dst % 16 == 8) == (misalign and i % 2 == 1) for i, t in enumerate(tasks))
    res = (G.TaskResult * k)()
    L.pco_gfx_profile_begin()
    G.check(L.pco_gfx_compress_chunks(k, tasks, C.byref(cfg), res, None, None))
    names = U.profile_names(L)
    host = comp.cpu().numpy()
    for i in range(k):
        assert res[i].status == 0 and 0 < res[i].n_out <= caps[i], (i, res[i].status, res[i].n_out)
    return [host[d_offs[i]:d_offs[i] + res[i].n_out].tobytes() for i in range(k)], names


# ------------------------------------------------------------------------------------------------ decode rows
def one_var(bits, i, n, rng):
    """Classic chunks: candidates of the one-variable expanders (2..64 bins, offsets of <= 16 bits, delta orders 0..2) and chunks they must
    refuse (delta order 3, one bin, more than 64 bins, offsets wider than 16 bits -- only 32 and 64-bit latents have those -- lookback)."""
    dt = (UINT, SINT)[i % 2][bits]
    step, nz, base = {8: (3, 9, 0), 16: (7, 40, 0), 32: (1000, 512, 1 << 30), 64: (1000, 512, 1 << 40)}[bits]
    top = (1 << min(bits, 62)) - 1
    k = i % 10
    if k in (0, 1, 2, 3):   # a noisy ramp: delta orders 0..3 (order 3 is left to dec_expand_kernel)
        x = base + np.arange(n, dtype=np.int64) * step + rng.integers(0, nz, n)
        return ints(x, dt), dict(mode=1, delta=2, delta_order=k) if k else dict(mode=1, delta=1)
    if k == 4: return ints(rng.integers(0, 40, n) * 3 + base, dt), dict(mode=1, delta=1)                        # a few bins, no offsets
    if k == 5: return ints(rng.integers(0, min(top, 4000), n) + base, dt), dict(mode=1, delta=1)              # several bins with offsets
    if k == 6: return ints(rng.integers(0, top, n, dtype=np.int64) if bits < 64 else rng.integers(0, 1 << 62, n), dt), dict(mode=1, delta=1)   # one bin, full width
    if k == 7:   # 200 spikes of unequal weight: more than 64 bins on long chunks
        w = rng.random(200) ** 3
        return ints(rng.choice(200, n, p=w / w.sum()) * (1 if bits == 8 else 300), dt), dict(mode=1, delta=1)
    if k == 8:   # lookback
        per = rng.integers(0, top, 37, dtype=np.int64)
        return ints(per[np.arange(n) % 37] + rng.integers(0, 3, n), dt), dict(mode=1, delta=3)
    if bits >= 32: return ints(rng.integers(0, 1 << (bits - 4), n) * 3, dt), dict(mode=1, delta=1)          # offsets beyond 16 bits
    return ints(np.cumsum(rng.integers(-2, 3, n)) + (1 << (bits - 1)), dt), dict(mode=1, delta=2, delta_order=1)   # a random walk


def two_var(bits, i, n, rng):
    """Two latent variables (dec_trail_kernel<L, true>): int-mult on the integer types of every width, float-mult and float-quant on f16 /
    f32 / f64; secondaries that are one constant bin and secondaries with real content; delta orders 0 and 1 on the primary."""
    k = i % 8
    if bits == 8 or k < 3:   # int-mult
        dt = (UINT, SINT)[i % 2][bits]
        b, hi = {8: (7, 35), 16: (100, 600), 32: (1000, 5000), 64: (1000, 5000)}[bits]
        lo = -(hi // 2) if dt is SINT[bits] else 0
        hi = hi // 2 if dt is SINT[bits] else hi
        kk = k % 3
        if kk == 0: return ints(rng.integers(lo, hi, n) * b, dt), dict(mode=4, mode_u64=b, delta=1)                                  # constant secondary
        if kk == 1: return ints(rng.integers(lo, hi, n) * b + rng.integers(0, 3, n), dt), dict(mode=4, mode_u64=b, delta=1)          # real secondary
        m = np.clip(np.cumsum(rng.integers(-3, 4, n)) + (lo + hi) // 2, lo, hi)
        return ints(m * b, dt), dict(mode=4, mode_u64=b, delta=2, delta_order=1)
    ft = FLOAT[bits]
    with np.errstate(all="ignore"):
        if k == 3:   # float-mult, constant adjustment
            if bits == 16: return (rng.integers(0, 2000, n) * np.float16(0.5)).astype(ft), dict(mode=2, mode_f64=0.5, delta=1)
            if bits == 32: return (rng.integers(10, 4000, n) * 0.25).astype(ft), dict(mode=2, mode_f64=0.25, delta=1)
            return rng.integers(1000, 900000, n) / 100.0, dict(mode=2, mode_f64=0.01, delta=1)
        if k == 4:   # float-mult, real adjustments (a few ulps)
            u = UINT[bits]
            x = (rng.integers(10, 2000, n) * {16: np.float16(0.1), 32: np.float32(0.1), 64: 0.1}[bits]).astype(ft)
            return (x.view(u) + rng.integers(0, 3, n).astype(u)).view(ft), dict(mode=2, mode_f64=0.1, delta=1)
        if k == 5:   # float-mult on a walk, delta order 1
            return ((np.cumsum(rng.integers(-55, 56, n)) + 5000) * {16: 0.25, 32: 0.1, 64: 0.01}[bits]).astype(ft), dict(mode=2, mode_f64={16: 0.25, 32: 0.1, 64: 0.01}[bits], delta=2, delta_order=1)
        q = {16: 5, 32: 20, 64: 45}[bits]
        u = UINT[bits]
        x = (rng.normal(0, 100, n).astype(ft).view(u) & u(~((1 << q) - 1) & ((1 << bits) - 1)))
        if k == 6: return x.view(ft), dict(mode=3, mode_u64=q, delta=1)                                       # float-quant, exact
        noisy = rng.random(n) < 0.2
        return np.where(noisy, x | rng.integers(0, 4, n).astype(u), x).astype(u).view(ft), dict(mode=3, mode_u64=q, delta=1)   # float-quant, real low bits


def trail_kind(f):
    """What the publishing walker's precise test makes of an oracle file's chunk: 0 none, 1 one-variable candidate, 2 two-variable candidate
    whose secondary is certainly not delta'd, 3 two-variable chunk that is one if its secondary is not delta'd (decode_fast.hip)."""
    info, bins = O.inspect_first_chunk(f)
    ob = [int(b[:, 2].max()) if len(b) else 0 for b in bins]
    if info.var_present[0] or info.delta_kind not in (0, 1) or (info.delta_kind == 1 and info.delta_order > 2):
        return 0
    prim = 1 <= info.n_bins[1] <= 64 and ob[1] <= 16
    if not info.var_present[2]:
        return 1 if info.mode_kind == 0 and prim and info.n_bins[1] > 1 else 0
    if info.mode_kind in (1, 2, 3) and prim and 1 <= info.n_bins[2] <= 64 and ob[2] <= 16 and (info.n_bins[1] > 1 or info.n_bins[2] > 1):
        return 2 if info.delta_kind == 0 else 3
    return 0


def decode_set(bits, two, seed):
    """Distinct arrays of one width (oracle files, chunks, trail kinds) for the D-trail (two=False) / D-trail2 (two=True) rows."""
    rng = np.random.default_rng(seed)
    make = two_var if two else one_var
    rows = []
    for i in range(40 if two else 36):
        a, kw = make(bits, i, SIZES[(i * 7) % len(SIZES)], rng)
        f, ch = oracle_chunk(a, dict(kw, enable_8_bit=True))
        rows.append((np.ascontiguousarray(a), kw, ch, trail_kind(f), O.inspect_first_chunk(f)))
    kinds = [r[3] for r in rows]
    assert (1 if not two else 2) in kinds and 0 in kinds, (bits, two, kinds)
    infos = [r[4][0] for r in rows]
    if not two:   # the refusals are really there: one bin, more than 64 bins, (32 / 64 bits) offsets beyond 16 bits
        assert any(x.n_bins[1] == 1 for x in infos) and any(x.n_bins[1] > 64 for x in infos), bits
        if bits >= 32: assert any(r[4][1][1][:, 2].max() > 16 for r in rows if len(r[4][1][1])), bits
    else:        # constant secondaries (one bin, no offset bits) next to real ones
        sec = [(x.n_bins[2], int(r[4][1][2][:, 2].max()) if x.n_bins[2] else 0) for x, r in zip(infos, rows) if x.var_present[2]]
        assert (1, 0) in sec and any(s != (1, 0) for s in sec), (bits, sec)
    # the GPU's own bytes for the same arrays, one small call per config: equal to the oracle's
    by_cfg = {}
    for j, r in enumerate(rows):
        by_cfg.setdefault(tuple(sorted(r[1].items())), []).append(j)
    for key, js in by_cfg.items():
        chunks, _ = encode_call([rows[j][0] for j in js], G.make_config(enable_8_bit=True, **dict(key)))
        for j, c in zip(js, chunks):
            assert c == rows[j][2], (bits, dict(key), rows[j][0].dtype, rows[j][0].size)
    return rows


def expand(rows, count):
    """`count` chunks of the distinct rows: first in runs of sixteen copies (walker blocks and expander waves of one kind: both chunks of a wave
    in the common shape take the straight-line pair path), then round-robin (every kind next to every other, copies in other blocks and slots)."""
    return [rows[(i // 16) % len(rows)] if i < count // 2 else rows[i % len(rows)] for i in range(count)]


def check_trail_decode(L, rows, count, bits):
    calls = expand(rows, count)
    # one chunk cut in half in the middle of a walker block (slot 4 of a block past the first round of blocks)
    dmg = next(i for i in range(8 * 40 + 4, count, 8) if len(calls[i][2]) > 64)
    blobs = [c[2][: len(c[2]) // 2] if i == dmg else c[2] for i, c in enumerate(calls)]
    kinds = [c[3] for c in calls]
    lower = sum(1 for i, (k, b) in enumerate(zip(kinds, blobs)) if k in (1, 2) and len(b) >= 24 and i != dmg)
    upper = sum(1 for k in kinds if k)
    m0, g0 = L.pco_gfx_trail_marked(), L.pco_gfx_trail_givebacks()
    L.pco_gfx_profile_begin()
    decode_call(blobs, [c[0] for c in calls], damaged={dmg})
    names = U.profile_names(L)
    marked, given = L.pco_gfx_trail_marked() - m0, L.pco_gfx_trail_givebacks() - g0
    print(f"{NAME[bits]}: {count} chunks, marked {marked} (candidates {lower}..{upper}), given back {given}")
    assert f"dec_walk+trail<{NAME[bits]}>" in names, names
    assert 0 < lower <= marked <= upper, (bits, marked, lower, upper)


@pytest.mark.parametrize("bits", WIDTHS)
def test_d_trail_one_variable(L, bits):
    """D-trail: 1100+ chunks of one width (u8/i8, u16/i16, u32/i32, u64/i64: dtypes alternate), ragged lengths, delta orders 0..3, classic
    candidates of dec_trail_kernel<L, false> among chunks it must refuse.  The walk + expanders ran (profile, trail_marked covers every
    candidate), all numbers come back, one truncated chunk fails alone.  Offsets wider than 16 bits exist only at 32 and 64 bits."""
    rows = decode_set(bits, False, 100 + bits)
    check_trail_decode(L, rows, 1100 + 3 * bits, bits)


@pytest.mark.parametrize("bits", WIDTHS)
def test_d_trail_two_variables(L, bits):
    """D-trail2: the same for dec_trail_kernel<L, true>: int-mult on every integer type, float-mult and float-quant on f16 / f32 / f64
    (8-bit types have no float, so the u8 group holds only int-mult), constant and real secondaries."""
    rows = decode_set(bits, True, 200 + bits)
    check_trail_decode(L, rows, 1150 + 2 * bits, bits)


@pytest.mark.parametrize("bits", WIDTHS)
def test_d_walk_below_the_trail_threshold(L, bits):
    """D-walk: the D-trail and D-trail2 arrays of a width in one call of fewer than 1024 chunks: dec_walk_kernel, then dec_expand_kernel."""
    rows = decode_set(bits, False, 100 + bits) + decode_set(bits, True, 200 + bits)
    calls = expand(rows, 900)
    assert len(calls) < TRAIL_MIN_CHUNKS
    L.pco_gfx_profile_begin()
    decode_call([c[2] for c in calls], [c[0] for c in calls])
    names = U.profile_names(L)
    assert f"dec_walk_kernel<{NAME[bits]}>" in names and f"dec_walk+trail<{NAME[bits]}>" not in names, names


def test_d_mixed_all_widths_take_the_trail(L):
    """D-mixed: one call with all four width groups at 1024+ chunks each (the ids remapped per group): each group takes the walk + expanders
    in turn, every number comes back."""
    calls = []
    for bits in WIDTHS:
        rows = decode_set(bits, False, 300 + bits) + decode_set(bits, True, 400 + bits)
        calls += expand(rows, TRAIL_MIN_CHUNKS + 16 + bits)
    order = np.random.default_rng(5).permutation(len(calls))   # the groups interleaved in the task array
    calls = [calls[i] for i in order]
    m0 = L.pco_gfx_trail_marked()
    L.pco_gfx_profile_begin()
    decode_call([c[2] for c in calls], [c[0] for c in calls])
    names = U.profile_names(L)
    for bits in WIDTHS:
        assert f"dec_walk+trail<{NAME[bits]}>" in names, (bits, names)
    lower = sum(1 for c in calls if c[3] in (1, 2) and len(c[2]) >= 24)
    assert L.pco_gfx_trail_marked() - m0 >= lower


# ------------------------------------------------------------------------------------------------ encode rows
def worst_bits(f):
    """Most tANS + offset bits one latent of the primary variable can take (the walkp qualification: <= 16)."""
    info, bins = O.inspect_first_chunk(f)
    return PM.worst_bits(info.ans_size_log[1], [tuple(int(x) for x in b) for b in bins[1]])


def walkp_item(f):
    """What enc_walkp_kernel's block test makes of a one-variable chunk, as far as the oracle's ChunkMeta shows it: "trivial", "refuse" or
    "ok" (pack_layout_model.walkp_item, which the pack-edge suites share)."""
    info, bins = O.inspect_first_chunk(f)
    return PM.walkp_item(info.mode_kind, [bool(p) for p in info.var_present], list(info.ans_size_log), [[tuple(int(x) for x in b) for b in v] for v in bins])


def walkp_n(bits, rng):
    # enc_walkp_kernel runs where the value -> bin tables (8 KB per chunk) are within max(64 MB, input / 2): beyond 8192 chunks that is
    # 16 KB of input per chunk, so the narrow types need longer chunks than u64's 2 k - 4 k numbers
    lo = {8: 16500, 16: 8300, 32: 4200, 64: 2100}[bits]
    return int(rng.integers(lo, 2 * lo))


def walkp_set(bits, kw, seed):
    rng = np.random.default_rng(seed)
    u, s = UINT[bits], SINT[bits]
    rows = []
    def add(a, tag):
        rows.append((np.ascontiguousarray(a), tag) + oracle_chunk(a, dict(kw, enable_8_bit=True)))
    for i in range(12):   # narrow: whole walkp blocks (rows 0..11)
        n = walkp_n(bits, rng)
        add(ints(np.cumsum(rng.geometric(0.2, n) % (9 + 4 * i)) + (1 << (bits - 2)), (u, s)[i % 2]), "narrow")   # skewed deltas: several bins
    n = walkp_n(bits, rng)
    add(ints(rng.integers(0, 1 << min(bits, 62), n, dtype=np.int64) if bits < 64 else rng.integers(0, 1 << 62, n), u), "wide")
    add(np.full(walkp_n(bits, rng), 123, u), "constant")
    if bits >= 16:   # latents spanning more than 4096 values (8-bit latents never do)
        add(ints(np.cumsum(rng.integers(0, 5000, walkp_n(bits, rng))), u), "span")
    found = {}
    for t in range(600):   # rare values far from the common ones: a latent of exactly 16 tANS + offset bits (qualifies) and one of 17 (does not)
        if 16 in found and 17 in found: break
        n = walkp_n(bits, rng)
        d = rng.integers(0, int(rng.integers(2, 12)), n)
        m = rng.random(n) < float(rng.choice([0.0005, 0.001, 0.002, 0.005]))
        d[m] = rng.integers(0, int(rng.choice([64, 128, 256] if bits > 8 else [64, 128])), int(m.sum())) + 12
        a = ints(np.cumsum(d), (u, s)[t % 2])
        f, ch = oracle_chunk(a, dict(kw, enable_8_bit=True))
        w = worst_bits(f)
        if w in (16, 17) and w not in found:
            found[w] = 1; rows.append((a, f"bits{w}", f, ch))
    assert 16 in found and 17 in found, (bits, found)
    return rows


@pytest.mark.parametrize("bits", WIDTHS)
def test_e_walkp_beyond_8192_items(L, bits):
    """E-walkp: more than 8192 one-variable chunks of one width (unsigned and signed), each distinct chunk copied many times across walk
    blocks of sixteen.  Blocks of narrow chunks qualify, and so do blocks where one of them is the chunk with a latent of exactly 16 tANS +
    offset bits (the two bytes per latent of the field scratch full); a block with the 17-bit chunk, a wide one (at 8 bits: one bin with
    offset bits, nothing to walk) or, at 16+ bits, one whose latents span more than 4096 values does not; constant chunks write nothing and
    break no block.  What each chunk makes of the block test is checked on the host from the oracle's ChunkMeta (walkp_item), and so is the
    number of qualifying blocks that hold the 16-bit chunk; the device shows only that enc_walkp_kernel and enc_place_kernel were launched
    (and enc_walk16_kernel was not).  Every copy equals the oracle's chunk (so all copies agree), half of them written to destinations 8
    bytes past a 16-byte boundary; all decode back."""
    kw = dict(mode=1, delta=2, delta_order=1)
    rows = walkp_set(bits, kw, 500 + bits)
    tag = {r[1]: j for j, r in enumerate(rows)}
    verdict = [walkp_item(r[2]) for r in rows]
    want = {"narrow": "ok", "bits16": "ok", "bits17": "refuse", "wide": "refuse", "constant": "trivial", "span": "refuse"}
    assert all(verdict[j] == want[r[1]] for j, r in enumerate(rows)), (bits, [(r[1], v) for r, v in zip(rows, verdict)])
    count = 8300
    rng = np.random.default_rng(600 + bits)

    def pick(i):
        if (i // 200) % 2:   # odd runs of 200: every kind round-robin
            return i % len(rows)
        blk = i // 16         # even runs: blocks of narrow chunks, every third with the 16-bit chunk in slot 5, every third with the 17-bit one in slot 9
        if blk % 3 == 1 and i % 16 == 5: return tag["bits16"]
        if blk % 3 == 2 and i % 16 == 9: return tag["bits17"]
        return int(rng.integers(0, 12))
    idx = [pick(i) for i in range(count)]
    blocks = [idx[b:b + 16] for b in range(0, count, 16)]
    n16 = sum(1 for blk in blocks if tag["bits16"] in blk and all(verdict[j] != "refuse" for j in blk))
    assert n16 >= 60, (bits, n16)   # qualifying blocks that pack the full 16-bit latent in enc_walkp_kernel
    arrays = [rows[j][0] for j in idx]
    chunks, names = encode_call(arrays, G.make_config(enable_8_bit=True, **kw), misalign=True)
    assert "enc_walkp_kernel" in names and "~enc_place_kernel" in names and "enc_walk16_kernel" not in names, names
    bad = [(i, rows[j][1], i % 2) for i, j in enumerate(idx) if chunks[i] != rows[j][3]]
    assert not bad, (bits, len(bad), bad[:8])
    decode_call(chunks, arrays)


def walk16_arrays(bits, kw, n_chunks, seed):
    rng = np.random.default_rng(seed)
    mode = kw["mode"]
    out = []
    for i in range(n_chunks):
        n = [1, 2, 255, 256, 257, 300, 511, 513, 1000, 1537][i % 10]
        if mode == 4:
            dt = (UINT, SINT)[i % 2][bits]
            b = kw["mode_u64"]; hi = {8: 16, 16: 300, 32: 5000, 64: 5000}[bits]
            lo = -hi if dt is SINT[bits] else 0
            out.append(ints(rng.integers(lo, hi, n) * b + (rng.integers(0, 3, n) if i % 3 else 0), dt))
        elif mode == 2:
            x = (rng.integers(10, 2000, n) * kw["mode_f64"]).astype(FLOAT[bits])
            if i % 3 == 0:
                x = (x.view(UINT[bits]) + rng.integers(0, 2, n).astype(UINT[bits])).view(FLOAT[bits])
            out.append(np.ascontiguousarray(x))
        else:
            q = kw["mode_u64"]; u = UINT[bits]
            with np.errstate(all="ignore"):
                x = rng.normal(0, 100, n).astype(FLOAT[bits]).view(u) & u(~((1 << q) - 1) & ((1 << bits) - 1))
            if i % 3 == 0:
                x = x | rng.integers(0, 3, n).astype(u)
            out.append(np.ascontiguousarray(x.view(FLOAT[bits])))
    return out


WALK16 = [(8, dict(mode=4, mode_u64=7, delta=1)), (16, dict(mode=4, mode_u64=100, delta=2, delta_order=1)), (16, dict(mode=2, mode_f64=0.5, delta=1)),
          (16, dict(mode=3, mode_u64=5, delta=1)), (32, dict(mode=4, mode_u64=1000, delta=1)), (32, dict(mode=2, mode_f64=0.25, delta=2, delta_order=1)),
          (32, dict(mode=3, mode_u64=20, delta=1)), (64, dict(mode=4, mode_u64=1000, delta=2, delta_order=1)), (64, dict(mode=2, mode_f64=0.01, delta=1)),
          (64, dict(mode=3, mode_u64=45, delta=1))]


MODE_NAME = {2: "fmult", 3: "fquant", 4: "imult"}


@pytest.mark.parametrize("bits,kw", WALK16, ids=[NAME[b] + "-" + MODE_NAME[k["mode"]] for b, k in WALK16])
def test_e_walk16_two_variable_launches(L, bits, kw):
    """E-walk16: more than 8192 two-variable items (4200 chunks of two variables) of one width: int-mult at every width (u8/i8 and 16-bit
    included), float-mult and float-quant on f16 / f32 / f64.  enc_walk16_kernel ran; the chunks equal the oracle's on a spread that covers
    every length and kind, and all decode back."""
    count = 4200
    arrays = walk16_arrays(bits, kw, count, 700 + bits + kw["mode"])
    chunks, names = encode_call(arrays, G.make_config(enable_8_bit=True, **kw))
    assert "enc_walk16_kernel" in names, names
    for i in list(range(0, count, 53)) + list(range(count - 60, count)):
        _, want = oracle_chunk(arrays[i], dict(kw, enable_8_bit=True))
        assert chunks[i] == want, (bits, kw, i, arrays[i].dtype, arrays[i].size)
    decode_call(chunks, arrays)


@pytest.mark.parametrize("bits", [8, 64])
def test_e_walkseg_long_pages(L, bits):
    """E-seg: a few long pages (>= 16 384 numbers, <= 4096 items) at 8 and 64 bits, batched: enc_walkseg_kernel ran, with tables that forget
    their state at once, slowly, and never (16 and 32 bits: test_segmented_encode_walk_never_depends_on_luck)."""
    rng = np.random.default_rng(31 + bits)
    u = UINT[bits]
    arrays = []
    for n in (16384, 16385, 20000, 65536 + 255, 1 << 18):
        arrays.append(rng.integers(0, 4, n).astype(u))                                      # four equal bins: never forgets
        arrays.append((rng.integers(0, 2, n) * 100).astype(u))                              # two equal bins
        arrays.append(np.where(rng.random(n) < 0.999, 5, 77).astype(SINT[bits]))            # one heavy bin: forgets slowly
        arrays.append((rng.geometric(0.3, n) % 16).astype(u))
        arrays.append(ints(rng.integers(0, 256 if bits == 8 else 1 << 20, n), u))         # many bins: forgets at once
    for kw in (dict(mode=1, delta=1), dict(mode=1, delta=2, delta_order=1)):
        chunks, names = encode_call(arrays, G.make_config(enable_8_bit=True, **kw))
        assert "enc_walkseg_kernel" in names, names
        for a, c in zip(arrays, chunks):
            assert c == oracle_chunk(a, dict(kw, enable_8_bit=True))[1], (bits, kw, a.dtype, a.size)
        decode_call(chunks, arrays)
