"""-m gpu: the decoders' offset readers at their width and section edges (the rows of offset_edges_util.py; what each row covers is certified
on the CPU by test_offset_reader_model.py).

Every call goes through ONE helper, decode(): all chunks in one source buffer filled with 0xff, exactly 16 bytes between consecutive
chunks -- so a reader that consumed bits of the slack would read ones, not the zeros every other decode test leaves there, and a read past
the slack lands in the next chunk --, all destinations in one buffer filled with a guard byte.  It asserts status 0, n_out and consumed of
every task, every number bit for bit, and every guard byte between the destinations.

  (a) pairs: at least kTrailMinChunks chunks of one width, every trail candidate in slots 2v and 2v + 1 of its walker block (the two chunks of
      one expander wave: the straight-line bodies are open to it), destinations on 16-byte boundaries.  The walk + expanders span ran, the
      walker marked exactly the predicted chunks, and none was given back.  WHICH body took a given batch depends on how far the walker was
      ahead at that moment and is not asserted.
  (b) the same chunks with every destination one element past a 16-byte boundary: no fast flag is set (decode_trail.hip: `aligned`), so the
      general bodies and their scalar store branches take every batch, deterministically.
  (c) odd neighbours: each candidate shares its wave with a chunk that keeps the pair off the straight-line bodies (k = 8 beside k = 7) or
      leaves it half way (a 70-number chunk beside a 1500-number one: the longer chunk goes from the lockstep body to the general one).
  (d) every row of the width in one call below kTrailMinChunks: dec_expand_kernel, dec_expand_lb_kernel and pco_decode_kernel, no trail span.
  (e) the k = 16 and k = 64 rows as wrapped pages, a row range that starts in the last batch (the kRange instantiation of the same reader),
      through test_gpu_page_ranges.run_ranges."""
import time

import numpy as np
import pytest

import gpu_util as U
import offset_edges_util as E
import oracle_lib as O
from pcodec_amd import _lib as G

pytestmark = pytest.mark.gpu

GUARD = 0xAB
FILL = 0xFF
NAME = {8: "u8", 16: "u16", 32: "u32", 64: "u64"}


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


def decode(L, bs, dst_shift_elems=0):
    """One synchronous pco_gfx_decompress_chunks call over the chunks of `bs` ([Built], repeats allowed).  Returns (kernel names of the
    profile, trail_marked delta, trail_givebacks delta, seconds of the call)."""
    import torch
    k = len(bs)
    s_offs, at = [], 0
    for b in bs:
        s_offs.append(at); at += len(b.chunk) + 16           # exactly 16 bytes between consecutive chunks
    host_src = np.full(at, FILL, np.uint8)
    for o, b in zip(s_offs, bs):
        host_src[o:o + len(b.chunk)] = np.frombuffer(b.chunk, np.uint8)
    src = torch.from_numpy(host_src).cuda()
    d_offs, at = [], 0
    for b in bs:
        a = b.row.array
        at = (at + 15) // 16 * 16 + 16 + dst_shift_elems * a.itemsize    # (at least 16 guard bytes in front of every destination)
        d_offs.append(at); at += a.nbytes
    total = at + 32
    out = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    tasks = (G.DecodeTask * k)(*[G.DecodeTask(src.data_ptr() + s_offs[i], len(b.chunk), out.data_ptr() + d_offs[i], b.row.array.size,
                                              G.DTYPE_BYTE[b.row.array.dtype.name], 0) for i, b in enumerate(bs)])
    assert all(t.dst % 16 == dst_shift_elems * b.row.array.itemsize for t, b in zip(tasks, bs))
    res = (G.TaskResult * k)()
    m0, g0 = L.pco_gfx_trail_marked(), L.pco_gfx_trail_givebacks()
    L.pco_gfx_profile_begin()
    t0 = time.perf_counter()
    rc = L.pco_gfx_decompress_chunks(k, tasks, res, None, None)
    dt = time.perf_counter() - t0
    names = U.profile_names(L)
    marked, given = L.pco_gfx_trail_marked() - m0, L.pco_gfx_trail_givebacks() - g0
    host = out.cpu().numpy()
    mask = np.ones(total, bool)
    bad = []
    for i, b in enumerate(bs):
        a = b.row.array
        if not (res[i].status == 0 and res[i].n_out == a.size and res[i].consumed == len(b.chunk)):
            bad.append(f"task {i} [{b.row.label}]: status {res[i].status}, n_out {res[i].n_out} of {a.size}, consumed {res[i].consumed} of {len(b.chunk)}")
            continue
        got = host[d_offs[i]:d_offs[i] + a.nbytes].view(a.dtype)
        if not U.bits_equal(got, a):
            u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize]
            d = np.flatnonzero(got.view(u) != a.view(u))
            bad.append(f"task {i} [{b.row.label}]: {d.size} of {a.size} numbers differ, the first at {int(d[0])} (batch {int(d[0]) // 256}, lane {int(d[0]) % 256 // 4}): "
                       f"{int(got.view(u)[d[0]]):#x} for {int(a.view(u)[d[0]]):#x}")
        mask[d_offs[i]:d_offs[i] + a.nbytes] = False
    once = list({m.split("]: ")[0].split(" [")[1]: m for m in bad}.values())   # (a row repeated round-robin fails alike: each row once)
    assert rc == 0 and not bad, f"rc {rc}\n" + "\n".join(once[:60]) + f"\n({len(bad)} tasks of {len(once)} rows in all)"
    assert (host[mask] == GUARD).all(), ("guard bytes between the destinations were written", np.flatnonzero(mask & (host != GUARD))[:8])
    return names, marked, given, dt


def candidates(width):
    return [b for b in E.built(width) if E.path(b.layout) in ("trail1", "trail2")]


def fill_to(seq, count):
    return [seq[i % len(seq)] for i in range(max(count, len(seq)))]


def predicted_marks(bs, width):
    """The chunks the publishing walker marks for the expanders: by the rows' own prediction (offset_edges_util.path) and by the suite's
    older one (test_gpu_foreign_tables.expander_kind, from the oracle's reading of the ChunkMeta) -- the two must agree."""
    from test_gpu_foreign_tables import expander_kind
    mine = [E.path(b.layout) in ("trail1", "trail2") for b in bs]
    kinds = {id(b): expander_kind(b.file, width) for b in {id(b): b for b in bs}.values()}
    theirs = [kinds[id(b)] != 0 and len(b.chunk) >= 24 for b in bs]
    assert mine == theirs, [b.row.label for b, x, y in zip(bs, mine, theirs) if x != y][:8]
    return sum(mine)


def check_trail(L, bs, width, shift, what):
    want = predicted_marks(bs, width)
    assert len(bs) >= E.kTrailMinChunks and want > 0
    names, marked, given, dt = decode(L, bs, shift)
    print(f"{NAME[width]} {what}: {len(bs)} chunks, {sum(len(b.chunk) for b in bs)} bytes, marked {marked} (predicted {want}), given back {given}, {dt * 1e3:.1f} ms")
    assert f"dec_walk+trail<{NAME[width]}>" in names, names
    assert marked == want, (marked, want)
    assert given == 0, f"{given} chunks the expanders should have finished were given back to dec_expand_kernel"


@pytest.mark.parametrize("width", E.WIDTHS)
def test_a_pairs_on_aligned_destinations(L, width):
    c = candidates(width)
    pairs = [b for b in c for _ in range(2)]                       # slots 2v and 2v + 1: one expander wave
    check_trail(L, fill_to(pairs, E.kTrailMinChunks + 2 * width), width, 0, "(a) pairs")


@pytest.mark.parametrize("width", E.WIDTHS)
def test_b_destinations_one_element_past_a_16_byte_boundary(L, width):
    c = candidates(width)
    pairs = [b for b in c for _ in range(2)]
    check_trail(L, fill_to(pairs, E.kTrailMinChunks + 2 * width), width, 1, "(b) unaligned")


@pytest.mark.parametrize("width", E.WIDTHS)
def test_c_odd_neighbours(L, width):
    c = [b for b in candidates(width) if E.path(b.layout) == "trail1"]
    k7 = [b for b in c if E.exact(b, 1, 7) and b.group == "res"]; k8 = [b for b in c if E.exact(b, 1, 8) and b.group == "res"]
    short = [b for b in c if b.row.array.size == 70]; long_ = [b for b in c if b.row.array.size > 1500]
    assert k7 and k8 and short and long_
    seq = []
    for i, b in enumerate(c):   # every candidate beside a neighbour of the other kind, on either side of the wave
        if E.exact(b, 1, 7): other = k8[i % len(k8)]                    # in kFlFast beside a chunk that is not
        elif b.row.array.size > 1500: other = short[i % len(short)]     # a long chunk whose neighbour ends after a batch or two
        else: other = k7[i % len(k7)] if not E.exact(b, 1, 8) or i % 2 else long_[i % len(long_)]
        seq += [b, other] if i % 2 else [other, b]
    check_trail(L, fill_to(seq, E.kTrailMinChunks + 2 * width), width, 0, "(c) odd neighbours")
    two = [b for b in candidates(width) if E.path(b.layout) == "trail2"]
    seq = []
    for i, b in enumerate(two):   # two-variable chunks: every row beside the next one (constant beside real secondaries, 15 beside 16 bits)
        seq += [b, two[(i + 1) % len(two)]]
    check_trail(L, fill_to(seq, E.kTrailMinChunks + 2 * width), width, 0, "(c) odd neighbours, two variables")


@pytest.mark.parametrize("width", E.WIDTHS)
def test_d_every_row_in_a_small_call(L, width):
    bs = list(E.built(width))
    assert len(bs) < E.kTrailMinChunks
    paths = {E.path(b.layout) for b in bs}
    assert {"trail1", "trail2", "expand", "expand_lb", "general"} <= paths, paths
    for shift in (0, 1):
        names, marked, given, dt = decode(L, bs, shift)
        print(f"{NAME[width]} (d) small call, destinations + {shift}: {len(bs)} chunks, {sum(len(b.chunk) for b in bs)} bytes, {dt * 1e3:.1f} ms")
        w = NAME[width]
        assert {f"dec_walk_kernel<{w}>", f"dec_expand_kernel<{w}>", f"dec_expand_lb_kernel<{w}>", f"pco_decode_kernel<{w}>"} <= set(names), names
        assert f"dec_walk+trail<{w}>" not in names and marked == 0 and given == 0, (names, marked, given)


@pytest.mark.parametrize("width", [w for w in E.WIDTHS if w >= 16])
def test_e_row_ranges_that_start_in_the_last_batch(L, width):
    """The k = 16 and k = 64 rows as one wrapped page each (test_encode(pages=...)); a range that starts in the page's last batch and one
    that starts in the batch before it, through the range decoder's instantiation of expand_item."""
    from test_gpu_page_ranges import Stream, check_ok, run_ranges
    ks = [k for k in (16, 64) if k <= width]
    rows = [b for b in E.built(width) if b.group in ("res", "last", "nd", "wide", "2048") and any(E.exact(b, 1, k) for k in ks)]
    assert {k for k in ks for b in rows if E.exact(b, 1, k)} == set(ks)
    jobs = []
    for b in rows:
        x = b.row.array
        meta, pages = O.test_encode(x, pages=[x.size], **b.row.kw)
        s = Stream(b.row.label, x, meta, pages[0])
        last = (x.size - 1) // 256 * 256
        firsts = {last, min(last + 3, x.size - 1), max(last - 200, 0)}
        for first in sorted(firsts):
            jobs.append((s, None, first, x.size - first))
    code, rec, got = run_ranges(L, jobs)
    assert code == 0
    check_ok(jobs, rec, got, f"u{width}")
