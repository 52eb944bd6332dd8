"""-m gpu: pco_gfx_decompress_pages_dir / pco_gfx_decompress_page_ranges_dir (include/pco_gfx.h section 4e) -- pages and row ranges decoded
from a page directory that lies in DEVICE memory, behind pco_gfx_compact_wrapped_chunks.

Truth is the input array (the writer's bytes are pinned to the oracle in test_gpu_wrapped_writer.py).  Every dst lies between canary bytes and
the whole output area is compared, so a refused task that wrote a byte, or a decoded one that wrote one too many, fails.  The host task array
and the PcoGfxDirectory are overwritten with VALID decoys (another output area; a directory whose chunks all read "dropped") as soon as each call
returns: a library that read them later would decode elsewhere or answer PCO_GFX_INSUFFICIENT_DATA.

Two things differ from the letter of the plan, because the encoder's argument checks do not allow them: float-mult is refused for integers, so
the float-mult rows hold f64 / f32 / f16 chunks beside the Classic rows' u64 / f32 / i16 / u8; and a dst_cap below pco_gfx_wrapped_chunk_cap is
refused before anything is launched, so the dropped chunk comes from a hand-edited copy of d_infos, as in
test_gpu_wrapped_writer.py::test_a_chunk_with_a_failed_piece_drops_whole.

Measured on an MI355X: the module takes 12 s (76 passed, no call above 0.7 s); the -m gpu suite takes 163 s with it (702 passed) and
154 s without it (626 passed).  Which rows four mutations of the resolve step fail is recorded in DESIGN.md section 2."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gpu_util as U  # noqa: E402
from pcodec_amd import _lib as G  # noqa: E402
from pcodec_amd import paged  # noqa: E402
from pcodec_amd.config import ChunkConfig  # noqa: E402
from test_gpu_wrapped_writer import Call, handle  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY, PAD, ALL_ONES = 0xA5, 64, (1 << 64) - 1
DIRPAGE_DT = np.dtype([("dst", "<u8"), ("page_n", "<u8"), ("meta_piece", "<u4"), ("page_piece", "<u4"), ("dtype", "<u4"), ("format_major", "<u4")])
DIRRANGE_DT = np.dtype([("dst", "<u8"), ("page_n", "<u8"), ("first", "<u8"), ("count", "<u8"), ("meta_piece", "<u4"), ("page_piece", "<u4"),
                        ("dtype", "<u4"), ("format_major", "<u4")])
RANGE_DT = np.dtype([("meta", "<u8"), ("meta_len", "<u8"), ("page", "<u8"), ("page_len", "<u8"), ("dst", "<u8"), ("page_n", "<u8"), ("first", "<u8"),
                     ("count", "<u8"), ("dtype", "<u4"), ("format_major", "<u4")])
assert DIRPAGE_DT.itemsize == 32 and DIRRANGE_DT.itemsize == 48 and RANGE_DT.itemsize == 72
EXACT, MAX_PAGE_N, N = [2049, 1111, 1448], 1537, 4608


@pytest.fixture(scope="module")
def L():
    lib = G.lib()
    assert lib.pco_gfx_device_count() >= 1, "these tests need an MI355X; the product has no CPU path"
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs: one encoded call per spec, written once; one compacted blob per (spec, gap)
# ---------------------------------------------------------------------------------------------------------------------------------------
SPECS = {
    "classic": dict(mode=1, delta=1), "classic+consecutive1": dict(mode=1, delta=2, delta_order=1), "classic+consecutive2": dict(mode=1, delta=2, delta_order=2),
    "classic+lookback": dict(mode=1, delta=3),
    "floatmult": dict(mode=2, mode_f64=0.01, delta=1), "floatmult+consecutive1": dict(mode=2, mode_f64=0.01, delta=2, delta_order=1),
    "floatmult+lookback": dict(mode=2, mode_f64=0.01, delta=3),
    "level12": dict(mode=1, delta=1, level=12),
}


def arrays_of(spec):
    rng = np.random.default_rng(sorted(SPECS).index(spec) + 100)
    cents = lambda n: rng.integers(1000, 10000, n) / 100.0   # noqa: E731
    if spec == "level12":   # 3000 distinct u16 values, six pages of 4608: more bins than the walkers' tables hold -- the general kernel and its table scratch
        distinct = rng.permutation(1 << 16)[:3000].astype(np.uint16)   # (in ONE page of 4608 a bin per value does not pay, and the writer keeps one bin)
        a = np.concatenate([distinct, distinct[rng.integers(0, 3000, 6 * N - 3000)]])
        return [a[rng.permutation(6 * N)]], [None]
    if spec.startswith("floatmult"):
        return [cents(N), cents(N).astype(np.float32), (rng.integers(0, 2000, N) / 100.0).astype(np.float16), cents(N)], [EXACT, None, EXACT, None]
    walk = np.cumsum(rng.integers(-5, 6, N))
    return [U.synth("c2", N, seed=5), cents(N).astype(np.float32), walk.astype(np.int16), rng.integers(0, 255, N).astype(np.uint8), U.synth("c4", N, seed=6)], [EXACT, None, EXACT, None, None]


_calls, _blobs = {}, {}


def encoded(L, spec):
    if spec not in _calls:
        arrays, lists = arrays_of(spec)
        c = Call(L, arrays, G.make_config(max_page_n=N if spec == "level12" else MAX_PAGE_N, enable_8_bit=True, **SPECS[spec]), lists)
        G.check(c.encode())
        assert (c.infos["status"] == 0).all() and [len(p) for p in c.pages] == ([6] if spec == "level12" else [3] * c.k)
        if spec == "level12":   # a bin of a u16 variable takes at most 12 + 16 + 5 bits of the ChunkMeta: more than 256 bins, beyond the walkers
            assert int(c.infos["len"][0]) * 8 > 256 * 33 + 64, c.infos["len"][0]
        _calls[spec] = c
    return _calls[spec]


class Blob:
    """The pieces of an encoded Call, compacted with `gap` canary bytes in front of each; blob_len is the stream's end, 64 more bytes are readable."""

    def __init__(self, c, gap, d_infos=None, infos=None, stream=None, cap=None):
        import torch
        self.c, self.gap = c, gap
        infos = c.infos if infos is None else infos
        self.cap = int((infos["len"] + gap).sum()) if cap is None else cap
        self.blob = torch.full((self.cap + 64,), 0xC3, dtype=torch.uint8, device="cuda")
        self.offs = torch.full((c.n_pieces + 1,), 0x1111111111111111, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        G.check(c.L.pco_gfx_compact_wrapped_chunks(c.k, c.tasks, C.addressof(c.cfg), (d_infos if d_infos is not None else c.d_infos).data_ptr(), gap, self.blob.data_ptr(),
                                                   self.cap, 0, self.offs.data_ptr(), None, handle(stream)))

    def directory(self, offs=None, blob_len=None):
        return G.Directory(self.blob.data_ptr(), self.cap if blob_len is None else blob_len, (self.offs if offs is None else offs).data_ptr(), self.c.n_pieces, self.gap, 0)


def blob_of(L, spec, gap):
    if (spec, gap) not in _blobs:
        _blobs[spec, gap] = Blob(encoded(L, spec), gap)
    return _blobs[spec, gap]


def all_pages(c):
    return [(i, p, 0, n) for i in range(c.k) for p, n in enumerate(c.pages[i])]


def reaches_the_end(first, count, page_n):
    return ((first + count + 255) // 256) * 256 >= page_n


class Job:
    """Tasks `want` = [(chunk, page, first, count)] over the pieces of Call `c`: their dsts side by side in one canary-filled device area, PAD canary
    bytes around each; `image` is what the area must hold when every task decodes."""

    def __init__(self, c, want, ranges, out=None):
        import torch
        self.c, self.want, self.ranges = c, want, ranges
        self.at = []; at = PAD
        for i, _, _, n in want:
            self.at.append(at); at += (n * c.arrays[i].dtype.itemsize + 15) // 16 * 16 + PAD
        self.size = at
        self.image = np.full(self.size, CANARY, np.uint8)
        self.spans = []
        for (i, p, f, n), o in zip(want, self.at):
            a = c.arrays[i]; r0 = sum(c.pages[i][:p]) + f
            b = a[r0: r0 + n].view(np.uint8).reshape(-1)
            self.image[o: o + b.size] = b; self.spans.append((o, b.size))
        self.out = out if out is not None else torch.full((self.size,), CANARY, dtype=torch.uint8, device="cuda")
        self.decoy_out = torch.full((self.size,), CANARY, dtype=torch.uint8, device="cuda")
        self.decoy_offs = torch.zeros(c.n_pieces + 1, dtype=torch.int64, device="cuda")   # a directory whose chunks all read "dropped"
        self.d_res = torch.full((max(len(want), 1) * U.RES_DT.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
        self.res = np.zeros(len(want), U.RES_DT); self.res["status"] = 99; self.res["n_out"] = 77
        torch.cuda.synchronize()

    def records(self, out):
        c = self.c
        t = np.zeros(len(self.want), DIRRANGE_DT if self.ranges else DIRPAGE_DT)
        for j, ((i, p, f, n), o) in enumerate(zip(self.want, self.at)):
            t[j]["dst"] = out.data_ptr() + o; t[j]["page_n"] = c.pages[i][p]
            t[j]["meta_piece"] = int(c.piece_first[i]); t[j]["page_piece"] = int(c.piece_first[i]) + 1 + p
            t[j]["dtype"] = c.dtb[i]; t[j]["format_major"] = 4
            if self.ranges:
                t[j]["first"] = f; t[j]["count"] = n
        return t

    def launch(self, directory, form, stream=None):
        """One call; the task array and the directory are decoys by the time this returns."""
        t = self.records(self.out); d = directory
        fn = self.c.L.pco_gfx_decompress_page_ranges_dir if self.ranges else self.c.L.pco_gfx_decompress_pages_dir
        code = fn(len(t), U.ptr(t), C.addressof(d), U.ptr(self.res) if form == "sync" else None, self.d_res.data_ptr(), handle(stream))
        status = self.c.L.pco_gfx_last_status()
        t[:] = self.records(self.decoy_out)
        C.memmove(C.addressof(d), C.addressof(G.Directory(d.d_blob, d.blob_len, self.decoy_offs.data_ptr(), d.n_pieces, d.gap, 0)), C.sizeof(G.Directory))
        del t, d; gc.collect()
        return code, status

    def check(self, infos, code, status, form, failing=None, out=None, d_res=None):
        """failing: {task index: status}.  Results, outputs and canaries of every task, the call's return code in the synchronous form."""
        import torch
        failing = failing or {}
        torch.cuda.synchronize()
        dev = (self.d_res if d_res is None else d_res).cpu().numpy().view(U.RES_DT)[: len(self.want)]
        recs = [("device", dev)] + ([("host", self.res)] if form == "sync" else [])
        for name, rec in recs:
            for j, (i, p, f, n) in enumerate(self.want):
                page_n = self.c.pages[i][p]; plen = int(infos["len"][int(self.c.piece_first[i]) + 1 + p])
                if j in failing:
                    wanted = (failing[j], 0, 0, 0)
                else:
                    wanted = (0, n, plen if (n and reaches_the_end(f, n, page_n)) else 0, 0)
                got = (int(rec["status"][j]), int(rec["n_out"][j]), int(rec["consumed"][j]), int(rec["aux"][j]))
                assert got == wanted, f"{name} result of task {j} {self.want[j]}: (status, n_out, consumed, aux) = {got}, expected {wanted}"
        if form == "sync":
            first = min(failing) if failing else None
            assert (code, status) == ((G.PcoSuccess, 0) if first is None else (G.PcoDecompressionError, failing[first])), (code, status)
        else:
            assert code == G.PcoSuccess
        image = self.image.copy()
        for j in failing:
            o, nb = self.spans[j]; image[o: o + nb] = CANARY
        host = (self.out if out is None else out).cpu().numpy()
        if not np.array_equal(host, image):
            bad = np.flatnonzero(host != image)
            j = int(np.searchsorted(self.at, int(bad[0]), side="right")) - 1
            raise AssertionError(f"{bad.size} bytes of the output area differ, first at {int(bad[0])} (task {j} {self.want[max(j, 0)]} starts at {self.at[max(j, 0)]})")
        assert (self.decoy_out.cpu().numpy() == CANARY).all(), "the decoy tasks were decoded: the task array was read after the call returned"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. whole pages, both forms
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("spec", sorted(SPECS))
def test_whole_pages_of_a_mixed_call(L, spec, gap, form):
    b = blob_of(L, spec, gap); c = b.c
    job = Job(c, all_pages(c), ranges=False)
    code, status = job.launch(b.directory(), form)
    job.check(c.infos, code, status, form)


def test_the_trailing_expanders(L):
    """1024 and 1032 one-variable u64 pages of 512 numbers in one width group (kTrailMinChunks), asynchronous.  Four clusters of 16 values: four
    bins (a page of one bin has nothing to walk and is no candidate for the expanders)."""
    centres = np.array([1 << 40, 1 << 41, 1 << 42, 1 << 43], np.uint64)
    dist = [centres[np.random.default_rng(s).integers(0, 4, 512)] + np.random.default_rng(s + 9).integers(0, 16, 512).astype(np.uint64) for s in range(4)]
    for k in (1024, 1032):
        c = Call(L, U.tile(dist, k), G.make_config(**SPECS["classic"]))
        G.check(c.encode())
        assert (c.infos["len"][0::2] >= 20).all(), "a ChunkMeta this short holds one bin"
        b = Blob(c, 4)
        job = Job(c, all_pages(c), ranges=False)
        before = L.pco_gfx_trail_marked()
        code, status = job.launch(b.directory(), "async")
        job.check(c.infos, code, status, "async")
        assert L.pco_gfx_trail_marked() > before, "no chunk was marked for the trailing expanders"


@pytest.mark.parametrize("gap", [0, 4])
def test_pages_of_zero_bytes(L, gap):
    """A constant uint32 chunk under Classic without delta: pages of 0 bytes beside a ChunkMeta of a few.  The dropped-chunk rule is the ChunkMeta's."""
    rng = np.random.default_rng(9)
    const = lambda v: np.full(3000, v, np.uint32)   # noqa: E731
    arrays = [U.synth("c2", 1500, seed=1), const(7), rng.normal(size=1200).astype(np.float32), const(0xDEADBEEF), const(0), np.cumsum(rng.integers(-5, 6, 900)).astype(np.int16)]
    c = Call(L, arrays, G.make_config(**SPECS["classic"]), [None, [1000, 1000, 1000], None, [1000, 1000, 1000], [1, 2998, 1], None])
    G.check(c.encode())
    for i in (1, 3, 4):
        k0 = int(c.piece_first[i])
        assert c.infos["len"][k0] > 0 and (c.infos["len"][k0 + 1: k0 + 4] == 0).all(), c.infos["len"][k0: k0 + 4]
    b = Blob(c, gap)
    for form in ("sync", "async"):
        job = Job(c, all_pages(c), ranges=False)
        code, status = job.launch(b.directory(), form)
        job.check(c.infos, code, status, form)
    want = [(i, p, f, n) for i in (0, 1, 3, 4) for p in range(len(c.pages[i])) for f, n in ((0, 1), (0, c.pages[i][p]), (c.pages[i][p] - 1, 1))]
    for form in ("sync", "async"):
        job = Job(c, want, ranges=True)
        code, status = job.launch(b.directory(), form)
        job.check(c.infos, code, status, form)


@pytest.mark.parametrize("gap", [0, 4])
def test_a_dropped_chunk(L, gap):
    """Chunk 2's first page carries a failure status in a hand-edited COPY of d_infos: the compactor drops the chunk whole, its tasks answer
    PCO_GFX_INSUFFICIENT_DATA with their canaries intact, every other chunk decodes."""
    import torch
    c = encoded(L, "classic+consecutive1")
    infos = c.infos.copy(); infos["status"][int(c.piece_first[2]) + 1] = G.ST_INVALID_ARGUMENT
    kept = infos.copy(); kept["len"][int(c.piece_first[2]): int(c.piece_first[3])] = 0   # (what the stream holds: for the blob's size)
    b = Blob(c, gap, d_infos=torch.from_numpy(infos.view(np.uint8).copy()).cuda(), infos=kept, cap=int((kept["len"] + gap).sum()) - gap * 4)
    offs = b.offs.cpu().numpy().view(np.uint64)
    assert len(set(offs[int(c.piece_first[2]): int(c.piece_first[3]) + 1].tolist())) == 1 and int(offs[-1]) == b.cap
    want = all_pages(c)
    failing = {j: G.ST_INSUFFICIENT_DATA for j, w in enumerate(want) if w[0] == 2}
    for ranges in (False, True):
        for form in ("sync", "async"):
            job = Job(c, want, ranges=ranges)
            code, status = job.launch(b.directory(), form)
            job.check(c.infos, code, status, form, failing)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. directory defects, each injected into a device COPY of d_offsets
# ---------------------------------------------------------------------------------------------------------------------------------------
def edited(b, edit):
    import torch
    offs = b.offs.cpu().numpy().view(np.uint64).copy()
    edit(offs)
    return torch.from_numpy(offs.view(np.int64)).cuda()


@pytest.mark.parametrize("ranges", [False, True], ids=["pages", "ranges"])
@pytest.mark.parametrize("form", ["sync", "async"])
def test_the_sentinel_refuses_every_task(L, form, ranges):
    b = blob_of(L, "classic+consecutive1", 4); c = b.c; n = c.n_pieces

    def edit(o): o[n] = ALL_ONES
    job = Job(c, all_pages(c), ranges=ranges)
    code, status = job.launch(b.directory(offs=edited(b, edit)), form)
    job.check(c.infos, code, status, form, {j: G.ST_INVALID_ARGUMENT for j in range(len(job.want))})


@pytest.mark.parametrize("ranges", [False, True], ids=["pages", "ranges"])
@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("defect", ["swapped pair", "end beyond blob_len", "extent of gap - 1"])
def test_a_defect_fails_the_named_tasks_alone(L, defect, form, ranges):
    """Each edit touches the LAST piece's entries (the last page of the last chunk): every other piece keeps its start and an end inside the blob."""
    b = blob_of(L, "classic+consecutive1", 4); c = b.c; n = c.n_pieces

    def edit(o):
        if defect == "swapped pair":
            o[n - 1], o[n] = o[n], o[n - 1]
        elif defect == "end beyond blob_len":
            o[n] = b.cap + 1   # (the blob has 64 readable bytes behind its end)
        else:
            o[n] = int(o[n - 1]) + 3
    want = all_pages(c)
    failing = {j: G.ST_INVALID_ARGUMENT for j, (i, p, _, _) in enumerate(want) if int(c.piece_first[i]) + 1 + p == n - 1}
    assert len(failing) == 1
    job = Job(c, want, ranges=ranges)
    code, status = job.launch(b.directory(offs=edited(b, edit)), form)
    job.check(c.infos, code, status, form, failing)


def test_a_defect_in_a_chunk_meta_fails_all_its_pages(L):
    b = blob_of(L, "classic", 4); c = b.c; k = int(c.piece_first[1])

    def edit(o): o[k + 1] = int(o[k]) + 3   # the ChunkMeta's extent is gap - 1 (its page 0 starts earlier then: it fails with its chunk anyway)
    want = all_pages(c)
    job = Job(c, want, ranges=False)
    code, status = job.launch(b.directory(offs=edited(b, edit)), "async")
    job.check(c.infos, code, status, "async", {j: G.ST_INVALID_ARGUMENT for j, w in enumerate(want) if w[0] == 1})


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. row ranges
# ---------------------------------------------------------------------------------------------------------------------------------------
def ranges_of(page_n):
    return [(0, 1), (255, 2), (256, 256), (page_n - 1, 1), (0, page_n), (page_n // 2, 0)]


@pytest.mark.parametrize("form", ["sync", "async"])
@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("spec", ["classic+consecutive1", "classic+lookback", "floatmult+consecutive1", "level12"])
def test_row_ranges(L, spec, gap, form):
    b = blob_of(L, spec, gap); c = b.c
    want = [(i, p, f, n) for i in range(c.k) for p, page_n in enumerate(c.pages[i]) for f, n in ranges_of(page_n)]
    job = Job(c, want, ranges=True)
    code, status = job.launch(b.directory(), form)
    job.check(c.infos, code, status, form)


def test_empty_ranges_are_ok_whatever_their_pieces_look_like(L):
    b = blob_of(L, "classic+consecutive1", 4); c = b.c; n = c.n_pieces

    def edit(o): o[1:] = o[1:][::-1].copy()
    job = Job(c, [(i, p, 5, 0) for i, p, _, _ in all_pages(c)], ranges=True)
    code, status = job.launch(b.directory(offs=edited(b, edit), blob_len=3), "async")
    job.check(c.infos, code, status, "async")
    assert n > 4


def test_a_page_damaged_behind_the_range(L):
    """The last page of the blob is overwritten from its middle on (its six batches' bits follow one another: behind batch 1).  Ranges inside batch
    0 answer OK; the ones beyond answer what pco_gfx_decompress_page_ranges answers for the same bytes through host-known pointers."""
    import torch
    b0 = blob_of(L, "classic+consecutive1", 4); c = b0.c
    b = Blob(c, 4)
    offs = b.offs.cpu().numpy().view(np.uint64); n = c.n_pieces
    start, end = int(offs[n - 1]) + 4, int(offs[n]); plen = end - start
    assert plen == int(c.infos["len"][n - 1]) and plen > 600
    b.blob[start + plen // 2: end] = 0xFF
    torch.cuda.synchronize()
    i = c.k - 1; p = len(c.pages[i]) - 1; page_n = c.pages[i][p]
    inside, beyond = [(0, 1), (0, 256), (17, 100), (255, 1)], [(0, page_n), (page_n - 1, 1), (page_n - 300, 300)]
    want = [(i, p, f, k) for f, k in inside + beyond]
    # the pointer form over the same bytes
    m0 = int(offs[int(c.piece_first[i])]) + 4; mlen = int(offs[int(c.piece_first[i]) + 1]) - m0
    ref = Job(c, want, ranges=True)
    t = np.zeros(len(want), RANGE_DT)
    for j, ((_, _, f, k), o) in enumerate(zip(want, ref.at)):
        t[j] = (b.blob.data_ptr() + m0, mlen, b.blob.data_ptr() + start, plen, ref.out.data_ptr() + o, page_n, f, k, c.dtb[i], 4)
    ref_res = np.zeros(len(want), U.RES_DT)
    L.pco_gfx_decompress_page_ranges(len(t), U.ptr(t), U.ptr(ref_res), None, None)
    assert (ref_res["status"][: len(inside)] == 0).all() and (ref_res["status"][len(inside):] != 0).all(), ref_res["status"]
    failing = {len(inside) + j: int(ref_res["status"][len(inside) + j]) for j in range(len(beyond))}
    for form in ("sync", "async"):
        job = Job(c, want, ranges=True)
        code, status = job.launch(b.directory(), form)
        torch.cuda.synchronize()
        rec = job.d_res.cpu().numpy().view(U.RES_DT)[: len(want)]
        print(f"damaged page, {form}: statuses {rec['status'].tolist()}, the pointer form's {ref_res['status'].tolist()}")
        for j in range(len(want)):
            assert (rec["status"][j], rec["n_out"][j], rec["consumed"][j], rec["aux"][j]) == (ref_res["status"][j], ref_res["n_out"][j], ref_res["consumed"][j], ref_res["aux"][j]), j
        host = job.out.cpu().numpy()
        for j, (o, nb) in enumerate(job.spans):   # (dst[0 .. count) of a failed range is unspecified; nothing else is written)
            if j not in failing:
                assert np.array_equal(host[o: o + nb], job.image[o: o + nb]), want[j]
            host[o: o + nb] = CANARY
        assert (host == CANARY).all(), "a byte outside the ranges' dst was written"
    assert set(failing.values()) <= {G.ST_INSUFFICIENT_DATA, G.ST_CORRUPTION}


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the pipeline: encode -> compact -> decode from the device directory -> snapshots, ONE synchronisation
# ---------------------------------------------------------------------------------------------------------------------------------------
def note(what, stream):
    print(f"  [note] {what}: stream.query() = {stream.query()} right after the call returned")


@pytest.mark.parametrize("ranges", [False, True], ids=["pages", "ranges"])
def test_the_pipeline_synchronises_once(L, ranges):
    import torch
    src = encoded(L, "classic+lookback")
    c = Call(L, src.arrays, src.cfg, src.page_lists)   # fresh slots and d_infos: nothing of this call is known on the host
    gap = 4; cap = sum(c.caps) + gap * c.n_pieces
    blob = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device="cuda"); offs = torch.zeros(c.n_pieces + 1, dtype=torch.int64, device="cuda")
    want = all_pages(c) if not ranges else [(i, p, f, n) for i, p, _, page_n in all_pages(c) for f, n in ranges_of(page_n)]
    job = Job(c, want, ranges=ranges)
    snap_blob, snap_offs, snap_out, snap_res = torch.zeros_like(blob), torch.zeros_like(offs), torch.zeros_like(job.out), torch.zeros_like(job.d_res)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    U.device_delay(s)
    tasks = c.make_tasks()
    G.check(L.pco_gfx_compress_wrapped_chunks_ex(c.k, tasks, C.addressof(c.cfg), None, c.d_infos.data_ptr(), handle(s))); note("encode", s)
    G.check(L.pco_gfx_compact_wrapped_chunks(c.k, tasks, C.addressof(c.cfg), c.d_infos.data_ptr(), gap, blob.data_ptr(), cap, 0, offs.data_ptr(), None, handle(s))); note("compact", s)
    code, status = job.launch(G.Directory(blob.data_ptr(), cap, offs.data_ptr(), c.n_pieces, gap, 0), "async", s); note("decode", s)
    with torch.cuda.stream(s):
        snap_blob.copy_(blob, non_blocking=True); snap_offs.copy_(offs, non_blocking=True); snap_out.copy_(job.out, non_blocking=True); snap_res.copy_(job.d_res, non_blocking=True)
    s.synchronize()   # the one synchronisation
    infos = c.device_infos()
    assert (infos["status"] == 0).all() and np.array_equal(infos["len"], src.infos["len"])
    job.check(infos, code, status, "async", out=snap_out, d_res=snap_res)
    so = snap_offs.cpu().numpy().view(np.uint64)
    assert np.array_equal(so, np.concatenate([[0], np.cumsum(infos["len"] + gap)]).astype(np.uint64))
    hb = snap_blob.cpu().numpy(); ref = blob_of(L, "classic+lookback", 4).blob.cpu().numpy()
    assert np.array_equal(hb[: int(so[-1])], ref[: int(so[-1])]), "the snapshot of the stream is not the stream"


def test_the_pipeline_through_paged(L):
    import torch
    src = encoded(L, "classic+consecutive2")
    s = torch.cuda.Stream()
    tensors = [torch.from_numpy(a.copy()).cuda() for a in src.arrays]
    torch.cuda.synchronize()
    cfg = paged_config()
    U.device_delay(s)
    comp = paged.compress_chunks(tensors, cfg, page_sizes=src.page_lists, gap=4, stream=s); note("paged.compress_chunks", s)
    assert comp.page_ns == src.pages
    outs, res = paged.decompress_chunks_async(comp, stream=s); note("paged.decompress_chunks_async", s)
    rows = [(0, 1), (2000, 2100), None, (0, N), (N - 1, N)]
    routs, rres = paged.decompress_rows_async(comp, rows, stream=s); note("paged.decompress_rows_async", s)
    with torch.cuda.stream(s):
        snaps = [o.clone() for o in outs] + [o.clone() for o in routs]; sres = res.clone(); srres = rres.clone()
    s.synchronize()   # the one synchronisation
    assert comp._dir is None, "the host directory was materialised"
    for a, o in zip(src.arrays, snaps[: len(outs)]):
        assert U.bits_equal(o.cpu().numpy(), a)
    for (lo, hi), a, o in zip([r for r in rows if r is not None], [a for a, r in zip(src.arrays, rows) if r is not None], snaps[len(outs):]):
        assert U.bits_equal(o.cpu().numpy(), a[lo: hi])
    r = sres.cpu().numpy().view(paged.RESULT_DT)
    assert len(r) == sum(len(p) for p in src.pages) and (r["status"] == 0).all() and np.array_equal(r["n_out"], np.concatenate(src.pages).astype(np.uint64))
    rr = srres.cpu().numpy().view(paged.RESULT_DT)
    n_parts = sum(len(paged.map_rows_to_pages(pl, *w)) for pl, w in zip(src.pages, rows) if w is not None)
    assert len(rr) == n_parts and (rr["status"] == 0).all() and int(rr["n_out"].sum()) == sum(hi - lo for lo, hi in (w for w in rows if w is not None))
    assert comp._dir is None


def paged_config():
    from pcodec_amd.config import DeltaSpec, ModeSpec, PagingSpec
    return ChunkConfig(mode_spec=ModeSpec.classic(), delta_spec=DeltaSpec.try_consecutive(2), paging_spec=PagingSpec.equal_pages_up_to(MAX_PAGE_N), enable_8_bit=True)


def test_two_streams_share_one_workspace(L):
    """Stream A: encode + compact of one call.  Stream B, at once: the directory decode of an EARLIER blob.  One thread, one workspace."""
    import torch
    b = blob_of(L, "classic+lookback", 0); c = b.c
    src = encoded(L, "floatmult+consecutive1")
    c2 = Call(L, src.arrays, src.cfg, src.page_lists)
    cap = sum(c2.caps); blob2 = torch.full((cap + 64,), 0xC3, dtype=torch.uint8, device="cuda"); offs2 = torch.zeros(c2.n_pieces + 1, dtype=torch.int64, device="cuda")
    job = Job(c, all_pages(c), ranges=False); rjob = Job(c, [(i, p, f, n) for i, p, _, page_n in all_pages(c) for f, n in ranges_of(page_n)], ranges=True)
    job2 = Job(c2, all_pages(c2), ranges=False)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    U.device_delay(sa, 10)
    G.check(L.pco_gfx_compress_wrapped_chunks_ex(c2.k, c2.tasks, C.addressof(c2.cfg), None, c2.d_infos.data_ptr(), handle(sa)))
    code, status = job.launch(b.directory(), "async", sb)
    G.check(L.pco_gfx_compact_wrapped_chunks(c2.k, c2.tasks, C.addressof(c2.cfg), c2.d_infos.data_ptr(), 0, blob2.data_ptr(), cap, 0, offs2.data_ptr(), None, handle(sa)))
    rcode, rstatus = rjob.launch(b.directory(), "async", sb)
    code2, status2 = job2.launch(G.Directory(blob2.data_ptr(), cap, offs2.data_ptr(), c2.n_pieces, 0, 0), "async", sa)
    torch.cuda.synchronize()
    job.check(c.infos, code, status, "async"); rjob.check(c.infos, rcode, rstatus, "async"); job2.check(src.infos, code2, status2, "async")
