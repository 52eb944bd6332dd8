"""The batched wrapped writer on torch device tensors (include/pco_gfx.h section 4c): what a row-group writer of an embedding format calls.

compress_chunks encodes every tensor as one wrapped chunk (ChunkMeta + pages, the bytes of wrapped::ChunkCompressor::write_meta / write_page)
and assembles the pieces into ONE contiguous device tensor, all on the caller's stream and without a host round trip;
decompress_chunks decodes such a blob page by page; decompress_chunks_async / decompress_rows_async do so from the directory as it lies on
the device (section 4e), so that encode -> compact -> decode is one stream-ordered pipeline; ChunkReader reads a chunk slice after slice from
the cursors the last read left, and save_cursors / decompress_chunks_from decode the segments of long pages side by side (section 4f);
index_pages builds those cursors in one asynchronous call and decompress_rows_from reads rows from them (section 4g).  torch is plumbing only (allocation, streams): every byte is produced by libpco_gfx.so,
and without a HIP device every call fails loudly."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as G
from .config import ChunkConfig

_TORCH_NAMES = {"torch.uint32": "uint32", "torch.uint64": "uint64", "torch.int32": "int32", "torch.int64": "int64", "torch.float32": "float32",
                "torch.float64": "float64", "torch.uint16": "uint16", "torch.int16": "int16", "torch.float16": "float16", "torch.uint8": "uint8",
                "torch.int8": "int8"}
INFO_DT = np.dtype([("offset", "<u8"), ("len", "<u8"), ("n", "<u8"), ("status", "<u4"), ("aux", "<u4")])   # PcoGfxPageInfo
RESULT_DT = np.dtype([("n_out", "<u8"), ("consumed", "<u8"), ("status", "<u4"), ("aux", "<u4")])   # PcoGfxTaskResult

Piece = namedtuple("Piece", "chunk piece n offset length")   # piece 0 = the chunk's ChunkMeta (n = 0), piece p = page p - 1; offset / length in the blob


def _require_device():
    L = G.lib()
    if L.pco_gfx_device_count() < 1:
        raise G.PcoGfxError(G.PcoCompressionError, G.ST_DEVICE_ERROR, "pcodec_amd.paged needs a HIP device; there is no CPU fallback")
    return L


def _dtype_name(t):
    try:
        return _TORCH_NAMES[str(t.dtype)]
    except KeyError:
        raise TypeError(f"unsupported data type: {t.dtype}")


class CompressedChunks:
    """What compress_chunks returns: `blob` (uint8 device tensor; the pieces, each behind `gap` untouched bytes), `offsets` (int64 device tensor of
    n_pieces + 1 entries: piece k occupies blob[offsets[k] + gap : offsets[k + 1]]), `page_ns` (per chunk the numbers in each of its pages:
    host arithmetic, known before the encode) and, on demand, the host-side `directory`.  Reading the directory (or `total`) is the only thing
    that synchronises."""

    def __init__(self, blob, offsets, d_infos, pieces_per_chunk, dtypes, gap, stream, keep, page_ns=None):
        self.blob, self.offsets, self.gap, self.dtypes, self.page_ns = blob, offsets, gap, dtypes, page_ns
        self._d_infos, self._ppc, self._stream, self._keep, self._dir = d_infos, pieces_per_chunk, stream, keep, None

    @property
    def directory(self):
        """[Piece(chunk, piece, n, offset, length)] of the chunks that were written (a chunk with a failed piece is left out whole and raises here)."""
        if self._dir is None:
            import torch
            (self._stream or torch.cuda.current_stream()).synchronize()
            infos = self._d_infos.cpu().numpy().view(INFO_DT)
            offs = self.offsets.cpu().numpy().view(np.uint64)
            if int(offs[-1]) == (1 << 64) - 1:
                raise G.PcoGfxError(G.PcoCompressionError, G.ST_INVALID_ARGUMENT, "compact: destination too small")
            bad = np.flatnonzero(infos["status"] != 0)
            if bad.size:
                raise G.PcoGfxError(G.PcoCompressionError, int(infos["status"][bad[0]]), f"wrapped encode: piece {int(bad[0])} failed")
            out = []; k = 0
            for c, npc in enumerate(self._ppc):
                for p in range(npc):
                    out.append(Piece(c, p, int(infos["n"][k]), int(offs[k]) + self.gap, int(infos["len"][k]))); k += 1
            self._dir = out; self._keep = None   # (the slots are no longer needed once the stream has drained)
        return self._dir

    @property
    def total(self):
        self.directory
        return int(self.offsets[-1].item())


def equal_pages(n, max_page_n):
    """The page sizes PagingSpec::EqualPagesUpTo(max_page_n) cuts n numbers into (0 => 2^18 per page; chunk_config.rs:145-161): as few pages as
    fit, the first n % n_pages of them one number longer.  Their count is pco_gfx_wrapped_n_pages(n, max_page_n)."""
    n, max_page_n = int(n), int(max_page_n) or 1 << 18
    if n == 0:
        return []
    n_pages = (n + max_page_n - 1) // max_page_n
    low, r = divmod(n, n_pages)
    return [low + 1] * r + [low] * (n_pages - r)


def compress_chunks(tensors, config=None, page_sizes=None, gap=0, stream=None):
    """Encode each 1-D device tensor as one wrapped chunk and compact the pieces.  `page_sizes`: None (the config's paging spec: EqualPagesUpTo,
    or its exact list when there is ONE tensor), or one entry per tensor, each None or a list of page sizes (PagingSpec::Exact).  `stream`: a
    torch.cuda.Stream (default: the current one).  Asynchronous under explicit mode / delta specs; Auto specs synchronise inside."""
    import torch
    L = _require_device()
    config = config or ChunkConfig()
    cfg = config.to_c()
    tensors = list(tensors)
    if page_sizes is None:
        exact = config.paging_spec.exact
        if exact is not None and len(tensors) != 1:
            raise ValueError("ChunkConfig.paging_spec is an exact page list: it applies to one chunk; pass page_sizes as a list per chunk for many")
        page_sizes = [exact] * len(tensors)
    if len(page_sizes) != len(tensors):
        raise ValueError("page_sizes needs one entry per tensor")
    stream = stream or torch.cuda.current_stream()
    k = len(tensors)
    tasks = (G.WrappedTask * max(k, 1))()
    keep = []; caps = []; ppc = []; names = []; page_ns = []
    for i, (t, ps) in enumerate(zip(tensors, page_sizes)):
        if t.dim() != 1 or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("every tensor must be a contiguous 1-D device tensor")
        name = _dtype_name(t); names.append(name); dt = G.DTYPE_BYTE[name]
        if ps is not None:
            arr = (C.c_uint64 * max(len(ps), 1))(*[int(x) for x in ps]); keep.append(arr)
            cap = L.pco_gfx_wrapped_chunk_cap_exact(arr, len(ps), dt, C.addressof(cfg)); npg = len(ps)
            if cap == 0 or npg == 0:
                raise G.PcoGfxError(G.PcoCompressionError, G.ST_INVALID_ARGUMENT, "cannot write data page of 0 numbers")
            page_ns.append([int(x) for x in ps])
        else:
            arr = None; npg = 0
            cap = L.pco_gfx_wrapped_chunk_cap(t.numel(), dt, C.addressof(cfg))
            page_ns.append(equal_pages(t.numel(), cfg.max_page_n))
            if len(page_ns[-1]) != L.pco_gfx_wrapped_n_pages(t.numel(), cfg.max_page_n):
                raise AssertionError("equal_pages disagrees with pco_gfx_wrapped_n_pages")
        caps.append(cap); ppc.append(1 + (npg or L.pco_gfx_wrapped_n_pages(t.numel(), cfg.max_page_n)))
        tasks[i] = G.WrappedTask(t.data_ptr(), t.numel(), 0, cap, dt, npg, C.cast(arr, C.c_void_p) if arr is not None else None)
    slot_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    n_pieces = int(sum(ppc))
    h = C.c_void_p(stream.cuda_stream)
    with torch.cuda.stream(stream):
        slots = torch.empty(int(slot_off[-1]) + 64, dtype=torch.uint8, device="cuda")   # (cap offsets are multiples of 16: every dst is aligned)
        d_infos = torch.empty(max(n_pieces, 1) * INFO_DT.itemsize, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n_pieces + 1, dtype=torch.int64, device="cuda")
        # (worst case of the stream: every slot full.  The blob is trimmed by the caller from offsets[-1] / the directory)
        blob = torch.empty(int(slot_off[-1]) + gap * n_pieces + 64, dtype=torch.uint8, device="cuda")
    for i in range(k):
        tasks[i].dst = slots.data_ptr() + int(slot_off[i])
    G.check(L.pco_gfx_compress_wrapped_chunks_ex(k, tasks, C.addressof(cfg), None, d_infos.data_ptr(), h))
    G.check(L.pco_gfx_compact_wrapped_chunks(k, tasks, C.addressof(cfg), d_infos.data_ptr(), gap, blob.data_ptr(), blob.numel(), 0, offsets.data_ptr(), None, h))
    return CompressedChunks(blob, offsets, d_infos, ppc, names, gap, stream, (slots, tensors), page_ns)


def _pieces_by_chunk(directory):
    """({chunk: its ChunkMeta piece}, {chunk: its page pieces in page order})"""
    metas = {}; pages = {}
    for p in directory:
        p = Piece(*p)
        if p.piece == 0:
            metas[p.chunk] = p
        else:
            pages.setdefault(p.chunk, []).append(p)
    return metas, {c: sorted(pl, key=lambda q: q.piece) for c, pl in pages.items()}


def decompress_chunks(blob, directory, dtypes, stream=None):
    """Decode every page of `directory` (CompressedChunks.directory, or the same tuples read from a file's footer) out of the device tensor `blob`
    through one pco_gfx_decompress_pages call.  `dtypes`: a numpy dtype name per chunk.  Returns one device tensor per chunk (raw bytes viewed
    as the chunk's dtype).  Synchronises `stream`."""
    import torch
    L = _require_device()
    stream = stream or torch.cuda.current_stream()
    metas, pages = _pieces_by_chunk(directory)
    outs = {}; tasks = []
    with torch.cuda.stream(stream):
        for c, pl in sorted(pages.items()):
            name = dtypes[c]; width = np.dtype(name).itemsize; n = sum(p.n for p in pl)
            outs[c] = torch.empty(n * width + 64, dtype=torch.uint8, device="cuda")
            at = 0; m = metas[c]
            for p in pl:
                tasks.append(G.PageTask(blob.data_ptr() + m.offset, m.length, blob.data_ptr() + p.offset, p.length, outs[c].data_ptr() + at * width, p.n,
                                        G.DTYPE_BYTE[name], 4))
                at += p.n
    arr = (G.PageTask * max(len(tasks), 1))(*tasks)
    res = (G.TaskResult * max(len(tasks), 1))()
    G.check(L.pco_gfx_decompress_pages(len(tasks), arr, res, None, C.c_void_p(stream.cuda_stream)))
    result = []
    for c in sorted(outs):
        name = dtypes[c]; n = sum(p.n for p in pages[c])
        result.append(outs[c][: n * np.dtype(name).itemsize].view(getattr(torch, name)))
    return result


def map_rows_to_pages(page_ns, start, stop):
    """The pages of a chunk that hold rows [start, stop) of it: [(page index, first row inside the page, count, offset in the output)].  Pure
    arithmetic over the chunk's page sizes; pages wholly outside the interval do not appear, an empty interval gives []."""
    total = sum(int(n) for n in page_ns)
    if start < 0 or start > stop or stop > total:
        raise ValueError(f"rows ({start}, {stop}) do not lie in a chunk of {total} rows")
    out = []; at = 0
    for p, n in enumerate(page_ns):
        lo, hi = max(start, at), min(stop, at + int(n))
        if lo < hi:
            out.append((p, lo - at, hi - lo, lo - start))
        at += int(n)
    return out


def decompress_rows(blob, directory, dtypes, rows, stream=None):
    """Rows of the chunks in `blob` without decoding the rest of their pages: `rows[c]` is (start, stop) in chunk c's row coordinates, or None to
    skip the chunk.  Every interval is mapped onto the pages it touches (map_rows_to_pages) and all of them go through ONE
    pco_gfx_decompress_page_ranges call, which walks each page only as far as its last wanted row.  Returns one device tensor of stop - start
    rows per requested chunk, in chunk order.  Synchronises `stream`."""
    import torch
    L = _require_device()
    stream = stream or torch.cuda.current_stream()
    metas, pages = _pieces_by_chunk(directory)
    outs = {}; tasks = []
    with torch.cuda.stream(stream):
        for c, want in enumerate(rows):
            if want is None:
                continue
            start, stop = int(want[0]), int(want[1])
            pl = pages.get(c, [])
            name = dtypes[c]; width = np.dtype(name).itemsize
            parts = map_rows_to_pages([p.n for p in pl], start, stop)
            outs[c] = (torch.empty((stop - start) * width + 64, dtype=torch.uint8, device="cuda"), stop - start)
            m = metas.get(c)
            for page_idx, first, count, at in parts:
                p = pl[page_idx]
                tasks.append(G.PageRangeTask(blob.data_ptr() + m.offset, m.length, blob.data_ptr() + p.offset, p.length, outs[c][0].data_ptr() + at * width,
                                             p.n, first, count, G.DTYPE_BYTE[name], 4))
    arr = (G.PageRangeTask * max(len(tasks), 1))(*tasks)
    res = (G.TaskResult * max(len(tasks), 1))()
    G.check(L.pco_gfx_decompress_page_ranges(len(tasks), arr, res, None, C.c_void_p(stream.cuda_stream)))
    return [outs[c][0][: outs[c][1] * np.dtype(dtypes[c]).itemsize].view(getattr(torch, dtypes[c])) for c in sorted(outs)]


def _directory_of(compressed):
    """PcoGfxDirectory of a CompressedChunks, and the index of each chunk's ChunkMeta piece (its pages follow it): host arithmetic only."""
    first = []; k = 0
    for pl in compressed.page_ns:
        first.append(k); k += 1 + len(pl)
    return G.Directory(compressed.blob.data_ptr(), compressed.blob.numel() - 64, compressed.offsets.data_ptr(), k, compressed.gap, 0), first


def decompress_chunks_async(compressed, stream=None):
    """Decode every page of a CompressedChunks through ONE asynchronous pco_gfx_decompress_pages_dir call: the page directory is read where
    compress_chunks left it, on the device, so nothing here synchronises and `compressed.directory` is never touched.  Returns (tensors,
    results): one device tensor per chunk, and a device tensor of PcoGfxTaskResult records (RESULT_DT), one per page in chunk-then-page order.
    Both are valid in `stream`'s order; a chunk the writer dropped shows as PCO_GFX_INSUFFICIENT_DATA in its pages' results."""
    import torch
    L = _require_device()
    stream = stream or torch.cuda.current_stream()
    d, first = _directory_of(compressed)
    outs = []; tasks = []
    with torch.cuda.stream(stream):
        for c, pl in enumerate(compressed.page_ns):
            name = compressed.dtypes[c]; width = np.dtype(name).itemsize
            out = torch.empty(sum(pl) * width + 64, dtype=torch.uint8, device="cuda"); outs.append(out)
            at = 0
            for p, n in enumerate(pl):
                tasks.append(G.DirPageTask(out.data_ptr() + at * width, n, first[c], first[c] + 1 + p, G.DTYPE_BYTE[name], 4))
                at += n
        results = torch.empty(max(len(tasks), 1) * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    arr = (G.DirPageTask * max(len(tasks), 1))(*tasks)
    G.check(L.pco_gfx_decompress_pages_dir(len(tasks), arr, C.addressof(d), None, results.data_ptr(), C.c_void_p(stream.cuda_stream)))
    tensors = [o[: sum(pl) * np.dtype(name).itemsize].view(getattr(torch, name)) for o, pl, name in zip(outs, compressed.page_ns, compressed.dtypes)]
    return tensors, results[: len(tasks) * RESULT_DT.itemsize]


def decompress_rows_async(compressed, rows, stream=None):
    """decompress_rows from the device directory: `rows[c]` is (start, stop) in chunk c's row coordinates, or None to skip the chunk; every
    interval goes through map_rows_to_pages and all of them through ONE asynchronous pco_gfx_decompress_page_ranges_dir call.  Returns (tensors,
    results) as decompress_chunks_async does, one tensor of stop - start rows per requested chunk and one result per page range, in task order.
    Never synchronises, never touches `compressed.directory`."""
    import torch
    L = _require_device()
    stream = stream or torch.cuda.current_stream()
    d, first = _directory_of(compressed)
    outs = {}; tasks = []
    with torch.cuda.stream(stream):
        for c, want in enumerate(rows):
            if want is None:
                continue
            start, stop = int(want[0]), int(want[1])
            pl = compressed.page_ns[c]
            name = compressed.dtypes[c]; width = np.dtype(name).itemsize
            parts = map_rows_to_pages(pl, start, stop)
            outs[c] = (torch.empty((stop - start) * width + 64, dtype=torch.uint8, device="cuda"), stop - start)
            for page_idx, row0, count, at in parts:
                tasks.append(G.DirPageRangeTask(outs[c][0].data_ptr() + at * width, pl[page_idx], row0, count, first[c], first[c] + 1 + page_idx,
                                                G.DTYPE_BYTE[name], 4))
        results = torch.empty(max(len(tasks), 1) * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    arr = (G.DirPageRangeTask * max(len(tasks), 1))(*tasks)
    G.check(L.pco_gfx_decompress_page_ranges_dir(len(tasks), arr, C.addressof(d), None, results.data_ptr(), C.c_void_p(stream.cuda_stream)))
    tensors = [outs[c][0][: outs[c][1] * np.dtype(compressed.dtypes[c]).itemsize].view(getattr(torch, compressed.dtypes[c])) for c in sorted(outs)]
    return tensors, results[: len(tasks) * RESULT_DT.itemsize]


# ---------------------------------------------------------------------------------------------------------------------------------------
# reading a page in slices, and from saved cursors (include/pco_gfx.h section 4f)
# ---------------------------------------------------------------------------------------------------------------------------------------
PageCursors = namedtuple("PageCursors", "chunk piece every_rows cursors")   # cursors: uint8 device tensor [k, 256]; row i stands in front of row (i + 1) * every_rows


def _run_reads(L, tasks, stream):
    arr = (G.PageReadTask * max(len(tasks), 1))(*tasks)
    res = (G.TaskResult * max(len(tasks), 1))()
    G.check(L.pco_gfx_decompress_page_reads(len(tasks), arr, res, None, C.c_void_p(stream.cuda_stream)))


class ChunkReader:
    """The rows of one chunk of `blob`, slice after slice: read(n_rows) returns the chunk's next n_rows as a device tensor, crossing pages, and
    keeps one PcoGfxPageCursor per page in a device tensor, so that a read costs the batches it covers and not the page's prefix (pages whose
    cursors are position-only -- Lookback, Conv1, Dict -- are decoded from their start each time: same rows, more work).  n_rows is a multiple of
    256 or reaches the chunk's end: the rule of the reference's PageDecompressor::read.  Each read synchronises `stream`."""

    def __init__(self, blob, directory, dtypes, chunk, stream=None):
        import torch
        self._L = _require_device()
        self._torch = torch
        self._stream = stream or torch.cuda.current_stream()
        metas, pages = _pieces_by_chunk(directory)
        self._blob, self._meta, self._pages = blob, metas[chunk], pages.get(chunk, [])
        self._name = dtypes[chunk]; self._width = np.dtype(self._name).itemsize
        self.n = sum(p.n for p in self._pages); self.pos = 0
        with torch.cuda.stream(self._stream):
            self.cursors = torch.zeros((max(len(self._pages), 1), G.CURSOR_BYTES), dtype=torch.uint8, device="cuda")
        self._cur_row = [0] * len(self._pages)   # the row each page's cursor stands in front of; 0: no cursor yet

    def _task(self, page_idx, first, count, dst, keep):
        p, m, base = self._pages[page_idx], self._meta, self._blob.data_ptr()
        cur = self.cursors.data_ptr() + page_idx * G.CURSOR_BYTES
        return G.PageReadTask(base + m.offset, m.length, base + p.offset, p.length, dst, p.n, first, count, G.DTYPE_BYTE[self._name], 4,
                              cur if self._cur_row[page_idx] else None, cur if keep else None)

    def read(self, n_rows):
        torch = self._torch
        n_rows = int(n_rows)
        if n_rows < 0 or n_rows > self.n - self.pos or (n_rows % 256 and n_rows != self.n - self.pos):
            raise ValueError(f"read({n_rows}): a multiple of 256 rows, or the {self.n - self.pos} rows that reach the chunk's end")
        with torch.cuda.stream(self._stream):
            out = torch.empty(n_rows * self._width + 64, dtype=torch.uint8, device="cuda")
        first_call = []; second_call = []; moved = []
        for page_idx, first, count, at in map_rows_to_pages([p.n for p in self._pages], self.pos, self.pos + n_rows):
            end, page_n, dst = first + count, self._pages[page_idx].n, out.data_ptr() + at * self._width
            floor = end // 256 * 256
            if end == page_n or end == floor:      # the cursor the read leaves stands at its end
                first_call.append(self._task(page_idx, first, count, dst, True)); moved.append((page_idx, end))
            elif floor <= first:                    # inside one batch: the cursor stays in front of it
                first_call.append(self._task(page_idx, first, count, dst, False))
            else:                                   # up to the last batch boundary, then the rest from the cursor that leaves
                first_call.append(self._task(page_idx, first, floor - first, dst, True)); moved.append((page_idx, floor))
                second_call.append((page_idx, floor, end - floor, dst + (floor - first) * self._width))
        _run_reads(self._L, first_call, self._stream)
        for page_idx, row in moved:
            self._cur_row[page_idx] = row
        if second_call:
            _run_reads(self._L, [self._task(*t, False) for t in second_call], self._stream)
        self.pos += n_rows
        return out[: n_rows * self._width].view(getattr(torch, self._name))


def save_cursors(blob, directory, dtypes, every_rows, stream=None):
    """Walk every page of `directory` once, in slices of `every_rows` (a multiple of 256), and keep the cursor in front of every slice but the
    first: [PageCursors(chunk, piece, every_rows, cursors)] in chunk-then-page order, for decompress_chunks_from.  One call per slice index over
    all pages; the rows themselves go to a scratch tensor and are dropped."""
    import torch
    L = _require_device()
    every_rows = int(every_rows)
    if every_rows <= 0 or every_rows % 256:
        raise ValueError("every_rows must be a positive multiple of 256")
    stream = stream or torch.cuda.current_stream()
    metas, pages = _pieces_by_chunk(directory)
    out = []; jobs = []
    with torch.cuda.stream(stream):
        for c, pl in sorted(pages.items()):
            for p in pl:
                k = max((p.n - 1) // every_rows, 0)
                pc = PageCursors(c, p.piece, every_rows, torch.zeros((k, G.CURSOR_BYTES), dtype=torch.uint8, device="cuda"))
                out.append(pc); jobs.append((pc, p, metas[c], dtypes[c]))
        scratch = torch.empty(max(len(jobs), 1) * every_rows * 8 + 64, dtype=torch.uint8, device="cuda")
    for s in range(max((pc.cursors.shape[0] for pc in out), default=0)):
        tasks = []
        for j, (pc, p, m, name) in enumerate(jobs):
            if s >= pc.cursors.shape[0]:
                continue
            cur = pc.cursors.data_ptr()
            tasks.append(G.PageReadTask(blob.data_ptr() + m.offset, m.length, blob.data_ptr() + p.offset, p.length, scratch.data_ptr() + j * every_rows * 8, p.n,
                                        s * every_rows, every_rows, G.DTYPE_BYTE[name], 4, cur + (s - 1) * G.CURSOR_BYTES if s else None, cur + s * G.CURSOR_BYTES))
        _run_reads(L, tasks, stream)
    return out


class PageIndex(list):
    """What index_pages returns: the [PageCursors] save_cursors returns, and `results`: a device tensor of PcoGfxTaskResult records (RESULT_DT), one
    per page in the list's order, valid in the call's stream order like the cursors themselves (n_out = the page's cursor count on status 0)."""
    results = None


def index_pages(blob, directory, dtypes, every_rows, stream=None):
    """save_cursors through ONE asynchronous pco_gfx_index_pages call (include/pco_gfx.h section 4g): every page of `directory` is walked once, as
    far as its last cursor, and no rows are decoded.  Returns the same [PageCursors], byte for byte, valid in `stream`'s order; nothing here
    synchronises, so a page that fails shows in `.results`, not as an exception."""
    import torch
    L = _require_device()
    every_rows = int(every_rows)
    if every_rows <= 0 or every_rows % 256:
        raise ValueError("every_rows must be a positive multiple of 256")
    stream = stream or torch.cuda.current_stream()
    metas, pages = _pieces_by_chunk(directory)
    out = PageIndex(); tasks = []
    with torch.cuda.stream(stream):
        for c, pl in sorted(pages.items()):
            m = metas[c]
            for p in pl:
                k = max((p.n - 1) // every_rows, 0)
                pc = PageCursors(c, p.piece, every_rows, torch.zeros((k, G.CURSOR_BYTES), dtype=torch.uint8, device="cuda"))
                out.append(pc)
                tasks.append(G.PageIndexTask(blob.data_ptr() + m.offset, m.length, blob.data_ptr() + p.offset, p.length, pc.cursors.data_ptr() if k else None, p.n,
                                             every_rows, G.DTYPE_BYTE[dtypes[c]], 4))
        out.results = torch.zeros(max(len(tasks), 1) * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")[: len(tasks) * RESULT_DT.itemsize]
    arr = (G.PageIndexTask * max(len(tasks), 1))(*tasks)
    G.check(L.pco_gfx_index_pages(len(tasks), arr, None, out.results.data_ptr(), C.c_void_p(stream.cuda_stream)))
    return out


def decompress_rows_from(blob, directory, dtypes, cursors, rows, stream=None):
    """decompress_rows with each page's task starting from the last saved cursor (save_cursors, index_pages) at or in front of its first row, not from
    the page's first batch: ONE pco_gfx_decompress_page_reads call whose tasks walk from their cursors to their last rows.  A page without saved
    cursors, or rows in front of its first one, is read from its start.  Synchronises `stream`."""
    import torch
    L = _require_device()
    stream = stream or torch.cuda.current_stream()
    metas, pages = _pieces_by_chunk(directory)
    saved = {(pc.chunk, pc.piece): pc for pc in (PageCursors(*x) for x in cursors)}
    outs = {}; tasks = []
    with torch.cuda.stream(stream):
        for c, want in enumerate(rows):
            if want is None:
                continue
            start, stop = int(want[0]), int(want[1])
            pl = pages.get(c, [])
            name = dtypes[c]; width = np.dtype(name).itemsize
            parts = map_rows_to_pages([p.n for p in pl], start, stop)
            outs[c] = (torch.empty((stop - start) * width + 64, dtype=torch.uint8, device="cuda"), stop - start)
            m = metas.get(c)
            for page_idx, first, count, at in parts:
                p = pl[page_idx]
                pc = saved.get((c, p.piece))
                s = min(first // pc.every_rows, pc.cursors.shape[0]) if pc is not None else 0   # cursor s - 1 stands in front of row s * every_rows
                tasks.append(G.PageReadTask(blob.data_ptr() + m.offset, m.length, blob.data_ptr() + p.offset, p.length, outs[c][0].data_ptr() + at * width,
                                            p.n, first, count, G.DTYPE_BYTE[name], 4, pc.cursors.data_ptr() + (s - 1) * G.CURSOR_BYTES if s else None, None))
    _run_reads(L, tasks, stream)
    return [outs[c][0][: outs[c][1] * np.dtype(dtypes[c]).itemsize].view(getattr(torch, dtypes[c])) for c in sorted(outs)]


def decompress_chunks_from(blob, directory, dtypes, cursors, stream=None):
    """decompress_chunks with every page cut at its saved cursors (save_cursors): all segments of all pages are tasks of ONE
    pco_gfx_decompress_page_reads call, each walking its own segment only -- a long page's tANS chain runs as many chains side by side as it has
    segments.  Returns one device tensor per chunk.  Synchronises `stream`."""
    import torch
    L = _require_device()
    stream = stream or torch.cuda.current_stream()
    metas, pages = _pieces_by_chunk(directory)
    saved = {(pc.chunk, pc.piece): pc for pc in (PageCursors(*x) for x in cursors)}
    outs = {}; tasks = []
    with torch.cuda.stream(stream):
        for c, pl in sorted(pages.items()):
            name = dtypes[c]; width = np.dtype(name).itemsize; n = sum(p.n for p in pl)
            outs[c] = (torch.empty(n * width + 64, dtype=torch.uint8, device="cuda"), n)
            at = 0; m = metas[c]
            for p in pl:
                pc = saved.get((c, p.piece))
                every = pc.every_rows if pc is not None and pc.cursors.shape[0] else p.n
                for s, row in enumerate(range(0, p.n, every)):
                    tasks.append(G.PageReadTask(blob.data_ptr() + m.offset, m.length, blob.data_ptr() + p.offset, p.length, outs[c][0].data_ptr() + (at + row) * width,
                                                p.n, row, min(every, p.n - row), G.DTYPE_BYTE[name], 4,
                                                pc.cursors.data_ptr() + (s - 1) * G.CURSOR_BYTES if s else None, None))
                at += p.n
    _run_reads(L, tasks, stream)
    return [outs[c][0][: outs[c][1] * np.dtype(dtypes[c]).itemsize].view(getattr(torch, dtypes[c])) for c in sorted(outs)]
