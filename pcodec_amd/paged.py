"""The batched wrapped writer on torch device tensors (include/pco_gfx.h section 4c): what a row-group writer of an embedding format calls.

compress_chunks encodes every tensor as one wrapped chunk (ChunkMeta + pages, the bytes of wrapped::ChunkCompressor::write_meta / write_page)
and assembles the pieces into ONE contiguous device tensor, all on the caller's stream and without a host round trip;
decompress_chunks decodes such a blob page by page; decompress_chunks_async / decompress_rows_async do so from the directory as it lies on
the device (section 4e), so that encode -> compact -> decode is one stream-ordered pipeline; ChunkReader reads a chunk slice after slice from
the cursors the last read left, and save_cursors / decompress_chunks_from decode the segments of long pages side by side (section 4f);
index_pages builds those cursors in one asynchronous call and decompress_rows_from reads rows from them (section 4g); with history=True it
snapshots a history beside every cursor of a Lookback page, and the two *_from functions take them as histories= (section 4j);
index_pages_async / decompress_chunks_from_async / decompress_rows_from_async are those three from the device directory (section 4k): encode ->
compact -> index -> decode in one stream's order; compress_standalone_chunks writes STANDALONE chunks (a .pco file) the same way, and the five *_async
functions take what it returns as well (section 4l); ChunkConfig(verify=True) makes either writer decode every chunk again and compare it with its
tensor, `.verified` says which chunks passed, and verify_chunks is that check as a step of its own (section 3b); scan_files / scan_files_async find the
chunk directory of .pco files that carry none, on the device, and decompress_files decodes such files chunk-parallel behind it (section 4m); take_rows /
take_rows_async take the rows that device-resident row ids name, from indexed pages, walking only the segments the ids fall into (section 4n).  torch is plumbing only (allocation, streams): every byte is produced by libpco_gfx.so,
and without a HIP device every call fails loudly.

Every decode function is the same three steps.  A page source (_BlobPages, _DirPages, _DirChunks) says where the pages are and builds the tasks; _whole_chunks /
_rows_of_chunks allocate the outputs and lay the tasks out, which is arithmetic; _launch hands a task list to the library."""
import ctypes as C
import functools
import os
from collections import namedtuple

import numpy as np

from . import _lib as G
from .config import ChunkConfig

INFO_DT = np.dtype([("offset", "<u8"), ("len", "<u8"), ("n", "<u8"), ("status", "<u4"), ("aux", "<u4")])   # PcoGfxPageInfo
RESULT_DT = np.dtype([("n_out", "<u8"), ("consumed", "<u8"), ("status", "<u4"), ("aux", "<u4")])   # PcoGfxTaskResult

Piece = namedtuple("Piece", "chunk piece n offset length")   # piece 0 = the chunk's ChunkMeta (n = 0), piece p = page p - 1; offset / length in the blob


def _require_device():
    L = G.lib()
    if L.pco_gfx_device_count() < 1:
        raise G.PcoGfxError(G.PcoCompressionError, G.ST_DEVICE_ERROR, "pcodec_amd.paged needs a HIP device; there is no CPU fallback")
    return L


def _dtype_name(t):
    name = str(t.dtype).rpartition(".")[2]   # "torch.uint32" -> numpy's name
    if name not in G.DTYPE_BYTE:
        raise TypeError(f"unsupported data type: {t.dtype}")
    return name


class CompressedChunks:
    """What compress_chunks returns: `blob` (uint8 device tensor; the pieces, each behind `gap` untouched bytes), `offsets` (int64 device tensor of
    n_pieces + 1 entries: piece k occupies blob[offsets[k] + gap : offsets[k + 1]]), `page_ns` (per chunk the numbers in each of its pages:
    host arithmetic, known before the encode) and, on demand, the host-side `directory`.  Reading the directory (or `total`) is the only thing
    that synchronises."""

    def __init__(self, blob, offsets, d_infos, pieces_per_chunk, dtypes, gap, stream, keep, page_ns=None, tasks=None, cfg=None):
        self.blob, self.offsets, self.gap, self.dtypes, self.page_ns = blob, offsets, gap, dtypes, page_ns
        self._d_infos, self._ppc, self._stream, self._keep, self._dir = d_infos, pieces_per_chunk, stream, keep, None
        self._tasks, self._cfg = tasks, cfg   # (verify_chunks: the encode's task array and config, valid while the slots are kept)
        self._meta_rows = self._meta_rows_host = None   # (`verified`: the ChunkMeta pieces' indices, pinned on the host and on the device, made on first use)

    @property
    def slots(self):
        """The encoder's worst-case slots (uint8 device tensor; chunk i's pieces lie at its task's dst), alive until `directory` or `total` is read;
        what verify_chunks decodes."""
        return None if self._keep is None else self._keep[0]

    @property
    def verified(self):
        """A device bool tensor per chunk, valid in the order of the encode's stream and made without a synchronisation: the chunk's ChunkMeta piece is OK and carries
        PCO_GFX_AUX_VERIFIED, i.e. every page of it was decoded again and equals its source (ChunkConfig(verify=True), or verify_chunks)."""
        import torch
        with torch.cuda.stream(self._stream or torch.cuda.current_stream()):
            if self._meta_rows is None:   # uploaded once, from PINNED memory in the stream's order: a pageable source would make torch wait for the stream
                self._meta_rows_host = torch.from_numpy(np.concatenate([[0], np.cumsum(self._ppc)[:-1]]).astype(np.int64)[: len(self._ppc)]).pin_memory()
                self._meta_rows = self._meta_rows_host.to("cuda", non_blocking=True)
            words = self._d_infos[: sum(self._ppc) * INFO_DT.itemsize].view(torch.int32).view(-1, INFO_DT.itemsize // 4)
            meta = words.index_select(0, self._meta_rows)
            return (meta[:, 6] == 0) & ((meta[:, 7] & G.AUX_VERIFIED) != 0)

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


def spec_array(specs, k, config=None):
    """The ctypes array a `specs=` keyword stands for: one ChunkSpec per tensor, or a single one applied to all k.  The config beside it must leave
    mode and delta at Auto, so that a spec is never silently overridden.  Host arithmetic: checked before a device is asked for."""
    if isinstance(specs, G.ChunkSpec):
        specs = [specs] * k
    specs = list(specs)
    if len(specs) != k:
        raise ValueError(f"specs needs one ChunkSpec per tensor, or a single one for all: {len(specs)} specs for {k} tensors")
    if any(not isinstance(s, G.ChunkSpec) for s in specs):
        raise TypeError("specs holds ChunkSpec objects (resolve_specs, spec_from_meta)")
    if config is not None and (config.mode_spec.kind != G.MODE_AUTO or config.delta_spec.kind != G.DELTA_AUTO):
        raise ValueError("with specs= the config must leave mode_spec and delta_spec at Auto: the specs say both")
    arr = (G.ChunkSpec * max(k, 1))()
    for i, s in enumerate(specs):
        C.memmove(C.addressof(arr[i]), C.addressof(s), C.sizeof(G.ChunkSpec))
    return arr


def resolve_specs(tensors, config=None, stream=None):
    """What an encode of `tensors` under `config` (default: Auto mode, Auto delta, level 8) would resolve, one ChunkSpec per tensor
    (pco_gfx_resolve_chunk_specs, section 3c).  Synchronous.  Keep the list and pass it as specs= to compress_chunks / compress_standalone_chunks
    for the later row groups of the same columns: they then encode through the explicit path, asynchronously, and write the bytes the Auto call
    writes as long as the data resolves the same way."""
    import torch
    L = _require_device()
    cfg = (config or ChunkConfig()).to_c()
    tensors = list(tensors)
    stream = stream or torch.cuda.current_stream()
    k = len(tensors)
    tasks = (G.EncodeTask * max(k, 1))()
    for i, t in enumerate(tensors):
        if t.dim() != 1 or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("every tensor must be a contiguous 1-D device tensor")
        tasks[i] = G.EncodeTask(t.data_ptr(), t.numel(), None, 0, G.DTYPE_BYTE[_dtype_name(t)], 0)
    out = (G.ChunkSpec * max(k, 1))()
    G.check(L.pco_gfx_resolve_chunk_specs(k, tasks, C.addressof(cfg), out, stream.cuda_stream))
    return [G.ChunkSpec.from_buffer_copy(out[i]) for i in range(k)]


def spec_from_meta(meta_bytes, dtype, format_major=4):
    """The ChunkSpec a ChunkMeta's mode and delta encoding describe (pco_gfx_chunk_spec_from_meta; no device).  `dtype`: a numpy / torch dtype, its
    name, or the type byte.  mode_inv is 0 -- the metadata does not store FloatMult's inverse -- so the spec means TryFloatMult(base), which need
    not give the bytes of the writer that found the base under Auto; resolve_specs does."""
    dtype = G.dtype_byte(dtype)
    meta = bytes(meta_bytes)
    buf = (C.c_uint8 * max(len(meta), 1)).from_buffer_copy(meta or b"\0")
    out = G.ChunkSpec()
    G.check(G.lib().pco_gfx_chunk_spec_from_meta(buf, len(meta), dtype, format_major, C.byref(out)))
    return out


def compress_chunks(tensors, config=None, page_sizes=None, gap=0, stream=None, specs=None):
    """Encode each 1-D device tensor as one wrapped chunk and compact the pieces.  `page_sizes`: None (the config's paging spec: EqualPagesUpTo,
    or its exact list when there is ONE tensor), or one entry per tensor, each None or a list of page sizes (PagingSpec::Exact).  `stream`: a
    torch.cuda.Stream (default: the current one).  Asynchronous under explicit mode / delta specs; Auto specs synchronise inside.  `specs`: one
    ChunkSpec per tensor, or a single one for all (resolve_specs, spec_from_meta): every chunk is encoded under its own, asynchronously, and the
    config must leave mode and delta at Auto."""
    tensors = list(tensors)
    d_specs = None if specs is None else spec_array(specs, len(tensors), config)
    import torch
    L = _require_device()
    config = config or ChunkConfig()
    cfg = config.to_c()
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
    with torch.cuda.stream(stream):
        slots = torch.empty(int(slot_off[-1]) + 64, dtype=torch.uint8, device="cuda")   # (cap offsets are multiples of 16: every dst is aligned)
        d_infos = torch.empty(max(n_pieces, 1) * INFO_DT.itemsize, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(n_pieces + 1, dtype=torch.int64, device="cuda")
        # (worst case of the stream: every slot full.  The blob is trimmed by the caller from offsets[-1] / the directory)
        blob = torch.empty(int(slot_off[-1]) + gap * n_pieces + 64, dtype=torch.uint8, device="cuda")
    for i in range(k):
        tasks[i].dst = slots.data_ptr() + int(slot_off[i])
    if d_specs is None:
        G.check(L.pco_gfx_compress_wrapped_chunks_ex(k, tasks, C.addressof(cfg), None, d_infos.data_ptr(), stream.cuda_stream))
    else:
        G.check(L.pco_gfx_compress_wrapped_chunks_specs(k, tasks, C.addressof(cfg), d_specs, None, d_infos.data_ptr(), stream.cuda_stream))
    G.check(L.pco_gfx_compact_wrapped_chunks(k, tasks, C.addressof(cfg), d_infos.data_ptr(), gap, blob.data_ptr(), blob.numel(), 0, offsets.data_ptr(), None,
                                             stream.cuda_stream))
    return CompressedChunks(blob, offsets, d_infos, ppc, names, gap, stream, (slots, tensors, keep), page_ns, tasks, cfg)


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


# Where the pages are: the two page sources.  Page i of chunk c is a (c, i) pair to everything below; only a source turns it into a task.
class _BlobPages:
    """The pages of `blob` by ADDRESS, from the host directory (CompressedChunks.directory, or the same tuples read from a file's footer).  Per
    chunk, in page order: `ns` its pages' row counts, `piece` their piece numbers, `pages` their (address, length); `metas`: each chunk's ChunkMeta
    likewise, and the two together are how every task by address starts.  The results of a call come to the host: it synchronises."""
    PAGE, RANGE, results, directory = G.PageTask, G.PageRangeTask, None, None

    def __init__(self, blob, directory, dtypes):
        base, self.dtypes, self.metas, pages = blob.data_ptr(), dtypes, {}, {}
        for c, piece, n, offset, length in directory:
            if piece == 0:
                self.metas[c] = (base + offset, length)
            else:
                pages.setdefault(c, []).append((piece, n, base + offset, length))
        for pl in pages.values():
            pl.sort()
        self.piece = {c: [p[0] for p in pl] for c, pl in pages.items()}
        self.ns = {c: [p[1] for p in pl] for c, pl in pages.items()}
        self.pages = {c: [p[2:] for p in pl] for c, pl in pages.items()}

    def page_task(self, c, i, dst):
        return G.PageTask(*self.metas[c], *self.pages[c][i], dst, self.ns[c][i], G.DTYPE_BYTE[self.dtypes[c]], 4)

    def range_task(self, c, i, dst, first, count):
        return G.PageRangeTask(*self.metas[c], *self.pages[c][i], dst, self.ns[c][i], first, count, G.DTYPE_BYTE[self.dtypes[c]], 4)

    def read_task(self, c, i, dst, first, count, from_, to):
        return G.PageReadTask(*self.metas[c], *self.pages[c][i], dst, self.ns[c][i], first, count, G.DTYPE_BYTE[self.dtypes[c]], 4, from_, to)

    def read_hist_task(self, c, i, dst, first, count, from_, to, history, history_len):
        return G.PageReadHistTask(*self.metas[c], *self.pages[c][i], dst, self.ns[c][i], first, count, G.DTYPE_BYTE[self.dtypes[c]], 4, from_, to, history, history_len)

    def index_task(self, c, i, cursors, every_rows):
        return G.PageIndexTask(*self.metas[c], *self.pages[c][i], cursors, self.ns[c][i], every_rows, G.DTYPE_BYTE[self.dtypes[c]], 4)

    def index_hist_task(self, c, i, cursors, every_rows, histories, history_stride):
        return G.PageIndexHistTask(*self.metas[c], *self.pages[c][i], cursors, self.ns[c][i], every_rows, G.DTYPE_BYTE[self.dtypes[c]], 4, histories, history_stride)

    def history_bytes(self, L, blob, c):
        """The bytes of one history of a page of chunk c: 0 unless the chunk's delta encoding is Lookback (pco_gfx_chunk_meta_info on the ChunkMeta's
        bytes, which are read back from the device: this synchronises)."""
        address, length = self.metas[c]
        at = address - blob.data_ptr()
        meta = blob[at: at + length].cpu().numpy().tobytes()
        info = G.ChunkMetaInfo()
        buf = (C.c_uint8 * max(length, 1)).from_buffer_copy(meta or b"\0")
        dt = G.DTYPE_BYTE[self.dtypes[c]]
        G.check(L.pco_gfx_chunk_meta_info(buf, length, dt, 4, C.byref(info)))
        return L.pco_gfx_lookback_history_bytes(info.window_n_log, dt) if info.delta_kind == 2 else 0


class _DirPages:
    """The pages of a CompressedChunks by PIECE INDEX into the directory as compress_chunks left it on the device: host arithmetic only, and the
    results of a call stay on the device too, so nothing synchronises.  Chunk c's ChunkMeta is piece first[c]; its pages follow it."""
    PAGE, RANGE, READ, INDEX, results = G.DirPageTask, G.DirPageRangeTask, G.DirPageReadTask, G.DirPageIndexTask, "empty"

    def __init__(self, compressed):
        self.dtypes, self.ns, self.first, k = compressed.dtypes, dict(enumerate(compressed.page_ns)), [], 0
        for pl in compressed.page_ns:
            self.first.append(k); k += 1 + len(pl)
        self.piece = {c: list(range(1, 1 + len(ns))) for c, ns in self.ns.items()}
        self.directory = G.Directory(compressed.blob.data_ptr(), compressed.blob.numel() - 64, compressed.offsets.data_ptr(), k, compressed.gap, 0)

    def page_task(self, c, i, dst):
        return G.DirPageTask(dst, self.ns[c][i], self.first[c], self.first[c] + 1 + i, G.DTYPE_BYTE[self.dtypes[c]], 4)

    def range_task(self, c, i, dst, first, count):
        return G.DirPageRangeTask(dst, self.ns[c][i], first, count, self.first[c], self.first[c] + 1 + i, G.DTYPE_BYTE[self.dtypes[c]], 4)

    # Reads and indexes (section 4k).  `piece`: page i of a chunk is piece i + 1 of it, as in the host directory, so that a PageCursors made from either
    # source has the same key and the same bytes.  There is ONE task kind per job here: a read without a history is the read with history None.
    def read_hist_task(self, c, i, dst, first, count, from_, to, history, history_len):
        return G.DirPageReadTask(dst, self.ns[c][i], first, count, self.first[c], self.first[c] + 1 + i, G.DTYPE_BYTE[self.dtypes[c]], 4, from_, to, history, history_len)

    def read_task(self, c, i, dst, first, count, from_, to):
        return self.read_hist_task(c, i, dst, first, count, from_, to, None, 0)

    def index_hist_task(self, c, i, cursors, every_rows, histories, history_stride):
        return G.DirPageIndexTask(cursors, self.ns[c][i], every_rows, self.first[c], self.first[c] + 1 + i, G.DTYPE_BYTE[self.dtypes[c]], 4, histories, history_stride)

    def index_task(self, c, i, cursors, every_rows):
        return self.index_hist_task(c, i, cursors, every_rows, None, 0)


class _DirChunks:
    """The STANDALONE chunks of a CompressedStandaloneChunks by piece index into the offsets pco_gfx_compact_chunks left on the device (section 4l).
    To everything below, chunk c is a chunk of ONE page of its n rows; the library finds the ChunkMeta and the page inside piece c on the device.  Its
    page's key is piece 1, as the first page of a wrapped chunk's, and a row range is a read without cursors: there is one task kind per job."""
    PAGE, RANGE, READ, INDEX, results = G.DirChunkTask, G.DirChunkReadTask, G.DirChunkReadTask, G.DirChunkIndexTask, "empty"

    def __init__(self, compressed):
        self.dtypes, self.ns = compressed.dtypes, {c: [int(n)] for c, n in enumerate(compressed.ns)}
        self.piece = {c: [1] for c in self.ns}
        self.directory = G.Directory(compressed.blob.data_ptr(), compressed.blob.numel() - 64, compressed.offsets.data_ptr(), len(compressed.ns), compressed.gap, 0)

    def page_task(self, c, i, dst):
        return G.DirChunkTask(dst, self.ns[c][i], c, c, G.DTYPE_BYTE[self.dtypes[c]], 4)

    def read_hist_task(self, c, i, dst, first, count, from_, to, history, history_len):
        return G.DirChunkReadTask(dst, self.ns[c][i], first, count, c, c, G.DTYPE_BYTE[self.dtypes[c]], 4, from_, to, history, history_len)

    def read_task(self, c, i, dst, first, count, from_, to):
        return self.read_hist_task(c, i, dst, first, count, from_, to, None, 0)

    def range_task(self, c, i, dst, first, count):
        return self.read_hist_task(c, i, dst, first, count, None, None, None, 0)

    def index_hist_task(self, c, i, cursors, every_rows, histories, history_stride):
        return G.DirChunkIndexTask(cursors, self.ns[c][i], every_rows, c, c, G.DTYPE_BYTE[self.dtypes[c]], 4, histories, history_stride)

    def index_task(self, c, i, cursors, every_rows):
        return self.index_hist_task(c, i, cursors, every_rows, None, 0)


class CompressedStandaloneChunks:
    """What compress_standalone_chunks returns: `blob` (uint8 device tensor), `offsets` (int64 device tensor of k + 1 entries: chunk c occupies
    blob[offsets[c] : offsets[c + 1]], a chunk that failed nothing), `ns` and `dtypes` (per chunk, host arithmetic), `results` (device tensor of
    RESULT_DT records, the encoder's) and `header_len`.  `total` and `file` are the only things that synchronise."""
    gap = 0

    def __init__(self, blob, offsets, results, ns, dtypes, header_len, stream, keep):
        self.blob, self.offsets, self.results, self.ns, self.dtypes, self.header_len = blob, offsets, results, ns, dtypes, header_len
        self._stream, self._keep = stream, keep
        self._tasks = self._blob_cap = None   # (verify_chunks: the encode's task array and the compactor's capacity, set by compress_standalone_chunks)

    @property
    def slots(self):
        """The encoder's worst-case slots (uint8 device tensor; chunk i lies at its task's dst), alive until `total` or `file` is read; what
        verify_chunks decodes."""
        return None if self._keep is None else self._keep[0]

    @property
    def verified(self):
        """A device bool tensor per chunk, valid in the order of the encode's stream and made without a synchronisation: the chunk's result is OK and carries
        PCO_GFX_AUX_VERIFIED (ChunkConfig(verify=True), or verify_chunks)."""
        import torch
        with torch.cuda.stream(self._stream or torch.cuda.current_stream()):
            words = self.results[: len(self.ns) * RESULT_DT.itemsize].view(torch.int32).view(-1, RESULT_DT.itemsize // 4)
            return (words[:, 4] == 0) & ((words[:, 5] & G.AUX_VERIFIED) != 0)

    @property
    def total(self):
        """The end of the last chunk (synchronises); a destination too small raises."""
        import torch
        (self._stream or torch.cuda.current_stream()).synchronize()
        self._keep = None
        end = int(self.offsets[-1].item())
        if end == -1:
            raise G.PcoGfxError(G.PcoCompressionError, G.ST_INVALID_ARGUMENT, "compact: destination too small")
        return end

    @property
    def file(self):
        """The trimmed blob: with file_frame a whole .pco file -- header, chunks, terminator (synchronises)."""
        return self.blob[: self.total + (1 if self.header_len else 0)]


def compress_standalone_chunks(tensors, config=None, stream=None, file_frame=True, blob_cap=None, specs=None):
    """Encode each 1-D device tensor (1 ..= 2^24 numbers) as one STANDALONE chunk through pco_gfx_compress_chunks and compact the chunks through
    pco_gfx_compact_chunks, both asynchronous on `stream` (Auto specs synchronise inside).  `file_frame`: the chunks start behind
    pco_gfx_write_standalone_header's bytes and the terminator follows the last one, so that the trimmed blob (`.file`) is a .pco file the reference
    reads.  `blob_cap`: the bytes the blob may take, header and terminator included (default: the chunks' worst case, which always fits); when the
    chunks need more, the compactor copies nothing, `.total` and `.file` raise and every decode task answers PCO_GFX_INVALID_ARGUMENT.  The decode
    functions that take a CompressedChunks take the result too (section 4l).  `specs`: as in compress_chunks (pco_gfx_compress_chunks_specs)."""
    tensors = list(tensors)
    d_specs = None if specs is None else spec_array(specs, len(tensors), config)
    import torch
    L = _require_device()
    cfg = (config or ChunkConfig()).to_c()
    stream = stream or torch.cuda.current_stream()
    k = len(tensors)
    tasks = (G.EncodeTask * max(k, 1))()
    names = []; caps = []
    verify = bool(cfg.flags & G.CFG_VERIFY) or os.environ.get("PCO_GFX_VERIFY", "")[:1] == "1"   # (the library reads the variable too)
    for t in tensors:
        if t.dim() != 1 or not t.is_contiguous() or not t.is_cuda:
            raise TypeError("every tensor must be a contiguous 1-D device tensor")
        if not 1 <= t.numel() <= 1 << 24:
            raise ValueError("a standalone chunk holds 1 ..= 2^24 numbers")
        names.append(_dtype_name(t))
        # (a verified encode asks for the documented 16 bytes behind the guarantee, which the decode behind it may read)
        caps.append((L.pco_gfx_guarantee_chunk_size(t.numel(), G.DTYPE_BYTE[names[-1]]) + (16 if verify else 0) + 15) // 16 * 16)
    header = b""
    if file_frame:
        buf = (C.c_uint8 * 64)()
        uniform = G.DTYPE_BYTE[names[0]] if names and len(set(names)) == 1 else 0
        header = bytes(buf[: L.pco_gfx_write_standalone_header(buf, 64, sum(t.numel() for t in tensors), uniform)])
    slot_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    with torch.cuda.stream(stream):
        slots = torch.empty(int(slot_off[-1]) + 64, dtype=torch.uint8, device="cuda")
        d_results = torch.empty(max(k, 1) * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
        offsets = torch.empty(k + 1, dtype=torch.int64, device="cuda")
        frame = len(header) + (1 if file_frame else 0)
        cap = frame + int(slot_off[-1]) if blob_cap is None else int(blob_cap)
        if cap < frame:
            raise ValueError("blob_cap is smaller than the file's frame")
        blob = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")   # (64 bytes of slack behind the capacity: the decoders may read 16 past a stream's end)
        host_header = torch.frombuffer(bytearray(header), dtype=torch.uint8) if header else None   # (kept until the stream has drained)
        if header:
            blob[: len(header)].copy_(host_header, non_blocking=True)
    for i, t in enumerate(tensors):
        tasks[i] = G.EncodeTask(t.data_ptr(), t.numel(), slots.data_ptr() + int(slot_off[i]), caps[i], G.DTYPE_BYTE[names[i]], 0)
    if d_specs is None:
        G.check(L.pco_gfx_compress_chunks(k, tasks, C.addressof(cfg), None, d_results.data_ptr(), stream.cuda_stream))
    else:
        G.check(L.pco_gfx_compress_chunks_specs(k, tasks, C.addressof(cfg), d_specs, None, d_results.data_ptr(), stream.cuda_stream))
    G.check(L.pco_gfx_compact_chunks(k, tasks, d_results.data_ptr(), blob.data_ptr(), cap - (1 if file_frame else 0), len(header), offsets.data_ptr(), None, stream.cuda_stream))
    if file_frame:   # the terminator behind the last chunk, placed on the device; the compactor's "destination too small" (an end of ~0) puts it into the slack
        with torch.cuda.stream(stream):
            end = offsets[-1:]
            blob.index_fill_(0, torch.where(end < 0, torch.full_like(end, cap), end), 0)
    out = CompressedStandaloneChunks(blob, offsets, d_results[: k * RESULT_DT.itemsize], [t.numel() for t in tensors], names, len(header), stream, (slots, tensors, host_header))
    out._tasks, out._blob_cap = tasks, cap
    return out


def verify_chunks(tensors, compressed, stream=None):
    """Verify what compress_chunks / compress_standalone_chunks wrote against `tensors` (the numbers, still on the device; one per chunk, in the
    encode's order): every chunk is decoded again from the encoder's slots (`compressed.slots`, so before `directory` / `total` let them go) through
    pco_gfx_verify_wrapped_chunks / pco_gfx_verify_chunks, the verdicts replace the encode's in place, and the chunks are compacted once more, so that
    a chunk that does not read back to its numbers is dropped from `compressed.blob` like one that failed to encode.  Asynchronous on `stream`
    (default: the stream of the encode).  Returns `compressed.verified`."""
    import torch
    L = _require_device()
    tensors = list(tensors)
    if compressed._keep is None or compressed._tasks is None:
        raise ValueError("verify_chunks needs the encoder's slots: call it before `directory`, `total` or `file` is read")
    standalone = isinstance(compressed, CompressedStandaloneChunks)
    k = len(compressed.ns) if standalone else len(compressed._ppc)
    if len(tensors) != k:
        raise ValueError("verify_chunks needs one tensor per chunk")
    stream = stream or compressed._stream or torch.cuda.current_stream()
    tasks = (type(compressed._tasks[0]) * max(k, 1))()
    for i, t in enumerate(tensors):
        if t.dim() != 1 or not t.is_contiguous() or not t.is_cuda or _dtype_name(t) != compressed.dtypes[i] or t.numel() != compressed._tasks[i].n:
            raise TypeError("every tensor must be a contiguous 1-D device tensor of its chunk's type and length")
        C.memmove(C.addressof(tasks[i]), C.addressof(compressed._tasks[i]), C.sizeof(tasks[i]))
        tasks[i].src = t.data_ptr()
    if standalone:
        d_res = compressed.results.data_ptr()
        G.check(L.pco_gfx_verify_chunks(k, tasks, d_res, None, d_res, stream.cuda_stream))
        frame_end = 1 if compressed.header_len else 0
        G.check(L.pco_gfx_compact_chunks(k, tasks, d_res, compressed.blob.data_ptr(), compressed._blob_cap - frame_end, compressed.header_len,
                                         compressed.offsets.data_ptr(), None, stream.cuda_stream))
        if frame_end:   # (the terminator behind the new end, as compress_standalone_chunks places it)
            with torch.cuda.stream(stream):
                end = compressed.offsets[-1:]
                compressed.blob.index_fill_(0, torch.where(end < 0, torch.full_like(end, compressed._blob_cap), end), 0)
    else:
        d_infos = compressed._d_infos.data_ptr()
        G.check(L.pco_gfx_verify_wrapped_chunks(k, tasks, C.addressof(compressed._cfg), d_infos, None, d_infos, stream.cuda_stream))
        G.check(L.pco_gfx_compact_wrapped_chunks(k, tasks, C.addressof(compressed._cfg), d_infos, compressed.gap, compressed.blob.data_ptr(), compressed.blob.numel(), 0,
                                                 compressed.offsets.data_ptr(), None, stream.cuda_stream))
    compressed._keep = compressed._keep + (tensors,)
    return compressed.verified


def _dir_source(compressed):
    """The page source of what a compress function returned: wrapped chunks by piece pair, standalone chunks by piece."""
    return _DirChunks(compressed) if isinstance(compressed, CompressedStandaloneChunks) else _DirPages(compressed)


PageCursors = namedtuple("PageCursors", "chunk piece every_rows cursors")   # cursors: uint8 device tensor [k, 256]; row i stands in front of row (i + 1) * every_rows


def _cursor(cursors, i):
    """The address of cursor i of a [k, 256] cursor tensor.  The cursor in front of row s * every_rows of a page is cursor s - 1 of its
    PageCursors: None, the page's start, for s = 0."""
    return None if i < 0 else cursors.data_ptr() + i * G.CURSOR_BYTES


def _saved(cursors):
    return {(pc.chunk, pc.piece): pc for pc in (PageCursors(*x) for x in cursors)}


def _saved_histories(cursors, histories):
    """histories (a list parallel to `cursors`: a [k, stride] uint8 device tensor or None per page, PageIndex.histories) by (chunk, piece)."""
    cursors = list(cursors); histories = list(histories)
    if len(histories) != len(cursors):
        raise ValueError("histories needs one entry per PageCursors")
    return {(pc.chunk, pc.piece): h for pc, h in zip((PageCursors(*x) for x in cursors), histories)}


def _segment_task(src, c, i, dst, first, count, pc, s, hists):
    """The task that reads rows [first, first + count) of page i of chunk c from cursor s - 1 of its PageCursors `pc` (s = 0, or no pc: the page's
    start).  hists None: a read task.  Else (_saved_histories) a read task with a history: history s - 1 of the page's, where it has any and s > 0,
    and to = None, which leaves the pair as it is -- an index stays reusable."""
    from_ = _cursor(pc and pc.cursors, s - 1)
    if hists is None:
        return src.read_task(c, i, dst, first, count, from_, None)
    h = hists.get((c, src.piece[c][i])) if s > 0 else None
    if h is None:
        return src.read_hist_task(c, i, dst, first, count, from_, None, None, 0)
    return src.read_hist_task(c, i, dst, first, count, from_, None, h.data_ptr() + (s - 1) * h.shape[1], h.shape[1])


# Outputs and task lists (arithmetic over a source and the addresses torch hands out), and the one way to the library.
_width = functools.lru_cache(maxsize=None)(lambda name: np.dtype(name).itemsize)


def _alloc(torch, n, name):
    """Room for n numbers of type `name` on the device and 64 bytes behind them, under the current stream: (uint8 tensor, n, name, width)."""
    width = _width(name)
    return torch.empty(n * width + 64, dtype=torch.uint8, device="cuda"), n, name, width


def _views(torch, outs, d_results=None):
    """The outputs as tensors of their types; with the device results of an asynchronous call, (tensors, results)."""
    tensors = [raw[: n * width].view(getattr(torch, name)) for raw, n, name, width in outs]
    return tensors if d_results is None else (tensors, d_results)


def _whole_chunks(torch, src, stream, saved=None, hists=None):
    """One output per chunk of `src` and the tasks that fill it page after page: (outs, tasks).  Without `saved`, one page task per page; with
    `saved` (_saved(cursors)), every page is cut at its saved cursors into read tasks, each starting from the cursor in front of its rows -- with
    `hists` (_saved_histories) beside its history (_segment_task)."""
    outs = []; tasks = []
    with torch.cuda.stream(stream):
        for c, ns in sorted(src.ns.items()):
            out = _alloc(torch, sum(ns), src.dtypes[c]); outs.append(out)
            dst, width = out[0].data_ptr(), out[3]
            for i, n in enumerate(ns):
                if saved is None:
                    tasks.append(src.page_task(c, i, dst))
                else:
                    pc = saved.get((c, src.piece[c][i]))
                    every = pc.every_rows if pc is not None and pc.cursors.shape[0] else n
                    tasks += [_segment_task(src, c, i, dst + row * width, row, min(every, n - row), pc, s, hists) for s, row in enumerate(range(0, n, every))]
                dst += n * width
    return outs, tasks


def _rows_of_chunks(torch, src, rows, stream, saved=None, hists=None):
    """One output per chunk c with rows[c] = (start, stop) and one task for every page the interval touches (map_rows_to_pages): (outs, tasks).
    Without `saved`, range tasks; with it, read tasks that start from the last saved cursor at or in front of their first row, with `hists` beside
    that cursor's history."""
    outs = []; tasks = []
    with torch.cuda.stream(stream):
        for c, want in enumerate(rows):
            if want is None:
                continue
            start, stop = int(want[0]), int(want[1])
            name = src.dtypes[c]
            parts = map_rows_to_pages(src.ns.get(c, []), start, stop)
            out = _alloc(torch, stop - start, name); outs.append(out)
            dst, width = out[0].data_ptr(), out[3]
            for i, first, count, at in parts:
                if saved is None:
                    tasks.append(src.range_task(c, i, dst + at * width, first, count))
                else:
                    pc = saved.get((c, src.piece[c][i]))
                    s = min(first // pc.every_rows, pc.cursors.shape[0]) if pc is not None else 0   # cursor s - 1 stands in front of row s * every_rows
                    tasks.append(_segment_task(src, c, i, dst + at * width, first, count, pc, s, hists))
    return outs, tasks


_ENTRY_POINT = {G.PageTask: "pco_gfx_decompress_pages", G.PageRangeTask: "pco_gfx_decompress_page_ranges", G.PageReadTask: "pco_gfx_decompress_page_reads",
                G.PageReadHistTask: "pco_gfx_decompress_page_reads_hist",   # (always with flags: 0 without `general`)
                G.PageIndexTask: "pco_gfx_index_pages", G.PageIndexHistTask: "pco_gfx_index_pages_hist", G.DirPageTask: "pco_gfx_decompress_pages_dir", G.DirPageRangeTask: "pco_gfx_decompress_page_ranges_dir",
                G.DirPageReadTask: "pco_gfx_decompress_page_reads_dir", G.DirPageIndexTask: "pco_gfx_index_pages_dir",   # (section 4k: the directory, then the flags)
                G.DirChunkTask: "pco_gfx_decompress_chunks_dir", G.DirChunkReadTask: "pco_gfx_decompress_chunk_reads_dir", G.DirChunkIndexTask: "pco_gfx_index_chunks_dir"}   # (section 4l)
_WITH_FLAGS = (G.PageReadHistTask, G.PageIndexHistTask, G.DirPageReadTask, G.DirPageIndexTask, G.DirChunkReadTask, G.DirChunkIndexTask)


def _launch(torch, L, kind, tasks, stream, results=None, directory=None, general=False):
    """The one library call of a list of `kind` tasks.  results None: they come to the host, so the call synchronises `stream` and a failing task
    raises.  results "empty" / "zeros": the asynchronous form; they go to a device tensor of RESULT_DT records that this torch function allocates
    and that is returned.  `directory`: the PcoGfxDirectory of the _dir entry points.  `general` (read and index tasks): the _ex entry point with
    PCO_GFX_CURSOR_GENERAL, under which Conv1, Dict and wide-table pages write and accept full-state cursors (include/pco_gfx.h section 4h).  Read tasks
    with a history (section 4i) go through pco_gfx_decompress_page_reads_hist, index tasks with histories (4j) through pco_gfx_index_pages_hist, and the
    read and index tasks of a device directory (4k) through their _dir entry points: their flags argument carries `general`."""
    n = len(tasks)
    arr = (kind * max(n, 1))(*tasks)
    host = d_results = None
    if results is None:
        host = (G.TaskResult * max(n, 1))()
    else:
        with torch.cuda.stream(stream):
            d_results = getattr(torch, results)(max(n, 1) * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    behind_tasks = () if directory is None else (C.addressof(directory),)
    if kind in _WITH_FLAGS:
        name, flags = _ENTRY_POINT[kind], (G.CURSOR_GENERAL if general else 0,)
    else:
        name, flags = (_ENTRY_POINT[kind] + "_ex", (G.CURSOR_GENERAL,)) if general else (_ENTRY_POINT[kind], ())
    G.check(getattr(L, name)(n, arr, *behind_tasks, *flags, host, None if results is None else d_results.data_ptr(), stream.cuda_stream))
    return None if results is None else d_results[: n * RESULT_DT.itemsize]


def _call(stream):
    """(torch, the library, the stream) of a call: what every public function starts with."""
    import torch
    return torch, _require_device(), stream or torch.cuda.current_stream()


# Whole pages and row ranges (include/pco_gfx.h sections 4b, 4d, 4e).
def _decompress_chunks(torch, L, src, stream):
    outs, tasks = _whole_chunks(torch, src, stream)
    return _views(torch, outs, _launch(torch, L, src.PAGE, tasks, stream, src.results, src.directory))


def _decompress_rows(torch, L, src, rows, stream):
    outs, tasks = _rows_of_chunks(torch, src, rows, stream)
    return _views(torch, outs, _launch(torch, L, src.RANGE, tasks, stream, src.results, src.directory))


def decompress_chunks(blob, directory, dtypes, stream=None):
    """Decode every page of `directory` (CompressedChunks.directory, or the same tuples read from a file's footer) out of the device tensor `blob`
    through one pco_gfx_decompress_pages call.  `dtypes`: a numpy dtype name per chunk.  Returns one device tensor per chunk (raw bytes viewed
    as the chunk's dtype).  Synchronises `stream`."""
    torch, L, stream = _call(stream)
    return _decompress_chunks(torch, L, _BlobPages(blob, directory, dtypes), stream)


def decompress_rows(blob, directory, dtypes, rows, stream=None):
    """Rows of the chunks in `blob` without decoding the rest of their pages: `rows[c]` is (start, stop) in chunk c's row coordinates, or None to
    skip the chunk.  Every interval is mapped onto the pages it touches (map_rows_to_pages) and all of them go through ONE
    pco_gfx_decompress_page_ranges call, which walks each page only as far as its last wanted row.  Returns one device tensor of stop - start
    rows per requested chunk, in chunk order.  Synchronises `stream`."""
    torch, L, stream = _call(stream)
    return _decompress_rows(torch, L, _BlobPages(blob, directory, dtypes), rows, stream)


def decompress_chunks_async(compressed, stream=None):
    """Decode every page of a CompressedChunks through ONE asynchronous pco_gfx_decompress_pages_dir call: the page directory is read where
    compress_chunks left it, on the device, so nothing here synchronises and `compressed.directory` is never touched.  Returns (tensors,
    results): one device tensor per chunk, and a device tensor of PcoGfxTaskResult records (RESULT_DT), one per page in chunk-then-page order.
    Both are valid in `stream`'s order; a chunk the writer dropped shows as PCO_GFX_INSUFFICIENT_DATA in its pages' results."""
    torch, L, stream = _call(stream)
    return _decompress_chunks(torch, L, _dir_source(compressed), stream)


def decompress_rows_async(compressed, rows, stream=None):
    """decompress_rows from the device directory: `rows[c]` is (start, stop) in chunk c's row coordinates, or None to skip the chunk; every
    interval goes through map_rows_to_pages and all of them through ONE asynchronous pco_gfx_decompress_page_ranges_dir call.  Returns (tensors,
    results) as decompress_chunks_async does, one tensor of stop - start rows per requested chunk and one result per page range, in task order.
    Never synchronises, never touches `compressed.directory`."""
    torch, L, stream = _call(stream)
    return _decompress_rows(torch, L, _dir_source(compressed), rows, stream)


# Reading a page in slices, and from saved cursors (include/pco_gfx.h sections 4f, 4g).
def _page_cursors(torch, src, every_rows, stream, out):
    """What save_cursors and the index functions share: `every_rows` validated, and one zeroed PageCursors per page of the page source `src` appended
    to `out` in chunk-then-page order.  Returns (every_rows, src, [(chunk, page index, the page's cursor count)] in out's order)."""
    every_rows = int(every_rows)
    if every_rows <= 0 or every_rows % 256:
        raise ValueError("every_rows must be a positive multiple of 256")
    src_pages = [(c, i, max((n - 1) // every_rows, 0)) for c, ns in sorted(src.ns.items()) for i, n in enumerate(ns)]
    with torch.cuda.stream(stream):
        for c, i, k in src_pages:
            out.append(PageCursors(c, src.piece[c][i], every_rows, torch.zeros((k, G.CURSOR_BYTES), dtype=torch.uint8, device="cuda")))
    return every_rows, src, src_pages


class ChunkReader:
    """The rows of one chunk of `blob`, slice after slice: read(n_rows) returns the chunk's next n_rows as a device tensor, crossing pages, and
    keeps one PcoGfxPageCursor per page in a device tensor, so that a read costs the batches it covers and not the page's prefix (pages whose
    cursors are position-only -- Lookback, and without `general` Conv1, Dict and wide tables -- are decoded from their start each time: same rows,
    more work).  n_rows is a multiple of 256 or reaches the chunk's end: the rule of the reference's PageDecompressor::read.  `general`: every
    read goes through pco_gfx_decompress_page_reads_ex with PCO_GFX_CURSOR_GENERAL.  `history`: a chunk under a Lookback delta gets one history
    buffer per page beside its cursor (sized by pco_gfx_lookback_history_bytes from the ChunkMeta's window_n_log) and every read goes through
    pco_gfx_decompress_page_reads_hist, so that a read of such a page costs the batches it covers too (include/pco_gfx.h section 4i); the planner
    below keeps a cursor only at batch boundaries, which is exactly when the library moves the history.  Each read synchronises `stream`."""

    def __init__(self, blob, directory, dtypes, chunk, stream=None, general=False, history=False):
        self._torch, self._L, self._stream = _call(stream)
        self._general = bool(general)
        self._hist_len, self.histories = 0, None
        self._src, self._chunk = _BlobPages(blob, directory, dtypes), chunk
        self._src.metas[chunk]   # (KeyError for a chunk the directory does not have)
        self._page_ns = self._src.ns.get(chunk, [])
        self.n = sum(self._page_ns); self.pos = 0
        with self._torch.cuda.stream(self._stream):
            self.cursors = self._torch.zeros((max(len(self._page_ns), 1), G.CURSOR_BYTES), dtype=self._torch.uint8, device="cuda")
        self._cur_row = [0] * len(self._page_ns)   # the row each page's cursor stands in front of; 0: no cursor yet
        if history:
            self._hist_len = self._history_bytes(blob, dtypes[chunk])
            if self._hist_len:   # (one row per page, each a multiple of 8 bytes: the library wants a history 8-byte aligned)
                with self._torch.cuda.stream(self._stream):
                    self.histories = self._torch.zeros((max(len(self._page_ns), 1), (self._hist_len + 7) // 8 * 8), dtype=self._torch.uint8, device="cuda")
        self._kind = G.PageReadHistTask if history else G.PageReadTask

    def _history_bytes(self, blob, name):
        """The bytes of one page's history: 0 unless the chunk's delta encoding is Lookback (pco_gfx_chunk_meta_info on the ChunkMeta's bytes)."""
        return self._src.history_bytes(self._L, blob, self._chunk)

    def _task(self, page_idx, first, count, dst, keep):
        cur = _cursor(self.cursors, page_idx)
        from_, to = cur if self._cur_row[page_idx] else None, cur if keep else None
        if self._kind is G.PageReadTask:
            return self._src.read_task(self._chunk, page_idx, dst, first, count, from_, to)
        hist = self.histories.data_ptr() + page_idx * self.histories.shape[1] if self.histories is not None else None
        return self._src.read_hist_task(self._chunk, page_idx, dst, first, count, from_, to, hist, self._hist_len if hist else 0)

    def read(self, n_rows):
        torch = self._torch
        n_rows = int(n_rows)
        if n_rows < 0 or n_rows > self.n - self.pos or (n_rows % 256 and n_rows != self.n - self.pos):
            raise ValueError(f"read({n_rows}): a multiple of 256 rows, or the {self.n - self.pos} rows that reach the chunk's end")
        with torch.cuda.stream(self._stream):
            out = _alloc(torch, n_rows, self._src.dtypes[self._chunk])
        base, width = out[0].data_ptr(), out[3]
        first_call = []; second_call = []; moved = []
        for page_idx, first, count, at in map_rows_to_pages(self._page_ns, self.pos, self.pos + n_rows):
            end, page_n, dst = first + count, self._page_ns[page_idx], base + at * width
            floor = end // 256 * 256
            if end == page_n or end == floor:      # the cursor the read leaves stands at its end
                first_call.append(self._task(page_idx, first, count, dst, True)); moved.append((page_idx, end))
            elif floor <= first:                    # inside one batch: the cursor stays in front of it
                first_call.append(self._task(page_idx, first, count, dst, False))
            else:                                   # up to the last batch boundary, then the rest from the cursor that leaves
                first_call.append(self._task(page_idx, first, floor - first, dst, True)); moved.append((page_idx, floor))
                second_call.append((page_idx, floor, end - floor, dst + (floor - first) * width))
        _launch(torch, self._L, self._kind, first_call, self._stream, general=self._general)
        for page_idx, row in moved:
            self._cur_row[page_idx] = row
        if second_call:
            _launch(torch, self._L, self._kind, [self._task(*t, False) for t in second_call], self._stream, general=self._general)
        self.pos += n_rows
        return _views(torch, [out])[0]


def save_cursors(blob, directory, dtypes, every_rows, stream=None, general=False):
    """Walk every page of `directory` once, in slices of `every_rows` (a multiple of 256), and keep the cursor in front of every slice but the
    first: [PageCursors(chunk, piece, every_rows, cursors)] in chunk-then-page order, for decompress_chunks_from.  One call per slice index over
    all pages; the rows themselves go to a scratch tensor and are dropped.  `general`: through pco_gfx_decompress_page_reads_ex with
    PCO_GFX_CURSOR_GENERAL -- full-state cursors for Conv1, Dict and wide-table pages too, to be read under the same flag."""
    torch, L, stream = _call(stream)
    out = []
    every_rows, src, src_pages = _page_cursors(torch, _BlobPages(blob, directory, dtypes), every_rows, stream, out)
    with torch.cuda.stream(stream):
        scratch = torch.empty(max(len(out), 1) * every_rows * 8 + 64, dtype=torch.uint8, device="cuda")
    for s in range(max((k for _, _, k in src_pages), default=0)):
        _launch(torch, L, G.PageReadTask, [src.read_task(c, i, scratch.data_ptr() + j * every_rows * 8, s * every_rows, every_rows,
                                                         _cursor(pc.cursors, s - 1), _cursor(pc.cursors, s))
                                           for j, (pc, (c, i, k)) in enumerate(zip(out, src_pages)) if s < k], stream, general=general)
    return out


class PageIndex(list):
    """What index_pages returns: the [PageCursors] save_cursors returns, and `results`: a device tensor of PcoGfxTaskResult records (RESULT_DT), one
    per page in the list's order, valid in the call's stream order like the cursors themselves (n_out = the page's cursor count on status 0).
    `histories` (index_pages(history=True), else None): a list parallel to the PageCursors -- per page a uint8 device tensor [k, stride], history i
    beside cursor i, or None for a page of a chunk without Lookback."""
    results = None
    histories = None


def index_pages(blob, directory, dtypes, every_rows, stream=None, general=False, history=False):
    """save_cursors through ONE asynchronous pco_gfx_index_pages call (include/pco_gfx.h section 4g): every page of `directory` is walked once, as
    far as its last cursor, and no rows are decoded.  Returns the same [PageCursors], byte for byte, valid in `stream`'s order; nothing here
    synchronises, so a page that fails shows in `.results`, not as an exception.  `general`: pco_gfx_index_pages_ex with PCO_GFX_CURSOR_GENERAL.
    `history`: through pco_gfx_index_pages_hist (section 4j) -- every page of a chunk under Lookback gets k histories beside its k cursors
    (`.histories`), which are kind 4 then: to be read with histories= by decompress_chunks_from / decompress_rows_from.  Each chunk's ChunkMeta is read
    back for its window first: the one synchronisation, in front of the call."""
    torch, L, stream = _call(stream)
    out = PageIndex()
    every_rows, src, src_pages = _page_cursors(torch, _BlobPages(blob, directory, dtypes), every_rows, stream, out)
    if history:
        stride = {c: (src.history_bytes(L, blob, c) + 7) // 8 * 8 for c in sorted(src.ns)}
        return _index_with_histories(torch, L, src, G.PageIndexHistTask, out, src_pages, every_rows, stride, stream, general)
    out.results = _launch(torch, L, G.PageIndexTask, [src.index_task(c, i, pc.cursors.data_ptr() if k else None, every_rows)
                                                      for pc, (c, i, k) in zip(out, src_pages)], stream, "zeros", general=general)
    return out


def _index_with_histories(torch, L, src, kind, out, src_pages, every_rows, stride, stream, general):
    """The index call with histories: per page of a chunk c with stride[c] != 0 a zeroed [k, stride[c]] tensor (`out.histories`), and ONE call of
    `kind` tasks."""
    with torch.cuda.stream(stream):
        out.histories = [torch.zeros((k, stride[c]), dtype=torch.uint8, device="cuda") if stride[c] else None for c, i, k in src_pages]
    tasks = [src.index_hist_task(c, i, pc.cursors.data_ptr() if k else None, every_rows, h.data_ptr() if h is not None and k else None,
                                 stride[c] if h is not None and k else 0) for pc, h, (c, i, k) in zip(out, out.histories, src_pages)]
    out.results = _launch(torch, L, kind, tasks, stream, "zeros", src.directory, general)
    return out


def decompress_rows_from(blob, directory, dtypes, cursors, rows, stream=None, general=False, histories=None):
    """decompress_rows with each page's task starting from the last saved cursor (save_cursors, index_pages) at or in front of its first row, not from
    the page's first batch: ONE pco_gfx_decompress_page_reads call whose tasks walk from their cursors to their last rows.  A page without saved
    cursors, or rows in front of its first one, is read from its start.  `general`: the flag the cursors were made under.  `histories`: the index's
    (PageIndex.histories) -- the call is pco_gfx_decompress_page_reads_hist then, and leaves cursors and histories as they are.  Synchronises `stream`."""
    torch, L, stream = _call(stream)
    hists = None if histories is None else _saved_histories(cursors, histories)
    outs, tasks = _rows_of_chunks(torch, _BlobPages(blob, directory, dtypes), rows, stream, _saved(cursors), hists)
    _launch(torch, L, G.PageReadTask if hists is None else G.PageReadHistTask, tasks, stream, general=general)
    return _views(torch, outs)


def decompress_chunks_from(blob, directory, dtypes, cursors, stream=None, general=False, histories=None):
    """decompress_chunks with every page cut at its saved cursors (save_cursors): all segments of all pages are tasks of ONE
    pco_gfx_decompress_page_reads call, each walking its own segment only -- a long page's tANS chain runs as many chains side by side as it has
    segments.  `general`: the flag the cursors were made under.  `histories`: the index's (PageIndex.histories), as decompress_rows_from takes them -- a
    Lookback page's segments then start from its kind-4 cursor / history pairs.  Returns one device tensor per chunk.  Synchronises `stream`."""
    torch, L, stream = _call(stream)
    hists = None if histories is None else _saved_histories(cursors, histories)
    outs, tasks = _whole_chunks(torch, _BlobPages(blob, directory, dtypes), stream, _saved(cursors), hists)
    _launch(torch, L, G.PageReadTask if hists is None else G.PageReadHistTask, tasks, stream, general=general)
    return _views(torch, outs)


# The same from the device directory (include/pco_gfx.h section 4k): encode -> compact -> index -> decode in one stream's order.
def index_pages_async(compressed, every_rows, stream=None, general=False, history=False):
    """index_pages from the directory as compress_chunks left it on the device: ONE asynchronous pco_gfx_index_pages_dir call, so that the cursors
    exist at write time.  Returns a PageIndex whose PageCursors have the keys and the bytes index_pages gives.  `history`: every page of every chunk
    gets k histories sized for the window a Lookback chunk of its row count gets (pco_gfx_lookback_window_n_log: host arithmetic, where index_pages
    reads the ChunkMeta back); the library leaves them alone on pages without Lookback, and the device refuses a stride that turns out too small.
    Never synchronises, never touches `compressed.directory`."""
    torch, L, stream = _call(stream)
    out = PageIndex()
    every_rows, src, src_pages = _page_cursors(torch, _dir_source(compressed), every_rows, stream, out)
    if history:
        stride = {c: (L.pco_gfx_lookback_history_bytes(L.pco_gfx_lookback_window_n_log(sum(ns)), G.DTYPE_BYTE[src.dtypes[c]]) + 7) // 8 * 8 for c, ns in src.ns.items()}
        return _index_with_histories(torch, L, src, src.INDEX, out, src_pages, every_rows, stride, stream, general)
    out.results = _launch(torch, L, src.INDEX, [src.index_task(c, i, pc.cursors.data_ptr() if k else None, every_rows)
                                                         for pc, (c, i, k) in zip(out, src_pages)], stream, "zeros", src.directory, general)
    return out


def _hists_of(index):
    return None if index.histories is None else _saved_histories(index, index.histories)


def decompress_chunks_from_async(compressed, index, stream=None, general=False):
    """decompress_chunks_from behind index_pages_async: every page cut at the index's cursors, all segments tasks of ONE asynchronous
    pco_gfx_decompress_page_reads_dir call, with `index.histories` beside the cursors when the index has them.  `general`: the flag the index was
    made under.  Returns (tensors, results) as decompress_chunks_async does, one result per segment in task order.  Never synchronises, never touches
    `compressed.directory`."""
    torch, L, stream = _call(stream)
    src = _dir_source(compressed)
    outs, tasks = _whole_chunks(torch, src, stream, _saved(index), _hists_of(index))
    return _views(torch, outs, _launch(torch, L, src.READ, tasks, stream, src.results, src.directory, general))


def decompress_rows_from_async(compressed, index, rows, stream=None, general=False):
    """decompress_rows_from behind index_pages_async: `rows[c]` is (start, stop) or None, and each page's task starts from the index's last cursor at
    or in front of its first row (and that cursor's history), in ONE asynchronous pco_gfx_decompress_page_reads_dir call.  Returns (tensors, results)
    as decompress_rows_async does.  Never synchronises, never touches `compressed.directory`."""
    torch, L, stream = _call(stream)
    src = _dir_source(compressed)
    outs, tasks = _rows_of_chunks(torch, src, rows, stream, _saved(index), _hists_of(index))
    return _views(torch, outs, _launch(torch, L, src.READ, tasks, stream, src.results, src.directory, general))


# Rows by row ids that live on the device (include/pco_gfx.h section 4n): filter -> take without a host round trip.
def _take(torch, L, src, rows, index, stream, results, general):
    """One output per chunk c with rows[c] a device tensor of chunk-relative row ids, and one take task per page of it, every page with row_base its
    first row in the chunk: the pages share the chunk's ids and its output, and each writes the entries it owns.  Returns (outs, [(first task, tasks,
    ids)] per wanted chunk, what _launch returned)."""
    saved = {} if index is None else _saved(index)
    outs = []; tasks = []; spans = []
    with torch.cuda.stream(stream):
        for c, want in enumerate(rows):
            if want is None:
                continue
            if not (want.is_cuda and want.dim() == 1 and want.is_contiguous() and want.dtype in (torch.int64, torch.uint64)):
                raise TypeError("rows[c] is a contiguous 1-D device tensor of int64 or uint64 row ids, or None")
            n = want.numel()
            out = _alloc(torch, n, src.dtypes[c]); outs.append(out)
            base = 0; spans.append((len(tasks), len(src.ns.get(c, [])), n))
            for i, page_n in enumerate(src.ns.get(c, [])):
                pc = saved.get((c, src.piece[c][i]))
                indexed = pc is not None and pc.cursors.shape[0] > 0
                tasks.append(G.TakeTask(*src.metas[c], *src.pages[c][i], page_n, base, pc.cursors.data_ptr() if indexed else None, pc.every_rows if indexed else 0,
                                        want.data_ptr() if n else None, n, out[0].data_ptr() if n else None, G.DTYPE_BYTE[src.dtypes[c]], 4))
                base += page_n
    n = len(tasks)
    arr = (G.TakeTask * max(n, 1))(*tasks)
    host = d_results = None
    if results is None:
        host = (G.TaskResult * max(n, 1))()
    else:
        with torch.cuda.stream(stream):
            d_results = torch.zeros(max(n, 1) * RESULT_DT.itemsize, dtype=torch.uint8, device="cuda")
    G.check(L.pco_gfx_take_rows(n, arr, G.CURSOR_GENERAL if general else 0, host, None if d_results is None else d_results.data_ptr(), stream.cuda_stream))
    return outs, spans, host if results is None else d_results[: n * RESULT_DT.itemsize]


def take_rows(blob, directory, dtypes, rows, index=None, stream=None, general=False):
    """The rows of the chunks in `blob` that device-resident row ids name: `rows[c]` is a device int64 / uint64 tensor of row ids in chunk c's row
    coordinates -- any order, duplicates allowed; what torch.nonzero of a filter's mask gives -- or None to skip the chunk.  `index`: what index_pages
    returned (made under the same `general`), or None.  ONE pco_gfx_take_rows call: every page is cut at its index's cursors, the device decides from
    the ids which segments are walked and how far, and only those are decoded.  Returns one device tensor per wanted chunk, out[j] = row rows[c][j].
    Raises IndexError when an id names no row of its chunk.  Lookback pages are taken without an index (section 4n).  Synchronises `stream` for
    the results; the ids are never read on the host."""
    torch, L, stream = _call(stream)
    outs, spans, res = _take(torch, L, _BlobPages(blob, directory, dtypes), rows, index, stream, None, general)
    for (first, n_pages, n), c in zip(spans, (c for c, want in enumerate(rows) if want is not None)):
        owned = sum(int(res[first + i].n_out) for i in range(n_pages))
        if owned < n:
            raise IndexError(f"{n - owned} of the {n} row ids of chunk {c} name no row of it")
    return _views(torch, outs)


def take_rows_async(compressed, rows, index=None, stream=None, general=False):
    """take_rows on what compress_chunks returned, through the asynchronous form: returns (tensors, results), the second a device tensor of
    PcoGfxTaskResult records (RESULT_DT), one per page of every wanted chunk in chunk-then-page order -- n_out the ids the page owned, aux the
    segments walked, consumed the batches walked.  The call makes no synchronisation and reads no id on the host; the tasks carry the pages'
    ADDRESSES (the _dir form of section 4n is not built), so `compressed.directory` is read first, which synchronises once if nobody has read it yet."""
    torch, L, stream = _call(stream)
    outs, _, d_results = _take(torch, L, _BlobPages(compressed.blob, compressed.directory, compressed.dtypes), rows, index, stream, "zeros", general)
    return _views(torch, outs, d_results)


# The chunk directory of standalone FILES, scanned on the device (include/pco_gfx.h section 4m): what a reader of .pco files that the reference's
# simple_compress or the pco CLI wrote starts with.
FileScan = namedtuple("FileScan", "offsets counts n_chunks version ns consumed")   # offsets: int64 device tensor [n_chunks + 1], file-relative; counts: uint32 device tensor [n_chunks]; ns: the counts on the host


def _to_host(t):
    """A device tensor's bytes on the host (synchronises the copy)."""
    return t.cpu().numpy()


class ScannedFiles:
    """What scan_files_async returns, valid in its stream's order: `blob` (uint8 device tensor: the files one behind the other, file i at
    blob[bases[i] : bases[i] + lens[i]]), `offsets[i]` (int64 device tensor of max_chunks + 1 entries: chunk k of file i starts at offsets[i][k],
    relative to the file's first byte, and the last chunk found ends at offsets[i][n_chunks]), `counts[i]` (uint32 device tensor: chunk k's n) and
    `results` (device tensor of RESULT_DT records: n_out = the file's chunk count, aux bits 8..15 its format version).  Entries beyond a file's chunks
    are not written.  `read()` is the only thing that synchronises."""

    def __init__(self, blob, bases, lens, dtypes, offsets, counts, small, stream, keep):
        self.blob, self.bases, self.lens, self.dtypes, self.offsets, self.counts = blob, bases, lens, dtypes, offsets, counts
        self.results = small[: len(bases) * RESULT_DT.itemsize]
        self._small, self._stream, self._keep = small, stream, keep

    def read(self):
        """[FileScan] per file, from ONE read-back of the results and the counts (synchronises); a file whose scan failed raises."""
        self._stream.synchronize()
        host = _to_host(self._small)
        k = len(self.bases)
        res = host[: k * RESULT_DT.itemsize].view(RESULT_DT)
        ns_all = host[k * RESULT_DT.itemsize:].view(np.uint32)
        out = []; at = 0
        for i in range(k):
            if int(res["status"][i]) != G.ST_OK:
                raise G.PcoGfxError(G.PcoDecompressionError, int(res["status"][i]), f"scan: file {i} failed behind {int(res['n_out'][i])} chunks")
            n = int(res["n_out"][i])
            out.append(FileScan(self.offsets[i][: n + 1], self.counts[i][:n], n, (int(res["aux"][i]) >> 8) & 0xFF, [int(x) for x in ns_all[at: at + n]], int(res["consumed"][i])))
            at += self.counts[i].shape[0]
        self._keep = None   # (the host copies of the files are no longer needed once the stream has drained)
        return out


def _scan_files(torch, L, blobs, dtype, max_chunks, stream):
    """The files staged into one device blob, each behind 64 bytes of slack, and ONE asynchronous pco_gfx_scan_chunks call over them."""
    blobs = list(blobs)
    names = [dtype] * len(blobs) if isinstance(dtype, str) else [str(d) for d in dtype]
    if len(names) != len(blobs) or any(nm not in G.DTYPE_BYTE for nm in names):
        raise TypeError("scan_files needs one number type name, or one per file")
    lens = [b.numel() if hasattr(b, "data_ptr") else len(b) for b in blobs]
    caps = [max(int(max_chunks), 1) if max_chunks is not None else n // 8 + 1 for n in lens]   # (a chunk is 4 preamble bytes and a ChunkMeta of 4 at the least)
    bases = []; total = 0
    for n in lens:
        bases.append(total); total += (n + 64 + 15) // 16 * 16
    k = len(blobs)
    keep = []
    with torch.cuda.stream(stream):
        blob = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
        all_offsets = torch.empty(sum(caps) + k, dtype=torch.int64, device="cuda")
        small = torch.empty(k * RESULT_DT.itemsize + sum(caps) * 4, dtype=torch.uint8, device="cuda")   # results, then every file's counts: one read-back
        for b, base, n in zip(blobs, bases, lens):
            if n == 0:
                continue
            if not hasattr(b, "data_ptr"):
                b = torch.frombuffer(bytearray(b), dtype=torch.uint8); keep.append(b)
            blob[base: base + n].copy_(b, non_blocking=True)
    offsets = []; counts = []; o_at = 0; c_at = k * RESULT_DT.itemsize
    tasks = []
    for base, n, cap, nm in zip(bases, lens, caps, names):
        offsets.append(all_offsets[o_at: o_at + cap + 1]); counts.append(small[c_at: c_at + cap * 4].view(torch.uint32))
        tasks.append(G.ScanTask(blob.data_ptr() + base, n, offsets[-1].data_ptr(), counts[-1].data_ptr(), cap, G.DTYPE_BYTE[nm], G.TASK_HAS_FILE_HEADER, 0))
        o_at += cap + 1; c_at += cap * 4
    arr = (G.ScanTask * max(k, 1))(*tasks)
    G.check(L.pco_gfx_scan_chunks(k, arr, None, small.data_ptr(), stream.cuda_stream))
    return ScannedFiles(blob, bases, lens, names, offsets, counts, small, stream, keep)


def scan_files_async(blobs, dtype, max_chunks=None, stream=None):
    """Find the chunks of standalone .pco files on the device: every file of `blobs` (bytes, or a uint8 device tensor holding exactly the file) is
    staged into one device blob and ONE asynchronous pco_gfx_scan_chunks call walks them side by side, storing no rows.  `dtype`: a numpy dtype name for
    all files, or one per file.  `max_chunks`: the chunks looked for per file (default: as many as the file's length can hold).  Returns a ScannedFiles:
    device arrays only, nothing is read back."""
    torch, L, stream = _call(stream)
    return _scan_files(torch, L, blobs, dtype, max_chunks, stream)


def scan_files(blobs, dtype, max_chunks=None, stream=None):
    """scan_files_async, then its one read-back: [FileScan(offsets, counts, n_chunks, version, ns, consumed)] per file -- the device offsets and counts
    (a PcoGfxDirectory's d_offsets, and page_n per chunk), the chunk count and the format version.  Synchronises `stream`; a file that fails raises."""
    return scan_files_async(blobs, dtype, max_chunks, stream).read()


def decompress_files(blobs, dtype, stream=None):
    """Decode whole .pco files of many chunks: the scan, ONE read-back of the counts, then ONE pco_gfx_decompress_chunks_dir call that decodes every
    chunk of every file side by side into one contiguous device tensor per file.  Synchronises `stream`."""
    torch, L, stream = _call(stream)
    scanned = _scan_files(torch, L, blobs, dtype, None, stream)
    files = scanned.read()
    n_entries = sum(f.n_chunks + 1 for f in files)
    outs = []; tasks = []; piece = 0
    with torch.cuda.stream(stream):
        # one directory over the staged blob: file i's offsets moved by its base, its chunk k piece (chunks and files in front of it) + k
        combined = torch.empty(max(n_entries, 1), dtype=torch.int64, device="cuda")
        for f, base, name in zip(files, scanned.bases, scanned.dtypes):
            torch.add(f.offsets, base, out=combined[piece: piece + f.n_chunks + 1])
            out = _alloc(torch, sum(f.ns), name); outs.append(out)
            dst, width = out[0].data_ptr(), out[3]
            for k, n in enumerate(f.ns):
                tasks.append(G.DirChunkTask(dst, n, piece + k, piece + k, G.DTYPE_BYTE[name], f.version))
                dst += n * width
            piece += f.n_chunks + 1
    if tasks:
        directory = G.Directory(scanned.blob.data_ptr(), scanned.blob.numel() - 64, combined.data_ptr(), n_entries - 1, 0, 0)
        _launch(torch, L, G.DirChunkTask, tasks, stream, None, directory)
    return _views(torch, outs)
