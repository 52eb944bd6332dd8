"""ctypes binding of libpco_gfx.so (the C ABI declared in include/pco_gfx.h).

The shared library is the product; this module only loads it.  There is no Python or CPU codec
behind it: if the library is missing, or no HIP device is visible, calls fail loudly.
"""
import ctypes as C
import os
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCO_GFX_LIB", os.path.join(HERE, "libpco_gfx.so"))  # override only for A/B experiments

PcoSuccess, PcoInvalidType, PcoCompressionError, PcoDecompressionError = range(4)
ST_OK, ST_CORRUPTION, ST_INSUFFICIENT_DATA, ST_INVALID_ARGUMENT, ST_UNSUPPORTED, ST_DEVICE_ERROR = range(6)
TASK_HAS_FILE_HEADER = 1

MODE_AUTO, MODE_CLASSIC, MODE_TRY_FLOAT_MULT, MODE_TRY_FLOAT_QUANT, MODE_TRY_INT_MULT, MODE_TRY_DICT = range(6)
DELTA_AUTO, DELTA_NOOP, DELTA_TRY_CONSECUTIVE, DELTA_TRY_LOOKBACK, DELTA_TRY_CONV1 = range(5)

CFG_STRICT_HISTOGRAM = 1  # PCO_GFX_CFG_STRICT_HISTOGRAM: replay the reference's quickselect histogram pivot by pivot
CFG_CONV1 = 2  # PCO_GFX_CFG_CONV1: encode DeltaSpec::TryConv1 (delta/conv1.rs) instead of refusing it
CFG_DICT = 4  # PCO_GFX_CFG_DICT: encode ModeSpec::TryDict (mode/dict.rs) instead of refusing it
CFG_VERIFY = 8  # PCO_GFX_CFG_VERIFY: decode every chunk again behind the encode and compare it with its source bit for bit
AUX_VERIFIED = 2  # PCO_GFX_AUX_VERIFIED in TaskResult.aux / PageInfo.aux: the bytes read back to the numbers

NumberType = namedtuple("NumberType", "byte name ref width")   # the type byte, numpy's name, the reference's name, bytes per number
NUMBER_TYPES = (NumberType(1, "uint32", "U32", 4), NumberType(2, "uint64", "U64", 8), NumberType(3, "int32", "I32", 4),
                NumberType(4, "int64", "I64", 8), NumberType(5, "float32", "F32", 4), NumberType(6, "float64", "F64", 8),
                NumberType(7, "uint16", "U16", 2), NumberType(8, "int16", "I16", 2), NumberType(9, "float16", "F16", 2),
                NumberType(10, "uint8", "U8", 1), NumberType(11, "int8", "I8", 1))   # pco_c/include/cpcodec.h:10-20: the one table
DTYPE_BYTE = {t.name: t.byte for t in NUMBER_TYPES}
DTYPE_BYTES = {t.byte: t.width for t in NUMBER_TYPES}
DTYPE_NAME = {t.byte: t.name for t in NUMBER_TYPES}       # np.dtype(name) and getattr(torch, name) are the array types
DTYPE_REF_NAME = {t.byte: t.ref for t in NUMBER_TYPES}
DTYPE_BYTE_OF_REF = {t.ref: t.byte for t in NUMBER_TYPES}


def dtype_byte(dtype):
    """The type byte of a number type given as the byte itself, a name ("float32"), a numpy dtype or scalar class, or a torch dtype."""
    if isinstance(dtype, int):
        return dtype
    name = getattr(dtype, "__name__", None) or str(dtype).rpartition(".")[2]
    return DTYPE_BYTE[name]


class PcoChunkConfig(C.Structure):  # pco_c/src/lib.rs:21-32
    _fields_ = [("compression_level", C.c_uint), ("max_page_n", C.c_size_t)]


class PcoChunkConfigEx(C.Structure):
    _fields_ = [("compression_level", C.c_uint32), ("mode_kind", C.c_uint32), ("mode_f64", C.c_double),
                ("mode_u64", C.c_uint64), ("delta_kind", C.c_uint32), ("delta_order", C.c_uint32),
                ("max_page_n", C.c_uint64), ("enable_8_bit", C.c_uint32), ("flags", C.c_uint32)]


class EncodeTask(C.Structure):
    _fields_ = [("src", C.c_void_p), ("n", C.c_uint64), ("dst", C.c_void_p), ("dst_cap", C.c_uint64),
                ("dtype", C.c_uint32), ("reserved", C.c_uint32)]


class DecodeTask(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_len", C.c_uint64), ("dst", C.c_void_p), ("dst_cap", C.c_uint64),
                ("dtype", C.c_uint32), ("flags", C.c_uint32)]


class ChunkSpec(C.Structure):   # PcoGfxChunkSpec: one chunk's resolved mode and delta (include/pco_gfx.h section 3c); mode_base / mode_inv of FloatMult are bit patterns in the number type
    _fields_ = [("mode_kind", C.c_uint32), ("delta_kind", C.c_uint32), ("delta_order", C.c_uint32), ("mode_k", C.c_uint32),
                ("mode_base", C.c_uint64), ("mode_inv", C.c_uint64), ("reserved", C.c_uint64)]

    def key(self):
        return (self.mode_kind, self.delta_kind, self.delta_order, self.mode_k, self.mode_base, self.mode_inv, self.reserved)

    def __eq__(self, other):
        return isinstance(other, ChunkSpec) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return "ChunkSpec(mode_kind=%d, delta_kind=%d, delta_order=%d, mode_k=%d, mode_base=%#x, mode_inv=%#x)" % self.key()[:6]


class TaskResult(C.Structure):
    _fields_ = [("n_out", C.c_uint64), ("consumed", C.c_uint64), ("status", C.c_uint32), ("aux", C.c_uint32)]


KIND_NAMES = {ST_CORRUPTION: "Corruption", ST_INSUFFICIENT_DATA: "InsufficientData", ST_INVALID_ARGUMENT: "InvalidArgument",
              ST_UNSUPPORTED: "Unsupported", ST_DEVICE_ERROR: "DeviceError"}


class PageInfo(C.Structure):   # PcoGfxPageInfo: one piece (ChunkMeta or page) of a chunk written by pco_gfx_compress_wrapped_chunks
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64), ("n", C.c_uint64), ("status", C.c_uint32), ("aux", C.c_uint32)]


class PageTask(C.Structure):   # PcoGfxPageTask: one wrapped page for pco_gfx_decompress_pages
    _fields_ = [("meta", C.c_void_p), ("meta_len", C.c_uint64), ("page", C.c_void_p), ("page_len", C.c_uint64),
                ("dst", C.c_void_p), ("page_n", C.c_uint64), ("dtype", C.c_uint32), ("format_major", C.c_uint32)]


class PageRangeTask(C.Structure):   # PcoGfxPageRangeTask: rows [first, first + count) of one wrapped page for pco_gfx_decompress_page_ranges
    _fields_ = [("meta", C.c_void_p), ("meta_len", C.c_uint64), ("page", C.c_void_p), ("page_len", C.c_uint64),
                ("dst", C.c_void_p), ("page_n", C.c_uint64), ("first", C.c_uint64), ("count", C.c_uint64),
                ("dtype", C.c_uint32), ("format_major", C.c_uint32)]


class PageCursor(C.Structure):   # PcoGfxPageCursor: 256 bytes of device memory, no pointers inside (include/pco_gfx.h section 4f)
    _fields_ = [("w", C.c_uint64 * 32)]


class PageReadTask(C.Structure):   # PcoGfxPageReadTask: PageRangeTask's fields, then the cursor to start from and the cursor to leave (device pointers or None)
    _fields_ = [("meta", C.c_void_p), ("meta_len", C.c_uint64), ("page", C.c_void_p), ("page_len", C.c_uint64),
                ("dst", C.c_void_p), ("page_n", C.c_uint64), ("first", C.c_uint64), ("count", C.c_uint64),
                ("dtype", C.c_uint32), ("format_major", C.c_uint32), ("from_", C.c_void_p), ("to", C.c_void_p)]


class PageReadHistTask(C.Structure):   # PcoGfxPageReadHistTask: PageReadTask's fields, then the page's lookback history buffer (device pointer or None) and its length (section 4i)
    _fields_ = PageReadTask._fields_ + [("history", C.c_void_p), ("history_len", C.c_uint64)]


class ChunkMetaInfo(C.Structure):   # PcoGfxChunkMetaInfo: what pco_gfx_chunk_meta_info reads back from a ChunkMeta's bytes
    _fields_ = [("mode_kind", C.c_uint32), ("mode_k", C.c_uint32), ("mode_base_latent", C.c_uint64), ("delta_kind", C.c_uint32), ("delta_order", C.c_uint32),
                ("window_n_log", C.c_uint32), ("state_n_log", C.c_uint32), ("secondary_uses_delta", C.c_uint32), ("n_vars_parsed", C.c_uint32),
                ("present", C.c_uint32 * 3), ("ans_size_log", C.c_uint32 * 3), ("n_bins", C.c_uint32 * 3), ("meta_bytes", C.c_uint64)]


class PageIndexTask(C.Structure):   # PcoGfxPageIndexTask: one wrapped page and where its cursors go, for pco_gfx_index_pages (section 4g)
    _fields_ = [("meta", C.c_void_p), ("meta_len", C.c_uint64), ("page", C.c_void_p), ("page_len", C.c_uint64),
                ("cursors", C.c_void_p), ("page_n", C.c_uint64), ("every_rows", C.c_uint64),
                ("dtype", C.c_uint32), ("format_major", C.c_uint32)]


class PageIndexHistTask(C.Structure):   # PcoGfxPageIndexHistTask: PageIndexTask's fields, then where the page's k histories go (device pointer or None) and their stride (section 4j)
    _fields_ = PageIndexTask._fields_ + [("histories", C.c_void_p), ("history_stride", C.c_uint64)]


CURSOR_BYTES = 256
CURSOR_VERSION, CURSOR_FULL, CURSOR_POSITION = 1, 1, 2
CURSOR_GENERAL_KIND = 3   # the full state of a page the general kernel decodes: written and accepted under CURSOR_GENERAL only (section 4h)
CURSOR_GENERAL = 1        # PCO_GFX_CURSOR_GENERAL, the flag of pco_gfx_decompress_page_reads_ex / pco_gfx_index_pages_ex
CURSOR_LOOKBACK_KIND = 4  # the tANS and bit state of a Lookback page read beside a history buffer: pco_gfx_decompress_page_reads_hist only (section 4i)
HISTORY_HEADER_BYTES = 64   # PCO_GFX_HISTORY_HEADER_BYTES: the stamp in front of a history buffer's ring


class Directory(C.Structure):   # PcoGfxDirectory: a compacted stream and its piece offsets, both on the device (include/pco_gfx.h section 4e)
    _fields_ = [("d_blob", C.c_void_p), ("blob_len", C.c_uint64), ("d_offsets", C.c_void_p), ("n_pieces", C.c_uint64),
                ("gap", C.c_uint32), ("reserved", C.c_uint32)]


class DirPageTask(C.Structure):   # PcoGfxDirPageTask: one wrapped page, named by piece index, for pco_gfx_decompress_pages_dir
    _fields_ = [("dst", C.c_void_p), ("page_n", C.c_uint64), ("meta_piece", C.c_uint32), ("page_piece", C.c_uint32),
                ("dtype", C.c_uint32), ("format_major", C.c_uint32)]


class DirPageRangeTask(C.Structure):   # PcoGfxDirPageRangeTask: rows [first, first + count) of such a page for pco_gfx_decompress_page_ranges_dir
    _fields_ = [("dst", C.c_void_p), ("page_n", C.c_uint64), ("first", C.c_uint64), ("count", C.c_uint64),
                ("meta_piece", C.c_uint32), ("page_piece", C.c_uint32), ("dtype", C.c_uint32), ("format_major", C.c_uint32)]


class DirPageReadTask(C.Structure):   # PcoGfxDirPageReadTask: DirPageRangeTask's fields, then PageReadHistTask's last four, for pco_gfx_decompress_page_reads_dir (section 4k)
    _fields_ = DirPageRangeTask._fields_ + [("from_", C.c_void_p), ("to", C.c_void_p), ("history", C.c_void_p), ("history_len", C.c_uint64)]


class DirPageIndexTask(C.Structure):   # PcoGfxDirPageIndexTask: one wrapped page, named by piece index, and where its cursors and histories go, for pco_gfx_index_pages_dir
    _fields_ = [("cursors", C.c_void_p), ("page_n", C.c_uint64), ("every_rows", C.c_uint64),
                ("meta_piece", C.c_uint32), ("page_piece", C.c_uint32), ("dtype", C.c_uint32), ("format_major", C.c_uint32),
                ("histories", C.c_void_p), ("history_stride", C.c_uint64)]


# Section 4l: the same three structs name STANDALONE chunks (meta_piece == page_piece == the chunk's piece).  Subclasses without fields of their own, so
# that pcodec_amd.paged's task lists say which entry point they are for.
class DirChunkTask(DirPageTask):
    pass


class DirChunkReadTask(DirPageReadTask):
    pass


class DirChunkIndexTask(DirPageIndexTask):
    pass


class ScanTask(C.Structure):   # PcoGfxScanTask: one standalone stream and where its chunk offsets and counts go, for pco_gfx_scan_chunks (section 4m)
    _fields_ = [("src", C.c_void_p), ("src_len", C.c_uint64), ("d_offsets", C.c_void_p), ("d_counts", C.c_void_p),
                ("max_chunks", C.c_uint32), ("dtype", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TakeTask(C.Structure):   # PcoGfxTakeTask: one wrapped page, its index and the device-resident row ids wanted of it, for pco_gfx_take_rows (section 4n)
    _fields_ = [("meta", C.c_void_p), ("meta_len", C.c_uint64), ("page", C.c_void_p), ("page_len", C.c_uint64),
                ("page_n", C.c_uint64), ("row_base", C.c_uint64), ("cursors", C.c_void_p), ("every_rows", C.c_uint64),
                ("d_rows", C.c_void_p), ("n_rows", C.c_uint64), ("dst", C.c_void_p), ("dtype", C.c_uint32), ("format_major", C.c_uint32)]


class WrappedTask(C.Structure):  # PcoGfxWrappedTask: one chunk for pco_gfx_compress_wrapped_chunks_ex / pco_gfx_compact_wrapped_chunks
    _fields_ = [("src", C.c_void_p), ("n", C.c_uint64), ("dst", C.c_void_p), ("dst_cap", C.c_uint64),
                ("dtype", C.c_uint32), ("n_pages", C.c_uint32), ("page_sizes", C.c_void_p)]   # page_sizes: HOST uint64[n_pages], NULL iff n_pages == 0


class AutoModeRecord(C.Structure):   # PcoGfxAutoModeRecord: one chunk of pco_gfx_debug_auto_mode (test hook: include/pco_gfx.h §6)
    _fields_ = [("route", C.c_uint32), ("n_entries", C.c_uint32), ("overflow", C.c_uint32), ("s_size", C.c_uint32),
                ("tz5", C.c_uint32), ("n_ints", C.c_uint32), ("n_gcd", C.c_uint32), ("has_euclid", C.c_uint32),
                ("sim", C.c_uint32 * 3), ("k", C.c_int32), ("cand_mask", C.c_uint32), ("bk", C.c_uint32), ("base_c", C.c_uint64),
                ("base", C.c_uint64 * 4), ("inv", C.c_uint64 * 4), ("s_int", C.c_int64 * 4), ("s_dbl", C.c_uint64 * 4)]


AUTO_DEBUG_MAX = 256   # PCO_GFX_AUTO_DEBUG_MAX


class AutoDeltaRecord(C.Structure):   # PcoGfxAutoDeltaRecord: one chunk of pco_gfx_debug_auto_delta (test hook: include/pco_gfx.h §6)
    _fields_ = [("sample_n", C.c_uint32), ("eval_mask", C.c_uint32), ("cost", C.c_float * 9),
                ("delta_kind", C.c_uint32), ("delta_order", C.c_uint32), ("window_n_log", C.c_uint32)]


class PcoGfxError(RuntimeError):
    """The reference's Python binding raises RuntimeError("pco error: pco <ErrorKind> error: <message>") (pco_python/src/utils.rs:78 over
    errors.rs:52-60): the same text here, so that callers (and the reference's own tests) that match on the kind keep working."""

    def __init__(self, code, status, msg):
        super().__init__(f"pco error: pco {KIND_NAMES.get(status, status)} error: {msg} (libpco_gfx code={code} status={status})")
        self.code, self.status = code, status


# Every function include/pco_gfx.h declares: (restype, argtypes), applied once by lib().  A pointer of any kind is c_void_p, so that byref(x),
# addressof(x), a ctypes array, an integer address and None all pass; tests/test_ctypes_signatures.py holds the table against the header.
_P, _Z, _B, _I, _U32, _U64 = C.c_void_p, C.c_size_t, C.c_ubyte, C.c_int, C.c_uint32, C.c_uint64
_COUNTER, _FREE, _SIZE_OF_HANDLE, _SIZE_OF_PAGE = (C.c_ulonglong, ()), (None, (_P,)), (_Z, (_P,)), (_Z, (_P, _Z))
_BATCH = (_I, (_Z, _P, _P, _P, _P))            # n_tasks, tasks, results, d_results, stream
_BATCH_WITH = (_I, (_Z, _P, _P, _P, _P, _P))   # ... with a config or a directory behind the tasks
SIGNATURES = {
    # 1. the reference's C ABI
    "pco_standalone_guarantee_file_size": (_Z, (_Z, _B)),
    "pco_standalone_simple_compress_into": (_I, (_P, _Z, _B, _P, _P, _Z, _P)),
    "pco_standalone_simple_decompress_into": (_I, (_P, _Z, _B, _P, _Z, _P)),
    # 2. the extended config
    "pco_gfx_last_status": (_I, ()), "pco_gfx_last_error": (C.c_char_p, ()), "pco_gfx_device_count": (_I, ()),
    "pco_gfx_simple_compress_into_ex": (_I, (_P, _Z, _B, _P, _I, _P, _Z, _P)),
    "pco_gfx_simple_compress_into_exact": (_I, (_P, _Z, _B, _P, _I, _P, _Z, _P, _Z, _P)),
    "pco_gfx_guarantee_file_size": (_Z, (_Z, _B, _U64)), "pco_gfx_guarantee_chunk_size": (_Z, (_Z, _B)),
    # 3. batched standalone chunks on device buffers
    "pco_gfx_compress_chunks": _BATCH_WITH, "pco_gfx_decompress_chunks": _BATCH,
    "pco_gfx_compact_chunks": (_I, (_Z, _P, _P, _P, _U64, _U64, _P, _P, _P)),
    # 3b. verified encodes: n_tasks, tasks, (config,) d_encoded, results, d_results, stream
    "pco_gfx_verify_chunks": _BATCH_WITH, "pco_gfx_verify_wrapped_chunks": (_I, (_Z, _P, _P, _P, _P, _P, _P)),
    # 3c. resolve once, encode from per-chunk specs: n_tasks, tasks, config, specs, (results | infos, d_results | d_infos,) stream
    "pco_gfx_resolve_chunk_specs": (_I, (_Z, _P, _P, _P, _P)), "pco_gfx_chunk_spec_from_meta": (_I, (_P, _Z, _B, _B, _P)),
    "pco_gfx_compress_chunks_specs": (_I, (_Z, _P, _P, _P, _P, _P, _P)), "pco_gfx_compress_wrapped_chunks_specs": (_I, (_Z, _P, _P, _P, _P, _P, _P)),
    "pco_gfx_write_standalone_header": (_Z, (_P, _Z, _U64, _B)), "pco_gfx_write_standalone_footer": (_Z, (_P, _Z)),
    "pco_gfx_release_workspace": (None, ()), "pco_gfx_workspace_bytes": (_Z, ()),
    "pco_gfx_strict_histogram_fallbacks": _COUNTER, "pco_gfx_trail_givebacks": _COUNTER, "pco_gfx_trail_marked": _COUNTER,
    "pco_gfx_profile_begin": (None, ()), "pco_gfx_profile_end": (_I, (_P, _Z, _P, _I)),
    # 4. the wrapped surface on host buffers
    "pco_wrapped_write_header": (_Z, (_P, _Z)), "pco_wrapped_read_header": (_I, (_P, _Z, _P, _P, _P)),
    "pco_chunk_compressor_new": (_I, (_P, _Z, _B, _P, _P)), "pco_chunk_compressor_new_exact": (_I, (_P, _Z, _B, _P, _P, _Z, _P)),
    "pco_chunk_compressor_n_pages": _SIZE_OF_HANDLE, "pco_chunk_compressor_page_n": _SIZE_OF_PAGE,
    "pco_chunk_compressor_meta_size": _SIZE_OF_HANDLE, "pco_chunk_compressor_page_size": _SIZE_OF_PAGE,
    "pco_chunk_compressor_meta_size_hint": _SIZE_OF_HANDLE, "pco_chunk_compressor_page_size_hint": _SIZE_OF_PAGE,
    "pco_chunk_compressor_write_meta": (_I, (_P, _P, _Z, _P)), "pco_chunk_compressor_write_page": (_I, (_P, _Z, _P, _Z, _P)),
    "pco_chunk_decompressor_new": (_I, (_P, _Z, _B, _B, _P, _P)),
    "pco_chunk_decompressor_read_page": (_I, (_P, _P, _Z, _Z, _P, _Z, _P, _P)),
    "pco_page_decompressor_new": (_I, (_P, _P, _Z, _Z, _P)), "pco_page_decompressor_read": (_I, (_P, _P, _Z, _P, _P)),
    "pco_page_decompressor_consumed": _SIZE_OF_HANDLE,
    "pco_chunk_compressor_free": _FREE, "pco_chunk_decompressor_free": _FREE, "pco_page_decompressor_free": _FREE,
    # 4b-4g. the wrapped surface, batched, on device buffers
    "pco_gfx_wrapped_n_pages": (_Z, (_Z, _U64)), "pco_gfx_wrapped_scratch_estimate": (_Z, (_Z, _P, _P)),
    "pco_gfx_wrapped_chunk_cap": (_Z, (_Z, _B, _P)), "pco_gfx_wrapped_chunk_cap_exact": (_Z, (_P, _Z, _B, _P)),
    "pco_gfx_compress_wrapped_chunks": _BATCH, "pco_gfx_compress_wrapped_chunks_ex": _BATCH_WITH,   # (a config and infos, not results)
    "pco_gfx_compact_wrapped_chunks": (_I, (_Z, _P, _P, _P, _U32, _P, _U64, _U64, _P, _P, _P)),
    "pco_gfx_decompress_pages": _BATCH, "pco_gfx_decompress_page_ranges": _BATCH, "pco_gfx_decompress_page_reads": _BATCH,
    "pco_gfx_decompress_pages_dir": _BATCH_WITH, "pco_gfx_decompress_page_ranges_dir": _BATCH_WITH,
    "pco_gfx_page_index_len": (_Z, (_U64, _U64)), "pco_gfx_index_pages": _BATCH,
    # 4h. ... with flags (PCO_GFX_CURSOR_GENERAL): n_tasks, tasks, flags, results, d_results, stream
    "pco_gfx_decompress_page_reads_ex": (_I, (_Z, _P, _U32, _P, _P, _P)), "pco_gfx_index_pages_ex": (_I, (_Z, _P, _U32, _P, _P, _P)),
    # 4i. ... with a history buffer per task; the bytes one takes
    "pco_gfx_decompress_page_reads_hist": (_I, (_Z, _P, _U32, _P, _P, _P)), "pco_gfx_lookback_history_bytes": (_Z, (_U32, _B)),
    # 4j. the index with k histories per task
    "pco_gfx_index_pages_hist": (_I, (_Z, _P, _U32, _P, _P, _P)),
    # 4k. 4i and 4j from the device directory: n_tasks, tasks, dir, flags, results, d_results, stream; the window a Lookback chunk of n numbers gets
    "pco_gfx_decompress_page_reads_dir": (_I, (_Z, _P, _P, _U32, _P, _P, _P)), "pco_gfx_index_pages_dir": (_I, (_Z, _P, _P, _U32, _P, _P, _P)),
    "pco_gfx_lookback_window_n_log": (_I, (_U64,)),
    # 4l. 4e's page form and 4k's two over standalone chunks; the same split on host bytes
    "pco_gfx_decompress_chunks_dir": _BATCH_WITH,
    "pco_gfx_decompress_chunk_reads_dir": (_I, (_Z, _P, _P, _U32, _P, _P, _P)), "pco_gfx_index_chunks_dir": (_I, (_Z, _P, _P, _U32, _P, _P, _P)),
    "pco_gfx_standalone_chunk_split": (_I, (_P, _Z, _B, _B, _P, _P, _P)),
    # 4m. the chunk directory of standalone files, scanned on the device
    "pco_gfx_scan_chunks": _BATCH,
    # 4n. rows by device-resident row ids: n_tasks, tasks, flags, results, d_results, stream
    "pco_gfx_take_rows": (_I, (_Z, _P, _U32, _P, _P, _P)),
    "pco_gfx_chunk_meta_info": (_I, (_P, _Z, _B, _B, _P)),
    "pco_chunk_compressor_meta_info": (_I, (_P, _B, _P)), "pco_chunk_decompressor_meta_info": (_I, (_P, _P)),
    "pco_gfx_chunk_meta_conv1": (_I, (_P, _Z, _B, _B, _P, _P, _P, _P)), "pco_gfx_chunk_meta_dict": (_I, (_P, _Z, _B, _B, _P, _P, _Z)),
    # 5. chunk-sharded files over RCCL
    "pco_gfx_comm_unique_id": (_I, (_P,)), "pco_gfx_comm_init": (_I, (_P, _I, _I, _P)), "pco_gfx_comm_free": _FREE,
    "pco_gfx_comm_rank": (_I, (_P,)), "pco_gfx_comm_size": (_I, (_P,)),
    "pco_gfx_gather_chunks": (_I, (_P, _I, _P, _U64, _P, _U64, _U64, _P, _P)),
    "pco_gfx_scatter_chunks": (_I, (_P, _I, _P, _U64, _P, _P, _U64, _P, _P)),
    # 6. test hooks
    "pco_gfx_debug_float_screen": (_I, (_P, _Z, _U32, _P)),
    "pco_gfx_debug_lookback_routes": (C.c_int64, (_P, _Z)), "pco_gfx_debug_auto_mode": (C.c_int64, (_P, _Z)),
    "pco_gfx_debug_histogram": (C.c_int64, (_U32, _U32, _P, _P, _P, _Z, _P)),
    "pco_gfx_debug_pack_routes": (C.c_int64, (_P, _Z)), "pco_gfx_debug_auto_delta": (C.c_int64, (_P, _Z)),
}

_lib = None


def lib():
    """Load libpco_gfx.so.  Raises if it has not been built (python -m pcodec_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m pcodec_amd.build` (needs hipcc). "
                              "pcodec_amd has no CPU fallback.")
        # When PyTorch-ROCm is used in the same process (device buffers for the batched API), load its HIP
        # runtime first so that both bind to ONE libamdhip64: two HIP runtimes in a process cannot both
        # open the device ("No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except Exception:  # torch is optional plumbing
            pass
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, list(argtypes)
        _lib = L
    return _lib


def check(code):
    if code != PcoSuccess:
        L = lib()
        raise PcoGfxError(code, L.pco_gfx_last_status(), (L.pco_gfx_last_error() or b"").decode())


def make_config(level=8, mode=MODE_AUTO, mode_f64=0.0, mode_u64=0, delta=DELTA_AUTO, delta_order=0, max_page_n=0,
                enable_8_bit=False, strict_histogram=False, conv1=False, dict=False, verify=False):
    return PcoChunkConfigEx(level, mode, mode_f64, mode_u64, delta, delta_order, max_page_n, 1 if enable_8_bit else 0,
                            (CFG_STRICT_HISTOGRAM if strict_histogram else 0) | (CFG_CONV1 if conv1 else 0) | (CFG_DICT if dict else 0) |
                            (CFG_VERIFY if verify else 0))


def chunk_meta_conv1(meta, dtype_byte, format_major=4):
    """(quantization, bias, weights) of a ChunkMeta's Conv1 delta encoding, read from its bytes; None when the delta encoding is not Conv1."""
    buf = (C.c_uint8 * max(len(meta), 1)).from_buffer_copy(bytes(meta) or b"\0")
    q, b, order, w = C.c_uint32(), C.c_int64(), C.c_uint32(), (C.c_int32 * 32)()
    check(lib().pco_gfx_chunk_meta_conv1(buf, len(meta), dtype_byte, format_major, C.byref(q), C.byref(b), w, C.byref(order)))
    return None if order.value == 0 else (q.value, b.value, list(w[:order.value]))


def chunk_meta_dict(meta, dtype_byte, format_major=4):
    """The dictionary of a Dict-mode ChunkMeta as a numpy array of ordered latents (unsigned, the number type's width); None when the mode is not Dict."""
    import numpy as np
    buf = (C.c_uint8 * max(len(meta), 1)).from_buffer_copy(bytes(meta) or b"\0")
    width = DTYPE_BYTES[dtype_byte]
    cap = max(len(meta) // width, 1)
    out = np.zeros(cap, dtype=f"u{width}")
    k = C.c_uint32()
    check(lib().pco_gfx_chunk_meta_dict(buf, len(meta), dtype_byte, format_major, C.byref(k), out.ctypes.data, cap))
    return None if k.value == 0 else out[:k.value].copy()
