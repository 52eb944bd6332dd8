/*
 * pco_gfx.h -- C ABI of libpco_gfx.so, the MI355X-native (gfx950, HIP) implementation of
 * pcodec's chunk encode / decode hot path.
 *
 * The library is a drop-in for that path only.  Section 1 is byte-compatible with the
 * reference's own C ABI (pco_c/include/cpcodec_generated.h, pco_c/include/cpcodec.h);
 * sections 2-4 are the entry points a `pco` FFI for this path would bind in addition:
 * the explicit mode/delta specs the reference C struct cannot express, a batched
 * many-chunk form operating on buffers already resident in HBM, and the wrapped
 * ChunkCompressor / ChunkDecompressor surface.  No torch / HIP types appear in any signature:
 * plain pointers and sizes only.  A `stream` argument is an opaque hipStream_t (NULL = the
 * default stream).
 *
 * Thread-safety: every function is re-entrant; the library keeps one lazily grown device
 * workspace per (thread, device) and no other state (cf. pco_c/src/lib.rs:57-70).
 */
#ifndef PCO_GFX_H
#define PCO_GFX_H

#include <stddef.h>
#include <stdint.h>

#if defined(__cplusplus)
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * 1. The reference C ABI, unchanged (replaces pco_c/src/lib.rs:128,146,178).
 * ---------------------------------------------------------------------------------------- */

/* number type bytes: pco_c/include/cpcodec.h:10-20, docs/format.md:205-217 */
#define PCO_TYPE_U32 1
#define PCO_TYPE_U64 2
#define PCO_TYPE_I32 3
#define PCO_TYPE_I64 4
#define PCO_TYPE_F32 5
#define PCO_TYPE_F64 6
#define PCO_TYPE_U16 7
#define PCO_TYPE_I16 8
#define PCO_TYPE_F16 9
#define PCO_TYPE_U8 10
#define PCO_TYPE_I8 11

typedef enum PcoError { /* pco_c/src/lib.rs:12-19 */
  PcoSuccess,
  PcoInvalidType,
  PcoCompressionError,
  PcoDecompressionError,
} PcoError;

typedef struct PcoChunkConfig { /* pco_c/src/lib.rs:21-32 */
  unsigned int compression_level; /* 0-12, default 8 */
  size_t max_page_n;              /* 0 => 2^18 */
} PcoChunkConfig;

/* pco_c/src/lib.rs:128-141 -> standalone/guarantee.rs:29-37 */
size_t pco_standalone_guarantee_file_size(size_t n, unsigned char dtype);

/* pco_c/src/lib.rs:146-173 -> standalone::simple_compress_into (standalone/simple.rs:22-48).
 * `nums` and `dst` are HOST buffers.  Config NULL => level 8, Auto mode, Auto delta,
 * enable_8_bit (pco_c/src/lib.rs:34-55). */
enum PcoError pco_standalone_simple_compress_into(const void* nums, size_t n, unsigned char dtype,
                                                  const struct PcoChunkConfig* config, void* dst,
                                                  size_t dst_cap, size_t* n_written);

/* pco_c/src/lib.rs:178-199 -> standalone::simple_decompress (standalone/simple.rs:149-152).
 * `dst_cap` and `*n_written` are in ELEMENTS.  A too-small dst is an error
 * (pco_c/src/lib.rs:110-112). */
enum PcoError pco_standalone_simple_decompress_into(const void* compressed, size_t compressed_len,
                                                    unsigned char dtype, void* dst, size_t dst_cap,
                                                    size_t* n_written);

/* ------------------------------------------------------------------------------------------
 * 2. Extended config: everything pco::ChunkConfig can say (chunk_config.rs:13-125,191-235).
 * ---------------------------------------------------------------------------------------- */

enum PcoModeSpecKind { /* chunk_config.rs:13-51 */
  PCO_MODE_AUTO = 0,
  PCO_MODE_CLASSIC = 1,
  PCO_MODE_TRY_FLOAT_MULT = 2,  /* mode_f64 = base */
  PCO_MODE_TRY_FLOAT_QUANT = 3, /* mode_u64 = k */
  PCO_MODE_TRY_INT_MULT = 4,    /* mode_u64 = base */
  PCO_MODE_TRY_DICT = 5,        /* needs PCO_GFX_CFG_DICT in `flags` (without it: PcoCompressionError, status PCO_GFX_UNSUPPORTED) */
};
enum PcoDeltaSpecKind { /* chunk_config.rs:61-109 */
  PCO_DELTA_AUTO = 0,
  PCO_DELTA_NOOP = 1,
  PCO_DELTA_TRY_CONSECUTIVE = 2, /* delta_order = order (0..7) */
  PCO_DELTA_TRY_LOOKBACK = 3,
  PCO_DELTA_TRY_CONV1 = 4,       /* delta_order = order (0..32); needs PCO_GFX_CFG_CONV1 in `flags` (without it: PcoCompressionError, status
                                    PCO_GFX_UNSUPPORTED); u8/u16/u32/i8/i16/i32/f16/f32 only */
};
typedef struct PcoChunkConfigEx {
  uint32_t compression_level; /* 0-12 */
  uint32_t mode_kind;         /* enum PcoModeSpecKind */
  double mode_f64;
  uint64_t mode_u64;
  uint32_t delta_kind;        /* enum PcoDeltaSpecKind */
  uint32_t delta_order;
  uint64_t max_page_n;        /* PagingSpec::EqualPagesUpTo; 0 => 2^18 */
  uint32_t enable_8_bit;
  uint32_t flags;             /* PCO_GFX_CFG_* bits; 0 = the reference's ChunkConfig and nothing else.  ZERO-INITIALISE the struct: bits
                                 this library does not know are rejected with PCO_GFX_INVALID_ARGUMENT (so that a later flag is never
                                 silently ignored by an older library, and an uninitialised word never silently turns a mode on) */
} PcoChunkConfigEx;
/* Strict histograms: replay the reference's quickselect (histograms.rs:208-280, sort_utils.rs) pivot by pivot on the device, so that
 * the chunk's bytes equal the reference's even on input ORDERS that send its histogram into the heapsort branch (histograms.rs:248-258),
 * the one place where the default (sort-free, order-independent) histogram kernels can differ from it.  Costs several passes over a
 * private copy of every latent variable; see DESIGN.md section 2 for when it matters (an order built against the pivot rule).
 * PCO_GFX_STRICT_HISTOGRAM=1 in the environment (read once, when the library is loaded) sets it for every call of the process -- for
 * callers of the reference's own three-function ABI, whose PcoChunkConfig has no field for it. */
#define PCO_GFX_CFG_STRICT_HISTOGRAM 1u
/* Conv1 delta encode: DeltaSpec::TryConv1(delta_order) behaves as in the reference (delta/conv1.rs choose_config / encode_in_place; chunk_config.rs:
 * 288-303): the least-squares fit runs on the device over the whole chunk's primary latents (after the mode split, so every mode combines with it), the
 * residuals page by page with each page's first `order` latents as its state.  Order > 32 or a 64-bit type: PCO_GFX_INVALID_ARGUMENT; order 0, or a fit
 * that yields no config (fewer than order + 1 numbers, a non-finite weight sum, a negative quantization): NoOp delta.  A page shorter than the order
 * (PagingSpec::Exact, tiny pages) is PCO_GFX_INVALID_ARGUMENT, where the reference panics.  Opt-in: without this bit TryConv1 is refused as before. */
#define PCO_GFX_CFG_CONV1 2u
/* Dict mode encode: ModeSpec::TryDict behaves as in the reference (mode/dict.rs:10-66): the dictionary holds the chunk's distinct ordered latents
 * (floats by bit pattern: -0.0, +0.0 and every NaN payload apart), most frequent first, and the primary latent variable is the u32 index into it
 * whatever the number type, delta'd by the delta spec (Auto included: the trials run on the indices as u32).  A chunk whose worst case beats the
 * baseline falls back to the Classic/NoOp chunk, as in the reference.  Ties between equal counts: the reference's order is not defined (HashMap
 * iteration); this library writes ascending ordered latent, one of the orders the reference may write, so the bytes are deterministic.
 * TryDict with TryConv1: PCO_GFX_UNSUPPORTED (the fit would run in the u32 index type).  The ChunkMeta holds the dictionary: pco_gfx_wrapped_chunk_cap
 * counts it.  Opt-in: without this bit TryDict is refused as before (also with PCO_GFX_CFG_CONV1 alone). */
#define PCO_GFX_CFG_DICT 4u
/* Verified encode (section 3b): behind the encode, on the same stream, every chunk (or wrapped piece) whose encode ended OK is decoded by the library's
 * own decode path from the bytes just written into workspace scratch and compared BIT FOR BIT with its source; the result carries
 * PCO_GFX_AUX_VERIFIED, or PCO_GFX_CORRUPTION.  No byte of dst differs from the unflagged call's.  Opt-in: without this bit nothing is launched.
 * PCO_GFX_VERIFY=1 in the environment (read once, when the library is loaded) sets it for every call of the process, like PCO_GFX_STRICT_HISTOGRAM. */
#define PCO_GFX_CFG_VERIFY 8u

/* Detailed status of the last failing call on this thread (errors.rs:8-24). */
enum PcoGfxStatus {
  PCO_GFX_OK = 0,
  PCO_GFX_CORRUPTION = 1,
  PCO_GFX_INSUFFICIENT_DATA = 2,
  PCO_GFX_INVALID_ARGUMENT = 3,
  PCO_GFX_UNSUPPORTED = 4,   /* feature outside the hot-path scope (Dict encode without PCO_GFX_CFG_DICT; Conv1 encode without PCO_GFX_CFG_CONV1; lookback with a delta'd secondary variable in an ASYNCHRONOUS decode call) */
  PCO_GFX_DEVICE_ERROR = 5,  /* no GPU / HIP failure: the product has no CPU fallback */
};
int pco_gfx_last_status(void);
const char* pco_gfx_last_error(void);
/* Number of visible HIP devices (0 => every compute entry point fails with DEVICE_ERROR). */
int pco_gfx_device_count(void);

/* standalone::simple_compress / simple_compress_into with a full ChunkConfig.
 * `uniform_type` != 0 writes the uniform dtype byte (simple_compress_into, simple.rs:27-29);
 * 0 leaves it 0 (simple_compress, simple.rs:65).  HOST buffers.  A chunk holds at most 2^24 numbers: a max_page_n (or an exact
 * size below) that asks for more is PCO_GFX_INVALID_ARGUMENT, and dst is not written. */
enum PcoError pco_gfx_simple_compress_into_ex(const void* nums, size_t n, unsigned char dtype,
                                              const PcoChunkConfigEx* config, int uniform_type,
                                              void* dst, size_t dst_cap, size_t* n_written);
/* The same under PagingSpec::Exact (chunk_config.rs:124,162-180): standalone::simple_compress cuts one chunk per entry of the
 * paging spec (standalone/simple.rs:32-45), so `page_sizes` are the chunk sizes; they must be non-zero and sum to n.
 * dst_cap: header + footer + sum of pco_gfx_guarantee_chunk_size(page_sizes[i]). */
enum PcoError pco_gfx_simple_compress_into_exact(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config,
                                                 int uniform_type, const size_t* page_sizes, size_t n_pages, void* dst,
                                                 size_t dst_cap, size_t* n_written);
size_t pco_gfx_guarantee_file_size(size_t n, unsigned char dtype, uint64_t max_page_n);
/* standalone/guarantee.rs:21-23: bound for one standalone chunk of n numbers */
size_t pco_gfx_guarantee_chunk_size(size_t n, unsigned char dtype);

/* ------------------------------------------------------------------------------------------
 * 3. Batched chunk codec on DEVICE buffers (one chunk per workgroup; what a many-chunk
 *    caller -- pco_cli bench, a columnar file writer -- would call once per row group).
 *
 *    A "standalone chunk" is exactly what standalone::ChunkCompressor::write emits
 *    (standalone/compressor.rs:191-203): dtype byte | 24-bit n-1 | ChunkMeta | one page.
 *    A .pco file is header | chunks... | 0x00 (standalone/simple.rs:62-91); use
 *    pco_gfx_write_standalone_header / _footer to frame device-produced chunks.
 * ---------------------------------------------------------------------------------------- */

typedef struct PcoGfxEncodeTask {
  const void* src;   /* DEVICE pointer to n numbers */
  uint64_t n;        /* 1 ..= 2^24 */
  void* dst;         /* DEVICE pointer, 8-byte aligned, >= pco_gfx_guarantee_chunk_size(n) + 16 bytes */
  uint64_t dst_cap;
  uint32_t dtype;
  uint32_t reserved;
} PcoGfxEncodeTask;

typedef struct PcoGfxDecodeTask {
  const void* src;   /* DEVICE pointer to >= 1 standalone chunks; 16 readable bytes past src_len */
  uint64_t src_len;
  void* dst;         /* DEVICE pointer, aligned to its number type (1, 2, 4 or 8 bytes); a 16-byte aligned dst is faster: only there
                      * do the decoders store a lane's four numbers, or a batch, with one instruction */
  uint64_t dst_cap;  /* elements */
  uint32_t dtype;
  uint32_t flags;    /* PCO_GFX_TASK_HAS_FILE_HEADER: src is a whole .pco file */
} PcoGfxDecodeTask;
#define PCO_GFX_TASK_HAS_FILE_HEADER 1u
/* wrapped surface: src = ChunkMeta followed by one page of exactly dst_cap numbers; bits 8..15 of
 * `flags` carry the wrapped format's major version (wrapped/file_decompressor.rs:44-52) */
#define PCO_GFX_TASK_WRAPPED_PAGE 2u
/* parse + validate a ChunkMeta only; `consumed` = its byte length */
#define PCO_GFX_TASK_META_ONLY 4u
/* decode the FIRST chunk of the stream only (standalone/decompressor.rs:233-301, one DecompressorItem at a time): result.aux bit 0 = another
 * chunk follows, `consumed` = the bytes through this chunk (and the terminator, if it was the last).  A file stores no chunk lengths, so
 * the chunks of one file decode one after the other; this is the step a caller (or pco_standalone_simple_decompress_into) repeats.  On a
 * stream without file header, bits 8..15 of `flags` carry the format's major version when it is not the current one. */
#define PCO_GFX_TASK_ONE_CHUNK 8u

typedef struct PcoGfxTaskResult {
  uint64_t n_out;    /* encode: bytes written; decode: elements written */
  uint64_t consumed; /* decode: bytes consumed from src; a verified encode that failed (section 3b): the index of the first differing number */
  uint32_t status;   /* enum PcoGfxStatus */
  uint32_t aux;      /* encode: bit0 = fell back to the uncompressed-equivalent chunk; bit1 = PCO_GFX_AUX_VERIFIED (section 3b) */
} PcoGfxTaskResult;
/* in PcoGfxTaskResult::aux and PcoGfxPageInfo::aux of an encode: the bytes were decoded again and equal the source bit for bit (section 3b) */
#define PCO_GFX_AUX_VERIFIED 2u

/* `tasks` and `results` are HOST arrays of n_tasks entries (copied by the library; results are
 * filled when the call returns, i.e. the call synchronises `stream`).  If `results` is NULL the
 * call is asynchronous and `d_results` (DEVICE array, may be NULL otherwise) receives the
 * results in stream order.
 * Decode, tANS tables beyond the general kernel's LDS budget (any valid ChunkMeta may carry them: ans_size_log up to 14, up to 2^14 bins):
 * such a chunk decodes in BOTH forms with status OK.  A synchronous call hands the task back internally and runs it once more with global
 * table scratch; an asynchronous call cannot come back, so it takes that scratch up front (832 KB per block of the general kernel, at
 * most 4096 blocks) and decodes the task in its one pass -- never PCO_GFX_UNSUPPORTED, never handed back to the caller. */
enum PcoError pco_gfx_compress_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks,
                                      const PcoChunkConfigEx* config, PcoGfxTaskResult* results,
                                      PcoGfxTaskResult* d_results, void* stream);
enum PcoError pco_gfx_decompress_chunks(size_t n_tasks, const PcoGfxDecodeTask* tasks,
                                        PcoGfxTaskResult* results, PcoGfxTaskResult* d_results,
                                        void* stream);

/* Device-side assembly of the chunk stream standalone::simple_compress writes (standalone/simple.rs:62-91: chunks back to back).
 * `tasks` (HOST array) and `d_results` (DEVICE array) are those of a pco_gfx_compress_chunks call on the same stream (pass a
 * d_results array to that call; it is filled in synchronous calls too).  Chunk i's bytes are copied to
 * d_dst[d_offsets[i] .. d_offsets[i+1]) with d_offsets[0] = dst_offset; d_offsets is a DEVICE array of n_tasks + 1 entries.
 * A chunk whose status in d_results is not PCO_GFX_OK contributes nothing (d_offsets[i] == d_offsets[i + 1]).  The destination is too
 * small when the END offset, dst_offset + the bytes of the chunks, exceeds dst_cap; then nothing is copied and d_offsets[n_tasks]
 * reads ~0 in either form.  If `total` is non-NULL the call synchronises `stream` and stores d_offsets[n_tasks] there: the end of the
 * stream, or ~0 together with PCO_GFX_INVALID_ARGUMENT when the destination is too small (NOT the size that would have been needed).
 * With total == NULL the call is asynchronous and d_offsets[n_tasks] == ~0 is the only sign.  At most 2^31 / ceil(max dst_cap /
 * 64 KiB) chunks per call. */
enum PcoError pco_gfx_compact_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoGfxTaskResult* d_results, void* d_dst,
                                     uint64_t dst_cap, uint64_t dst_offset, uint64_t* d_offsets, uint64_t* total, void* stream);

/* ------------------------------------------------------------------------------------------
 * 3b. VERIFIED encodes: know, before the originals are freed, that what was written reads back to what was put in.
 *
 * PCO_GFX_CFG_VERIFY in PcoChunkConfigEx::flags (or PCO_GFX_VERIFY=1 in the environment) holds for pco_gfx_compress_chunks,
 * pco_gfx_compress_wrapped_chunks[_ex], pco_gfx_simple_compress_into_ex / _exact and pco_standalone_simple_compress_into.  The flag path IS the two
 * entry points below, called behind the encode on its stream; they are also public steps of their own, for chunks encoded earlier or moved since
 * whose numbers are still on the device.
 *   Per task whose encode status is PCO_GFX_OK: the bytes in dst are decoded by the library's own decode path into workspace scratch and the
 *   numbers compared with src as BYTES -- NaN payloads and -0.0 / +0.0 are distinct; never a float ==.
 *     decoded OK, exactly n numbers, no difference   aux |= PCO_GFX_AUX_VERIFIED; everything else is what the unflagged call writes
 *     anything else                                  status = PCO_GFX_CORRUPTION, n_out = 0, aux keeps bit 0 and lacks bit 1, and `consumed` (unused on
 *                                                    encode results otherwise) says why: the decode ended OK -> the index of the first number that
 *                                                    differs, or the decoded count when that is below n and everything before it matched; the decode
 *                                                    did not end OK -> ~0
 *   A task whose encode status is not PCO_GFX_OK keeps its result word for word; its dst is not decoded (the device copy of its decode task is
 *   refused the way a directory task is: section 4e).  So is a task whose encode result names more bytes than dst_cap - 16: it reports
 *   PCO_GFX_CORRUPTION with consumed = ~0, and nothing of it is read.
 *   A wrapped piece (PcoGfxPageInfo has no `consumed`) reports status and aux only; offset, len and n stay.  A ChunkMeta piece is verified iff
 *   all its pages are, and PCO_GFX_CORRUPTION when a page is; a chunk whose ChunkMeta piece is not PCO_GFX_OK keeps every piece as it is.
 *   The bytes of dst are never modified, neither inside nor beyond n_out; src is only read.
 *   The compactors drop a chunk whose status (any piece's, for wrapped chunks) is not PCO_GFX_OK, so encode(verify) -> pco_gfx_compact_chunks /
 *   pco_gfx_compact_wrapped_chunks leaves an unverified chunk out with no further step.
 *   Forms: results / d_results (infos / d_infos) as in the encode entry points.  The asynchronous form makes no host synchronisation of its own
 *   (the source lengths are patched on the device from the encode's results); an Auto spec still synchronises inside the encode (section 3c: resolve once, then encode from specs without one).  A synchronous
 *   flagged call beyond the workspace budget runs in passes as before, each pass verifying its own chunks; the per-chunk figure grows by the
 *   scratch (one slot of numbers per chunk) and the decode's own buffers.
 *   Scratch: n * sizeof(number) per task (rounded up to 256 bytes) plus what pco_gfx_decompress_chunks / _pages takes for the same tasks.
 *   Two limits of a verify, both PCO_GFX_INVALID_ARGUMENT, and checked by a flagged encode BEFORE it launches anything (nothing is written):
 *     chunks (wrapped: pages) per call: at most 2^31 / ceil(the longest one's bytes / 64 KiB) -- the compare kernel's grid, as in pco_gfx_compact_chunks;
 *     a flagged pco_gfx_compress_chunks needs the documented dst_cap >= pco_gfx_guarantee_chunk_size(n) + 16 in every task: the decode behind the
 *     encode may read 16 bytes past a chunk, while the encoders alone fill dst to within 8 bytes of dst_cap.  (The wrapped caps and the host-buffer
 *     entry points always leave them.)  pco_gfx_verify_chunks on its own takes any dst_cap >= 16 and refuses the one task, as said above.
 *
 * pco_gfx_verify_chunks: `tasks` (HOST) are those of the encode call -- src / n / dtype the numbers, dst / dst_cap the chunk; d_encoded (DEVICE,
 * required) is that call's d_results.  results / d_results: synchronous / asynchronous as everywhere; d_results may alias d_encoded.  Output per
 * task is exactly what the flag would have left.
 * pco_gfx_verify_wrapped_chunks: the wrapped counterpart; `config` is read for max_page_n only, as in pco_gfx_compact_wrapped_chunks; d_encoded
 * is the encode's d_infos; d_infos may alias it.
 * Host checks, made before a device is asked for (PCO_GFX_INVALID_ARGUMENT, nothing launched, results untouched): n_tasks != 0 with tasks == NULL;
 * d_encoded == NULL; both result arrays NULL; n outside 1 ..= 2^24; an unknown dtype; a dst_cap below 16; a NULL src or dst; a src that is not
 * aligned to its number type; for wrapped chunks also page_sizes ==
 * NULL with n_pages != 0 (or the reverse), a page of 0 numbers, sizes that do not sum to n.  n_tasks == 0 succeeds without a device.
 * In the synchronous form a task that ends in PCO_GFX_CORRUPTION makes the call return PcoCompressionError with the last error set.
 * ---------------------------------------------------------------------------------------- */
enum PcoError pco_gfx_verify_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoGfxTaskResult* d_encoded, PcoGfxTaskResult* results,
                                    PcoGfxTaskResult* d_results, void* stream);

/* standalone/compressor.rs:85-105 and :157-162 (host-side framing, tiny) */
size_t pco_gfx_write_standalone_header(void* dst, size_t dst_cap, uint64_t n_hint, unsigned char uniform_dtype);
size_t pco_gfx_write_standalone_footer(void* dst, size_t dst_cap);

/* Release this thread's device workspace. */
void pco_gfx_release_workspace(void);
/* Bytes of device memory this thread's workspace holds right now (the library's scratch: it grows to what the largest call so far needed and
 * stays until released).  For capacity planning and for the benchmark's `workspace_bytes_per_input_byte`; the reference has no counterpart
 * (its scratch is the host heap). */
size_t pco_gfx_workspace_bytes(void);
/* How many (chunk, latent variable) histograms of this thread's PCO_GFX_CFG_STRICT_HISTOGRAM calls on the current device replayed the
 * reference's heapsort branch (histograms.rs:248-258) since the workspace was created: 0 on any data that was not ordered against the
 * pivot rule.  Waits for the thread's last call.  (This counter and the two below are 64-bit totals kept on the host: they survive
 * pco_gfx_release_workspace and the library's own re-allocations.) */
unsigned long long pco_gfx_strict_histogram_fallbacks(void);
/* How many chunks of this thread's decode calls on the current device were marked for the expander kernel that runs UNDER the tANS walk
 * (decode_trail.hip) and had to be expanded after it instead, because their expander wave saw no walker beside it for ~55 ms (a device shared with
 * another process' kernels) or left early: such a call is correct but slower.  0 on an idle device.  Waits for the thread's last call. */
unsigned long long pco_gfx_trail_givebacks(void);
/* ... and how many chunks the walker marked for that kernel in the first place (the denominator). */
unsigned long long pco_gfx_trail_marked(void);

/* Per-kernel timing (HIP events on the launch stream): begin() arms it for this thread; end()
 * synchronises and returns the number of kernels launched since begin(), writing their names
 * NUL-separated into `names` and their durations in milliseconds into `ms`. */
void pco_gfx_profile_begin(void);
int pco_gfx_profile_end(char* names, size_t names_cap, float* ms, int cap);

/* ------------------------------------------------------------------------------------------
 * 3c. RESOLVE ONCE, encode from saved per-chunk specs.  Under ModeSpec::Auto / DeltaSpec::Auto (the reference's default ChunkConfig) every encode
 *     call first resolves each chunk's mode and delta: sample gathers, two detection stages with a host step between them, up to four waves of
 *     trial encodes -- and several host synchronisations.  A writer that sends row group after row group of the same columns needs that answer
 *     once.  pco_gfx_resolve_chunk_specs runs the resolution alone and hands the answer out as one PcoGfxChunkSpec per chunk;
 *     pco_gfx_compress_chunks_specs and pco_gfx_compress_wrapped_chunks_specs (declared in section 4c, beside its task type) encode from such an
 *     array -- a DIFFERENT spec per chunk, which one PcoChunkConfigEx cannot say -- through the explicit-spec path: the same kernels in the same
 *     order as an explicit call, nothing resolved, and in the asynchronous form no host synchronisation.
 *
 *     Why a spec and not (mode_kind, mode_f64): Auto's FloatMult configs that were snapped to a round inverse come from
 *     FloatMultConfig::from_inv_base (mode/float_mult.rs:261-275,330-334) and carry an inv_base that need not equal 1 / base, while an explicit
 *     TryFloatMult(base) computes 1 / base (from_base); the encoded bytes depend on inv_base (float_mult.rs:39-44).  A ChunkMeta stores the base
 *     only.  mode_inv carries the inverse, so the specs call writes the Auto call's bytes.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxChunkSpec {   /* 40 bytes */
  uint32_t mode_kind;    /* PCO_MODE_CLASSIC, _TRY_INT_MULT, _TRY_FLOAT_MULT, _TRY_FLOAT_QUANT: never AUTO */
  uint32_t delta_kind;   /* PCO_DELTA_NOOP, _TRY_CONSECUTIVE, _TRY_LOOKBACK: never AUTO */
  uint32_t delta_order;  /* Consecutive: 1..7 (ignored otherwise) */
  uint32_t mode_k;       /* FloatQuant: k */
  uint64_t mode_base;    /* IntMult: the base (its low bits at the number type's width); FloatMult: the BIT PATTERN of the base in the number type */
  uint64_t mode_inv;     /* FloatMult: the bit pattern of inv_base; 0 = "1 / base, as TryFloatMult computes it" (no finite non-zero base of f16,
                            f32 or f64 has a zero inverse) */
  uint64_t reserved;     /* 0 */
} PcoGfxChunkSpec;
/* What an encode of `tasks` under `config` would resolve, and nothing else: the encode's validation, kernels and host decisions up to the point
 * where its plans are complete, then one spec per task into `specs` (HOST array).  tasks[i].src, n and dtype are read; dst and dst_cap are
 * ignored and may be NULL / 0.  Synchronous; writes no device memory of the caller's.  The conversion is lossless: a specs call under the same
 * level writes the bytes the Auto call writes (a Lookback window is a function of n, the unoptimized bin count of level and n).
 * With mode AND delta explicit in `config` no device is needed and nothing is launched: the result is what the explicit call plans --
 * TryConsecutive(0) comes back as NOOP, TryFloatMult with mode_inv = 1 / base in the number type, TryIntMult with the base cut to the type's width.
 * Errors are the encode's ("The chosen mode was invalid for the number type", ...).  PCO_MODE_TRY_DICT and PCO_DELTA_TRY_CONV1 are
 * PCO_GFX_UNSUPPORTED with or without their flag bits: a spec cannot carry a dictionary or a fit. */
enum PcoError pco_gfx_resolve_chunk_specs(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config, PcoGfxChunkSpec* specs,
                                          void* stream);
/* The spec a ChunkMeta's mode and delta encoding describe (host arithmetic over pco_gfx_chunk_meta_info, whose errors it returns): what the
 * reference's users do when they read ChunkMeta.mode / delta_encoding and pass TryFloatMult(base) / TryConsecutive(k) from then on.  mode_inv
 * is 0 -- the metadata does not store the inverse -- so the spec has Try* semantics and reproduces the WRITER's bytes only where the writer's
 * inverse was 1 / base; keep the spec pco_gfx_resolve_chunk_specs gave for the bytes of an Auto call.  Dict, Conv1 and secondary_uses_delta
 * metas: PCO_GFX_UNSUPPORTED. */
enum PcoError pco_gfx_chunk_spec_from_meta(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, PcoGfxChunkSpec* spec);
/* pco_gfx_compress_chunks with chunk i's mode and delta taken from specs[i] (HOST array of n_tasks entries, read before the call returns).
 * `config` (may be NULL) supplies the level, max_page_n, enable_8_bit and the flags; PCO_GFX_CFG_VERIFY and _STRICT_HISTOGRAM hold as in the call
 * it mirrors, and so do results / d_results (NULL results: asynchronous, and then WITHOUT a host synchronisation), the passes of a synchronous
 * call beyond the workspace budget (planned from the specs' shape, remembered apart from an Auto call's footprint), the verify behind the encode.
 * A spec is Try* semantics: a mode or delta that does not pay on the data falls back as the explicit call does (aux bit 0), so a stale spec costs
 * compression, never correctness.  pco_gfx_debug_auto_mode / _delta read all-zero after the call: nothing was resolved.
 * Host refusals, in this order, before a device is asked for (nothing launched, results untouched):
 *   tasks == NULL or specs == NULL with n_tasks != 0                                   PCO_GFX_INVALID_ARGUMENT
 *   (wrapped: infos == NULL and d_infos == NULL comes first)
 *   config->mode_kind or config->delta_kind not AUTO (a spec is never silently overridden)     PCO_GFX_INVALID_ARGUMENT
 *   PCO_GFX_CFG_CONV1 or PCO_GFX_CFG_DICT in config->flags                                  PCO_GFX_INVALID_ARGUMENT
 *   then per task i, first failing task first, the message starting "chunk spec i: " --        all PCO_GFX_INVALID_ARGUMENT
 *     an invalid dtype
 *     a mode_kind that is not one of the four above (AUTO, TRY_DICT, unknown); then likewise the delta_kind
 *     TRY_INT_MULT on a float type ("unable to use int mult mode on floats"); a float mode on an integer type ("unable to use float mode for ints")
 *     an IntMult base that is 0 at the type's width ("The chosen mode was invalid for the number type ...", as the three below)
 *     a FloatMult base that is zero, infinite or NaN, or a base / mode_inv with bits beyond the type's width
 *     a FloatQuant k outside 1..precision (f16 10, f32 23, f64 52)
 *     a Consecutive order outside 1..7
 *     reserved != 0
 *     a non-zero mode_inv on a spec that is not FloatMult
 * What the mirrored entry point refuses after these (level, unknown flag bits, n, alignment, caps) it refuses here as it does there. */
enum PcoError pco_gfx_compress_chunks_specs(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config, const PcoGfxChunkSpec* specs,
                                            PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4. Wrapped surface (wrapped/chunk_compressor.rs:544-705, wrapped/file_decompressor.rs:24-52,
 *    wrapped/chunk_decompressor.rs:74-80, wrapped/page_decompressor.rs:193-246), host buffers.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxChunkCompressor PcoGfxChunkCompressor;
typedef struct PcoGfxChunkDecompressor PcoGfxChunkDecompressor;

size_t pco_wrapped_write_header(void* dst, size_t dst_cap);                    /* file_compressor.rs:54 */
enum PcoError pco_wrapped_read_header(const void* src, size_t len, size_t* consumed,
                                      uint8_t* major, uint8_t* minor);          /* file_decompressor.rs:24 */
enum PcoError pco_chunk_compressor_new(const void* nums, size_t n, unsigned char dtype,
                                       const PcoChunkConfigEx* config,
                                       PcoGfxChunkCompressor** out);            /* chunk_compressor.rs:442 */
/* PagingSpec::Exact (chunk_config.rs:124,162-180): the sizes must be non-zero and sum to n */
enum PcoError pco_chunk_compressor_new_exact(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config,
                                             const size_t* page_sizes, size_t n_pages, PcoGfxChunkCompressor** out);
size_t pco_chunk_compressor_n_pages(const PcoGfxChunkCompressor*);
/* exact byte lengths of what write_meta / write_page will write (the *_size_hint functions mirror the reference's estimates) */
size_t pco_chunk_compressor_meta_size(const PcoGfxChunkCompressor*);
size_t pco_chunk_compressor_page_size(const PcoGfxChunkCompressor*, size_t page_idx);
size_t pco_chunk_compressor_page_n(const PcoGfxChunkCompressor*, size_t page_idx); /* n_per_page :544 */
size_t pco_chunk_compressor_meta_size_hint(const PcoGfxChunkCompressor*);       /* :556 */
size_t pco_chunk_compressor_page_size_hint(const PcoGfxChunkCompressor*, size_t page_idx); /* :599 */
enum PcoError pco_chunk_compressor_write_meta(const PcoGfxChunkCompressor*, void* dst, size_t dst_cap, size_t* n_written);          /* :564 */
enum PcoError pco_chunk_compressor_write_page(const PcoGfxChunkCompressor*, size_t page_idx, void* dst, size_t dst_cap, size_t* n_written); /* :659 */
void pco_chunk_compressor_free(PcoGfxChunkCompressor*);

enum PcoError pco_chunk_decompressor_new(const void* src, size_t len, unsigned char dtype,
                                         uint8_t format_major, PcoGfxChunkDecompressor** out,
                                         size_t* consumed);                     /* file_decompressor.rs:44 */
/* PageDecompressor::read of one whole page of `page_n` numbers (page_decompressor.rs:242) */
enum PcoError pco_chunk_decompressor_read_page(PcoGfxChunkDecompressor*, const void* src, size_t len,
                                               size_t page_n, void* dst, size_t dst_cap,
                                               size_t* n_processed, size_t* consumed);
void pco_chunk_decompressor_free(PcoGfxChunkDecompressor*);

/* ChunkDecompressor::page_decompressor + PageDecompressor::read / into_src (wrapped/chunk_decompressor.rs:74-80,
 * page_decompressor.rs:193-246): `read` fills up to dst_len numbers; dst_len must be a multiple of 256 or at least the count of
 * numbers remaining in the page (InvalidArgument otherwise); *n_processed / *finished are the reference's Progress. */
typedef struct PcoGfxPageDecompressor PcoGfxPageDecompressor;
enum PcoError pco_page_decompressor_new(PcoGfxChunkDecompressor*, const void* src, size_t len, size_t page_n, PcoGfxPageDecompressor** out);
enum PcoError pco_page_decompressor_read(PcoGfxPageDecompressor*, void* dst, size_t dst_len, size_t* n_processed, int* finished);
size_t pco_page_decompressor_consumed(const PcoGfxPageDecompressor*);
void pco_page_decompressor_free(PcoGfxPageDecompressor*);

/* ------------------------------------------------------------------------------------------
 * 4b. The wrapped surface, BATCHED, on DEVICE buffers: what an embedding format (the reference's `pcopage` bench codec,
 *     pco_cli/src/bench/codecs/pcopage.rs:33-113; a Parquet- or Zarr-style container) calls once per row group.  A chunk is cut into
 *     pages by PagingSpec::EqualPagesUpTo(config->max_page_n) (chunk_config.rs:145-161); every page is an independent tANS stream
 *     with its own delta state (wrapped/chunk_compressor.rs:164-213,659-705), so the pages of one chunk encode and decode side by side.
 *     The bytes are exactly ChunkCompressor::write_meta's and write_page's.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxPageInfo {
  uint64_t offset;   /* where the piece starts, in bytes from the chunk's dst */
  uint64_t len;      /* bytes written */
  uint64_t n;        /* numbers in the page (0 for the ChunkMeta entry) */
  uint32_t status;   /* enum PcoGfxStatus */
  uint32_t aux;      /* bit0 = the chunk fell back to the uncompressed-equivalent encoding; bit1 = PCO_GFX_AUX_VERIFIED (section 3b) */
} PcoGfxPageInfo;
/* number of pages EqualPagesUpTo(max_page_n) cuts n numbers into (0 => 2^18 per page), and the dst_cap a chunk of n numbers needs */
size_t pco_gfx_wrapped_n_pages(size_t n, uint64_t max_page_n);
size_t pco_gfx_wrapped_chunk_cap(size_t n, unsigned char dtype, const PcoChunkConfigEx* config);
/* wrapped::FileCompressor::chunk_compressor + write_meta + write_page for every page, n_tasks chunks in one pass.  tasks[i].dst (DEVICE,
 * 16-byte aligned, dst_cap >= pco_gfx_wrapped_chunk_cap) receives the ChunkMeta at offset 0 and the pages at the offsets reported.
 * `infos` (HOST) gets 1 + pco_gfx_wrapped_n_pages(tasks[i].n, max_page_n) entries per chunk, chunk after chunk: the ChunkMeta's, then one
 * per page.  Synchronous (the call returns when the bytes are there). */
enum PcoError pco_gfx_compress_wrapped_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config,
                                              PcoGfxPageInfo* infos, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4c. The batched wrapped WRITER: caller-chosen page sizes (PagingSpec::Exact, chunk_config.rs:124,162-180), an asynchronous form with the piece
 *     directory on the device, and the assembly of the pieces into one contiguous stream -- encode, compact, then hand the stream to a file
 *     writer or to pco_gfx_gather_chunks, all on the caller's stream.  pco_gfx_compress_wrapped_chunks above is unchanged (it is this entry
 *     point with n_pages == 0 everywhere and host infos only).
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxWrappedTask {   /* 48 bytes */
  const void* src;              /* DEVICE pointer to n numbers */
  uint64_t n;                   /* 1 ..= 2^24 */
  void* dst;                    /* DEVICE pointer, 16-byte aligned */
  uint64_t dst_cap;             /* >= pco_gfx_wrapped_chunk_cap (n_pages == 0) / pco_gfx_wrapped_chunk_cap_exact (n_pages != 0) */
  uint32_t dtype;
  uint32_t n_pages;             /* 0: PagingSpec::EqualPagesUpTo(config->max_page_n); else PagingSpec::Exact with the sizes below */
  const uint64_t* page_sizes;   /* HOST array of n_pages entries, non-zero, summing to n; NULL iff n_pages == 0.  Read before the call returns */
} PcoGfxWrappedTask;
/* the dst_cap of a chunk cut into exactly these pages: equal to pco_gfx_wrapped_chunk_cap(n, ...) when the sizes are those EqualPagesUpTo cuts.
 * 0 for an invalid dtype, an empty or NULL list, or a page of 0 numbers. */
size_t pco_gfx_wrapped_chunk_cap_exact(const uint64_t* page_sizes, size_t n_pages, unsigned char dtype, const PcoChunkConfigEx* config);
/* pco_gfx_compress_wrapped_chunks with a page list per chunk (a call may mix Exact and EqualPagesUpTo chunks) and the piece directory on the
 * device.  Pieces are ordered as there: per chunk the ChunkMeta's entry, then one per page, chunk after chunk; their count is the sum of
 * 1 + (n_pages ? n_pages : pco_gfx_wrapped_n_pages(n, max_page_n)).  `infos` (HOST) / `d_infos` (DEVICE) follow pco_gfx_compress_chunks'
 * results / d_results: with infos != NULL the call synchronises `stream` and fills infos (and d_infos, if given); with infos == NULL the call is
 * asynchronous, d_infos is required and is filled in stream order (both NULL: PCO_GFX_INVALID_ARGUMENT).  Asynchronous calls: explicit specs do
 * not synchronise; an Auto mode or delta spec synchronises inside the call (the decision is the host's; section 3c's specs call carries a decision made earlier and does not); a full-width latent slot and, in Dict
 * mode, an HBM table are taken for every chunk up front.  Synchronous calls whose scratch would exceed the workspace budget
 * (PCO_GFX_WORKSPACE_GB, default 80 % of free device memory) run as consecutive passes of whole chunks, at least 64 per pass, like
 * pco_gfx_compress_chunks; a device allocation that fails anyway halves the pass.
 * Every argument is checked before anything is launched: a page of 0 numbers, sizes that do not sum to n, page_sizes == NULL with n_pages != 0
 * (or the reverse), a dst that is not 16-byte aligned, a dst_cap below the cap are PCO_GFX_INVALID_ARGUMENT and nothing is written.  A Conv1
 * page shorter than the order is found on the device: its chunk's pieces carry PCO_GFX_INVALID_ARGUMENT. */
enum PcoError pco_gfx_compress_wrapped_chunks_ex(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config,
                                                 PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos, void* stream);
/* Worst-case bytes of workspace one pass over all of `tasks` is planned with under `config` (what the pass-cutting above divides the budget
 * by; host arithmetic only).  For capacity planning: a budget below it makes a synchronous call of more than 64 chunks run in passes. */
size_t pco_gfx_wrapped_scratch_estimate(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config);
/* Device-side assembly of the pieces, the wrapped counterpart of pco_gfx_compact_chunks.  `tasks` (HOST) and `d_infos` (DEVICE) are those of a
 * pco_gfx_compress_wrapped_chunks_ex call on the same stream; `config` is read for max_page_n only (the piece count of the chunks with
 * n_pages == 0: the directory lives on the device, and the host must know its length to size the work).  d_offsets is a DEVICE array of
 * n_pieces + 1 entries, d_offsets[0] = dst_offset; piece k is copied to d_dst[d_offsets[k] + gap .. d_offsets[k + 1]).  The `gap` bytes in
 * front of each piece are for the caller's own framing (gap = 4: pcopage's n_pages / page_n words): they are never read or written.  A chunk
 * with ANY piece whose status is not PCO_GFX_OK contributes nothing: all its d_offsets entries are equal, neither gaps nor bytes are written.
 * The destination is too small when the END offset exceeds dst_cap; then nothing is copied and d_offsets[n_pieces] reads ~0 in either form.
 * If `total` is non-NULL the call synchronises `stream` and stores d_offsets[n_pieces] there: the end of the stream, or ~0 together with
 * PCO_GFX_INVALID_ARGUMENT when the destination is too small (NOT the size that would have been needed).  With total == NULL the call is
 * asynchronous and d_offsets[n_pieces] == ~0 is the only sign.  Fewer than 2^31 pieces per call. */
enum PcoError pco_gfx_compact_wrapped_chunks(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config,
                                             const PcoGfxPageInfo* d_infos, uint32_t gap, void* d_dst, uint64_t dst_cap, uint64_t dst_offset,
                                             uint64_t* d_offsets, uint64_t* total, void* stream);

/* section 3c's encode from per-chunk specs over wrapped chunks (declared here: it takes the writer's task type): pco_gfx_compress_wrapped_chunks_ex
 * with chunk i's mode and delta from specs[i].  Config, refusals and forms as pco_gfx_compress_chunks_specs says; infos / d_infos, paging and caps
 * as above. */
enum PcoError pco_gfx_compress_wrapped_chunks_specs(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config,
                                                    const PcoGfxChunkSpec* specs, PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos, void* stream);

/* section 3b's check as a step of its own over wrapped chunks (declared here: it takes the writer's task type) */
enum PcoError pco_gfx_verify_wrapped_chunks(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config, const PcoGfxPageInfo* d_encoded,
                                            PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos, void* stream);

typedef struct PcoGfxPageTask {
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes (shared by the chunk's pages) */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one page; 16 readable bytes past page_len */
  uint64_t page_len;
  void* dst;             /* DEVICE: room for page_n numbers */
  uint64_t page_n;       /* the page's count of numbers: the wrapping format stores it (wrapped/chunk_decompressor.rs:74-80) */
  uint32_t dtype;
  uint32_t format_major; /* of the wrapped header (pco_wrapped_read_header); the current one is 4 */
} PcoGfxPageTask;
/* ChunkDecompressor::page_decompressor + PageDecompressor::read of the whole page, n_tasks pages in one pass (pages of one chunk or of
 * many; each names its chunk's ChunkMeta).  results[i].n_out = page_n, .consumed = the page's bytes.  results / d_results as in
 * pco_gfx_decompress_chunks. */
enum PcoError pco_gfx_decompress_pages(size_t n_tasks, const PcoGfxPageTask* tasks, PcoGfxTaskResult* results,
                                       PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4d. A ROW RANGE of a wrapped page, without decoding the rest: PageDecompressor::read stops when its caller stops asking
 *     (wrapped/page_decompressor.rs:193-246), and a page decodes strictly forwards, so rows [first, first + count) need the tANS walk up
 *     to batch ceil((first + count) / 256) and nothing behind it.  What a LIMIT query, a row-group index or a sampling reader calls.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxPageRangeTask {   /* 72 bytes */
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes, as in PcoGfxPageTask */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one page; 16 readable bytes past page_len */
  uint64_t page_len;
  void* dst;             /* DEVICE: room for `count` numbers, nothing more */
  uint64_t page_n;       /* numbers in the WHOLE page */
  uint64_t first, count; /* the rows wanted: first + count <= page_n */
  uint32_t dtype;
  uint32_t format_major;
} PcoGfxPageRangeTask;
/* Output: dst[0 .. count) receives rows first .. first + count of the page, bit-identical to what pco_gfx_decompress_pages writes there; no
 *   byte outside dst[0 .. count * width) is written.
 * Forms: results / d_results select the synchronous and the asynchronous form exactly as in pco_gfx_decompress_pages; caller streams, and two
 *   streams on one workspace, work as they do there.
 * Results: n_out = count, aux = 0.  consumed = the page's byte length when the range reaches the page's last batch (the end-of-page padding
 *   check then applies as in a whole decode), else 0.
 * Work is bounded by the prefix: the tANS walk ends with batch ceil((first + count) / 256), and nothing of the page behind that batch is read
 *   or validated.  A page truncated or damaged BEHIND the last batch a range touches decodes with PCO_GFX_OK (the reference's incremental
 *   behaviour, wrapped/page_decompressor.rs:115-221); a range that touches the first batch that cannot be finished gives
 *   PCO_GFX_INSUFFICIENT_DATA with n_out = 0 -- dst[0 .. count) is then unspecified, nothing else is written.
 * Tasks are independent: several ranges of one page in one call are several tasks, each walking its own prefix.
 * count == 0 is legal: status OK, n_out 0, nothing of the task is read; dst may then be NULL.
 * Every argument is checked before anything is launched, and the call then writes nothing: first + count > page_n, page_n == 0 or > 2^24, an
 *   invalid dtype, a NULL meta / page, a NULL dst with count > 0 are PCO_GFX_INVALID_ARGUMENT; format_major > 4 is PCO_GFX_CORRUPTION as in
 *   pco_gfx_decompress_pages.
 * Reach: every stream pco_gfx_decompress_pages decodes -- all number types and modes, no delta, Consecutive, Lookback and Conv1, tables
 *   beyond the walkers' LDS.  Pages without a delta start at batch first / 256; a consecutive delta sums the batches in front for its
 *   moments without joining or storing them.  Lookback, Conv1, Dict and tables beyond the walkers' LDS keep their history in the output, so
 *   their prefix [0, ceil((first + count) / 256) * 256) is decoded into workspace scratch -- that many numbers plus one batch (at most
 *   page_n) -- and the range copied out.  A synchronous call takes that scratch for the tasks that need it, in passes under
 *   PCO_GFX_WORKSPACE_GB; an asynchronous call takes it for every task up front, like the table scratch of pco_gfx_decompress_chunks, and
 *   answers lookback with a delta'd secondary variable with PCO_GFX_UNSUPPORTED as pco_gfx_decompress_pages does.  Two limits of this entry
 *   point alone: a lookback state of more than 256 numbers (no encoder writes more than 2) is PCO_GFX_UNSUPPORTED unless the range reaches
 *   the page's last batch, and the prefixes of one call may take 48 GiB of symbol scratch (3 bytes per number walked) at most. */
enum PcoError pco_gfx_decompress_page_ranges(size_t n_tasks, const PcoGfxPageRangeTask* tasks, PcoGfxTaskResult* results,
                                             PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4e. Pages and row ranges from a page directory in DEVICE memory: the read side of the asynchronous writer.  pco_gfx_compress_wrapped_chunks_ex
 *     (infos == NULL) + pco_gfx_compact_wrapped_chunks (total == NULL) leave a blob and d_offsets on the device without a host synchronisation;
 *     these two entry points decode behind them without one either: a task names its ChunkMeta and its page by PIECE INDEX, and the device
 *     looks the bytes up.  Encode -> compact -> decode is one stream-ordered pipeline.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxDirectory {   /* 40 bytes */
  const void* d_blob;          /* DEVICE: the compacted stream; 16 readable bytes past blob_len */
  uint64_t blob_len;
  const uint64_t* d_offsets;   /* DEVICE: n_pieces + 1 entries, as pco_gfx_compact_wrapped_chunks writes them */
  uint64_t n_pieces;           /* < 2^31 */
  uint32_t gap, reserved;      /* piece k's bytes are d_blob[d_offsets[k] + gap .. d_offsets[k + 1]) */
} PcoGfxDirectory;
typedef struct PcoGfxDirPageTask {   /* 32 bytes */
  void* dst;             /* DEVICE: room for page_n numbers */
  uint64_t page_n;       /* the page's count of numbers: the wrapping format's reader knows it */
  uint32_t meta_piece, page_piece;   /* indices into d_offsets: the chunk's ChunkMeta piece and the page's piece (different, < n_pieces) */
  uint32_t dtype, format_major;
} PcoGfxDirPageTask;
typedef struct PcoGfxDirPageRangeTask {   /* 48 bytes */
  void* dst;             /* DEVICE: room for `count` numbers, nothing more */
  uint64_t page_n, first, count;   /* numbers in the WHOLE page; the rows wanted: first + count <= page_n */
  uint32_t meta_piece, page_piece, dtype, format_major;
} PcoGfxDirPageRangeTask;
/* pco_gfx_decompress_pages / pco_gfx_decompress_page_ranges with each task's meta, meta_len, page and page_len taken from the directory ON THE
 *   DEVICE.  `tasks` and `*dir` are HOST memory; the library copies them, and they may be overwritten as soon as the call returns.
 * Forms: results / d_results select the synchronous and the asynchronous form exactly as in the pointer-taking entry points.  The asynchronous
 *   form (results == NULL) makes no host synchronisation and reads nothing of the directory on the host; caller streams, and two streams on one
 *   workspace, behave as there.  Scratch as there: table and prefix scratch up front in asynchronous calls; a delta'd secondary variable under
 *   lookback stays PCO_GFX_UNSUPPORTED in them.
 * Results of a well-described task: dst and the task's result (n_out, consumed, aux; the prefix-bounded work of a range, count == 0, a page
 *   damaged behind the range) are bit-identical to those of the pointer form given the pointers and lengths the directory describes.
 * Directory verdicts are made on the device, in this order.  A task that fails one has the result {status, n_out 0, consumed 0, aux 0}; nothing of
 *   the blob is read for it and no byte of dst is written:
 *     d_offsets[n_pieces] == ~0 (the compactor's "destination too small": nothing was copied)      every task PCO_GFX_INVALID_ARGUMENT
 *     for either piece k of the task: d_offsets[k] > d_offsets[k + 1] or d_offsets[k + 1] > blob_len    PCO_GFX_INVALID_ARGUMENT
 *     d_offsets[meta_piece + 1] == d_offsets[meta_piece]: the chunk was dropped                          PCO_GFX_INSUFFICIENT_DATA
 *     the ChunkMeta is kept, but either piece's extent is smaller than gap                               PCO_GFX_INVALID_ARGUMENT
 *   (The compactor drops a chunk with any failed piece as a whole, and a kept ChunkMeta is at least one byte.  A kept PAGE may be 0 bytes long
 *   -- a constant chunk under Classic without delta -- and decodes with PCO_GFX_OK, for gap == 0 too.)  A range task with count == 0 is
 *   PCO_GFX_OK and reads nothing, neither the directory's entries nor the blob, whatever its pieces look like.
 * Host checks, made before anything is launched and before a device is asked for; nothing is written and `results` stays untouched:
 *   PCO_GFX_INVALID_ARGUMENT for NULL tasks with n_tasks > 0, a NULL dir, d_blob or d_offsets, results and d_results both NULL, n_pieces >= 2^31,
 *   a piece index >= n_pieces, meta_piece == page_piece, an invalid dtype, page_n == 0 or > 2^24, a NULL dst (with count > 0 for ranges),
 *   first + count > page_n (a sum that wraps included); PCO_GFX_CORRUPTION for format_major > 4.  In the synchronous form a failing task sets the
 *   last error as in pco_gfx_decompress_pages.
 * Not covered: a page_n that lives on the device.  (Standalone chunks behind pco_gfx_compact_chunks' offsets: 4l.) */
enum PcoError pco_gfx_decompress_pages_dir(size_t n_tasks, const PcoGfxDirPageTask* tasks, const PcoGfxDirectory* dir,
                                           PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);
enum PcoError pco_gfx_decompress_page_ranges_dir(size_t n_tasks, const PcoGfxDirPageRangeTask* tasks, const PcoGfxDirectory* dir,
                                                 PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4f. Reading a page in SLICES, and from a restart point: the other half of PageDecompressor::read (wrapped/page_decompressor.rs:193-246),
 *     whose tANS states, bit position and delta state live on between two reads.  A range task (4d) walks its page from batch 0 every time; a
 *     read task starts from a CURSOR an earlier read left and leaves one for the next.  A cursor holds no pointers, so it is also a restart
 *     point: walk a page once, keep the cursors, and decode its segments side by side in one call later.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxPageCursor { uint64_t w[32]; } PcoGfxPageCursor;   /* 256 bytes, DEVICE memory, 8-byte aligned, no pointers inside */
typedef struct PcoGfxPageReadTask {   /* 88 bytes: PcoGfxPageRangeTask's fields in its order, then the two cursors */
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes, as in PcoGfxPageTask */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one page; 16 readable bytes past page_len */
  uint64_t page_len;
  void* dst;             /* DEVICE: room for `count` numbers, nothing more */
  uint64_t page_n;       /* numbers in the WHOLE page */
  uint64_t first, count; /* the rows wanted: first + count <= page_n */
  uint32_t dtype;
  uint32_t format_major;
  const PcoGfxPageCursor* from;   /* DEVICE, or NULL: the page's start */
  PcoGfxPageCursor* to;           /* DEVICE, or NULL: not wanted.  May equal `from` */
} PcoGfxPageReadTask;
/* Results: dst[0 .. count), n_out, consumed, aux and the status are bit-identical to pco_gfx_decompress_page_ranges on the same page, first and
 *   count, whatever `from` is: a page damaged behind the read decodes with PCO_GFX_OK, one damaged inside it gives PCO_GFX_INSUFFICIENT_DATA
 *   with n_out = 0; count == 0 is PCO_GFX_OK, nothing is read -- `from` included -- and `to` is not written.
 * The cursor: `from` describes a row `at` of the page, with at % 256 == 0 or at == page_n, and at <= first; the walk starts at batch at / 256,
 *   not at 0.  On PCO_GFX_OK `to` describes row min(ceil((first + count) / 256) * 256, page_n); on any other status it is left as it was.  The
 *   content of `to` is a function of the page and that row only: byte-identical whether the row was reached in one read or in many, and with
 *   from == NULL or not.  A cursor may be copied and reused any number of times; one written by a task must not be read by another task of the
 *   same call.
 * Layout (version 1), in 64-bit words:
 *     w[0]        version (bits 0..31) = 1 | kind (bits 32..63): 1 = full state, 2 = position only
 *     w[1]        row
 *     w[2]        bit position in the page (0 in a position-only cursor)
 *     w[3]        page_n (bits 0..31) | dtype (bits 32..63)
 *     w[4..9]     states[3][4] as tANS state INDICES (not table addresses): chain j of latent variable v (0 delta, 1 primary, 2 secondary) in bits
 *                 32 (j % 2) .. of w[4 + 2 v + j / 2]; 0 for a variable the page does not have
 *     w[10..25]   moments[2][8]: the consecutive-delta moments of the primary and of the secondary variable, 0 beyond the delta's order
 *     w[26..31]   0
 *   A position-only cursor holds w[0], w[1] and w[3]; every other word is 0.
 * Reach: pages on pco_gfx_decompress_page_ranges' two-kernel route -- no delta or Consecutive orders 1-7 on either variable, tables inside the
 *   walkers' LDS slices -- get full-state cursors, and a read's work is proportional to the batches between `at` and its end.  The others
 *   (Lookback, Conv1, Dict, tables beyond the walkers' LDS) keep their history in the output, and that does not fit 256 bytes: they get
 *   POSITION-ONLY cursors, and a read from one decodes the prefix from row 0 into workspace scratch as a range task does.  The numbers are the
 *   same; only the cost differs.  Of these only Lookback needs it: 4h's flag gives the others full-state cursors of a kind of their own (3).
 * The verdict on `from` is made on the device (the cursor lives there), once the ChunkMeta and the page header are parsed and before anything
 *   of the cursor is used.  Any of these is PCO_GFX_INVALID_ARGUMENT, with nothing of dst or `to` written: a wrong version, or a kind other
 *   than the page's route writes; a page_n or dtype other than the task's; at > first; at neither a multiple of 256 nor page_n; a bit
 *   position before the page body's first bit or beyond page_len * 8; a state index >= 2^ans_size_log of its variable (>= 1 for a variable
 *   the page does not have).  A cursor that passes may still belong to ANOTHER page: the result is then wrong numbers or
 *   PCO_GFX_INSUFFICIENT_DATA, never an access outside the page, the tables or dst -- the checks above bound every address the walker forms
 *   (its start batch, its window position, its table entries), and the cursor is read once: what is judged is what is used.
 * Host checks, forms, streams: as pco_gfx_decompress_page_ranges -- every argument of the task's first ten fields is checked before anything is
 *   launched, and `results` stays untouched on refusal.
 * Scratch: a synchronous call gives prefix scratch to the tasks of the second kind only; an asynchronous call takes it for every task up front.
 *   Symbol scratch (3 bytes per number) is sized by the batches the call's tasks WALK, ceil((first + count) / 256) - at / 256, not by their end
 *   batch: a synchronous call reads the rows of its `from` cursors back to know them.  An asynchronous call cannot know `at` on the host and
 *   sizes by the end batch, as a range call does.
 * Not covered: the host-buffer pco_page_decompressor_* handle, cursors written by the encoder.  Conv1, Dict and wide tables resume under 4h's
 *   flag, Lookback beside a history buffer through 4i's entry point; the directory form is 4k. */
enum PcoError pco_gfx_decompress_page_reads(size_t n_tasks, const PcoGfxPageReadTask* tasks, PcoGfxTaskResult* results,
                                            PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4g. Indexing a page in ONE walk: the cursors 4f's side-by-side decode starts from.  A read task writes one `to` cursor, and a cursor written
 *     by a task may not be read in the same call, so k cursors through 4f cost k chained calls -- each parsing the ChunkMeta again and decoding
 *     rows nobody wants, and on Lookback, Conv1 and Dict pages each decoding its prefix from row 0.  An index task makes the decoder's own walk
 *     once, stores no rows and has no dst: encode -> compact -> index is one stream-ordered pipeline, as encode -> compact -> decode is.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxPageIndexTask {   /* 64 bytes */
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes, as in PcoGfxPageTask */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one page; 16 readable bytes past page_len */
  uint64_t page_len;
  PcoGfxPageCursor* cursors;   /* DEVICE, 8-byte aligned: room for pco_gfx_page_index_len(page_n, every_rows) cursors; may be NULL when that is 0 */
  uint64_t page_n;       /* numbers in the WHOLE page */
  uint64_t every_rows;   /* a positive multiple of 256 */
  uint32_t dtype;
  uint32_t format_major;
} PcoGfxPageIndexTask;
/* k = (page_n - 1) / every_rows: the cursors of an index, every one with rows behind it (k * every_rows < page_n).  0 for what the entry point
 *   refuses: page_n == 0 or > 2^24, every_rows == 0 or not a multiple of 256. */
size_t pco_gfx_page_index_len(uint64_t page_n, uint64_t every_rows);
/* Output: on PCO_GFX_OK cursors[i], i = 0 .. k - 1, is the cursor in front of row (i + 1) * every_rows, byte-identical to the `to` cursor a
 *   pco_gfx_decompress_page_reads task ending at that row writes (4f: a function of the page and the row only).  No byte outside cursors[0 .. k) is
 *   written.  The caller keeps the cursor arrays of two tasks apart.
 * Work: one walk per page, over batches [0, k * every_rows / 256), and it ends there: nothing of the page behind that batch is read or
 *   validated.  No rows are stored.
 * Results: n_out = k on PCO_GFX_OK and 0 otherwise; consumed = 0 (the walk never reaches the page's last batch); aux bit 0 = 1 when the index is
 *   position-only.  k == 0: PCO_GFX_OK with n_out 0, nothing of the task is read, and `cursors` may be NULL.
 * Kinds: a page gets the kind of cursor that reads of that page write and accept.  Pages on the two-kernel route (no delta or Consecutive orders
 *   1-7 on either variable, tables inside the walkers' LDS slices) get full-state cursors.  The others (Lookback, Conv1, Dict, tables beyond the
 *   walkers' LDS) get position-only cursors and are not walked at all: the task's status is the one the pco_gfx_decompress_page_ranges task
 *   {first 0, count 1} on the same bytes reports in the same form -- the verdict on the ChunkMeta and the page header, the first batch, and
 *   PCO_GFX_UNSUPPORTED for a delta'd secondary variable under lookback in the asynchronous form.
 *   Under 4h's flag only the Lookback pages stay of this kind; the others are walked once and get kind-3 cursors.
 * Failure: a page whose bytes end inside the walked prefix is PCO_GFX_INSUFFICIENT_DATA, as the range task {first 0, count k * every_rows} is;
 *   one damaged behind its last cursor is PCO_GFX_OK.  On any status but PCO_GFX_OK the task's cursor slots hold unspecified bytes, to be
 *   discarded; bytes outside them stay untouched, and neighbouring tasks are unaffected.
 * Forms, streams: results / d_results select the synchronous and the asynchronous form as in every entry point of this section; the
 *   asynchronous form makes no host synchronisation.  In the synchronous form a failing task sets the last error as in pco_gfx_decompress_pages.
 * Scratch: symbol scratch is 3 bytes per number WALKED, sized by the call's largest k * every_rows, under the 48 GiB limit of a range call;
 *   for the pages of the second kind every task takes two batches of prefix scratch up front, in both forms: there are no passes.
 * Host checks, made before anything is launched and before a device is asked for; `results` stays untouched: PCO_GFX_INVALID_ARGUMENT for NULL
 *   tasks with n_tasks > 0, results and d_results both NULL, a NULL meta or page, an invalid dtype, page_n == 0 or > 2^24, every_rows == 0 or
 *   not a multiple of 256, k > 0 with NULL or misaligned `cursors`; PCO_GFX_CORRUPTION for format_major > 4.  n_tasks == 0 succeeds without a
 *   device.
 * Not covered: extending an existing index from its last cursor.  (An index of a Lookback page -- its reads resume from a cursor AND a history
 *   buffer, 4i -- is pco_gfx_index_pages_hist, 4j; Conv1, Dict and wide tables get full-state cursors under 4h's flag; the directory form is 4k.) */
enum PcoError pco_gfx_index_pages(size_t n_tasks, const PcoGfxPageIndexTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results,
                                  void* stream);

/* ------------------------------------------------------------------------------------------
 * 4h. FULL-STATE cursors for the pages the general kernel decodes (opt-in): pco_gfx_decompress_page_reads_ex and pco_gfx_index_pages_ex are 4f's
 *     and 4g's entry points with a `flags` argument.  flags == 0 IS the entry point without it, byte for byte: results, dst, cursors.  Any bit
 *     other than PCO_GFX_CURSOR_GENERAL is PCO_GFX_INVALID_ARGUMENT before anything is launched, `results` untouched.  The task structs are
 *     4f's and 4g's.  With PCO_GFX_CURSOR_GENERAL:
 * Pages on the two-kernel route: as without the flag -- kind 1, the same bytes.
 * GENERAL pages -- every other page without Lookback on either variable: Conv1, Dict under None / Consecutive / Conv1, and tANS / bin tables beyond
 *   the walkers' LDS slices under None / Consecutive, with one, two or three variables -- write and accept KIND 3.  What the general kernel
 *   carries between two batches of such a page is the bit position, the states, the count left and either the consecutive moments or Conv1's
 *   `order` <= 32 residuals (Conv1 never has a delta'd secondary): it fits the cursor.  Layout (version 1), in 64-bit words:
 *     w[0..3]     as kind 1: version | kind = 3, row, bit position, page_n | dtype
 *     w[4..9]     states[3][4] as state indices below 2^ans_size_log, 0 for a variable the page does not have
 *     w[10..25]   under no delta or Consecutive: moments[2][8] exactly as kind 1, 0 beyond each order.  Under Conv1: the `order` residuals the
 *                 decoder carries in front of the row's batch (delta/conv1.rs: the latents of rows [row, row + order), in Dict mode the
 *                 dictionary indices -- the output lags the deltas by `order`) as u32, residual i in bits 32 (i % 2) .. of w[10 + i / 2],
 *                 0 beyond the order
 *     w[26..31]   0
 *   A read of such a page walks batches [at / 256, ceil((first + count) / 256)) and nothing in front of them; an index task walks batches
 *   [0, k * every_rows / 256) once -- tANS walk, offset unpack, delta decode; no mode join, no dictionary lookup, no store (an index beyond
 *   the dictionary is still PCO_GFX_CORRUPTION) -- and its result is {n_out k, consumed 0, aux bit 0 = 0}.  A page that ends inside the walked
 *   prefix is PCO_GFX_INSUFFICIENT_DATA; one damaged behind the last cursor is PCO_GFX_OK.
 * LOOKBACK pages (any mode) keep kind 2, the prefix decode from row 0 and aux bit 0 = 1: their history is the output itself -- a data
 *   dependency on every row in front, not a matter of layout.  No other page's carried state was found not to fit.
 * A cursor's bytes stay a function of the page and the row only: identical whether the row was reached by one read, by many, with from == NULL
 *   or by the index.
 * A page accepts exactly the kind its route writes under the call's flags.  PCO_GFX_INVALID_ARGUMENT, with nothing of dst or `to` written: a
 *   kind-3 cursor in a call with flags == 0; a kind-2 cursor on a general page under the flag; any cursor of another kind than 2 on a Lookback
 *   page; and, for kind 3, 4f's list -- version, page_n, dtype, at > first, at neither a multiple of 256 nor page_n, a bit position before the
 *   page body's first bit or beyond page_len * 8, a state index >= 2^ans_size_log of its variable (>= 1 for a variable the page does not
 *   have) -- and a walk of more batches than the host gave scratch for (a cursor that changed after a synchronous call sized by it).  The
 *   verdict is made on ONE copy of the cursor, after the ChunkMeta and the page header are parsed and the tables built.  w[10..25] are not
 *   judged: moments and Conv1 residuals are summands of the numbers -- and, in Dict mode, of an index that is compared with the dictionary's
 *   length before it is used -- and no address is formed from them.  A cursor that passes may belong to ANOTHER page: wrong numbers,
 *   PCO_GFX_INSUFFICIENT_DATA or PCO_GFX_CORRUPTION, never an access outside the page, the tables or the scratch.
 * Scratch: a general page's read takes prefix scratch for the batches it walks and one more in a synchronous call (which reads the rows of the
 *   kind-3 `from` cursors back), for its end batch in an asynchronous one; passes under PCO_GFX_WORKSPACE_GB as in 4f.  An index task takes
 *   two batches, which only a Lookback page uses.
 * Host checks, forms, streams, two streams on one workspace: as 4f and 4g.
 * Not covered: resumable Lookback through these two entry points (the caller-supplied history window is another interface: 4i, and its index 4j),
 *   extending an index from its last cursor, cursors written by the encoder, the host-buffer pco_page_decompressor_* handle. */
#define PCO_GFX_CURSOR_GENERAL 1u
enum PcoError pco_gfx_decompress_page_reads_ex(size_t n_tasks, const PcoGfxPageReadTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                               PcoGfxTaskResult* d_results, void* stream);
enum PcoError pco_gfx_index_pages_ex(size_t n_tasks, const PcoGfxPageIndexTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                     PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4i. LOOKBACK pages in slices: a HISTORY ring beside the cursor.  What the reference's PageDecompressor carries between two reads is the tANS
 *     and bit state and, under Lookback, its window_buffer (delta/lookback.rs:187-246).  The first is a cursor; the second is the caller's
 *     history buffer here, read by a task and updated in place, so that a slice of a Lookback page costs its own batches and nothing in front.
 *     pco_gfx_decompress_page_reads_hist is 4h's read entry point with a history per task; the older entry points are what they were.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxPageReadHistTask {   /* 104 bytes: PcoGfxPageReadTask's fields in its order, then the history */
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes, as in PcoGfxPageTask */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one page; 16 readable bytes past page_len */
  uint64_t page_len;
  void* dst;             /* DEVICE: room for `count` numbers, nothing more */
  uint64_t page_n;       /* numbers in the WHOLE page */
  uint64_t first, count; /* the rows wanted: first + count <= page_n */
  uint32_t dtype;
  uint32_t format_major;
  const PcoGfxPageCursor* from;   /* DEVICE, or NULL: the page's start */
  PcoGfxPageCursor* to;           /* DEVICE, or NULL: not wanted.  May equal `from` */
  void* history;         /* DEVICE, 8-byte aligned, or NULL: the page's lookback history, read by the task and updated in place */
  uint64_t history_len;  /* bytes at `history`; 0 iff history == NULL */
} PcoGfxPageReadHistTask;
#define PCO_GFX_HISTORY_HEADER_BYTES 64
/* 64 + (1 << window_n_log) * width(dtype): the bytes a page's history takes (window_n_log: pco_gfx_chunk_meta_info).  0 for an invalid dtype or a
 *   window_n_log outside 1..24. */
size_t pco_gfx_lookback_history_bytes(uint32_t window_n_log, unsigned char dtype);
/* flags: 0 or PCO_GFX_CURSOR_GENERAL, with 4h's meaning for the pages without Lookback; any other bit is PCO_GFX_INVALID_ARGUMENT before anything is
 *   launched.
 * A task with history == NULL: every dst, cursor and result is bit-identical to pco_gfx_decompress_page_reads_ex with the same flags, Lookback pages
 *   included (kind 2, the prefix decode).
 * A task with a history on a page without Lookback: the history is neither read nor written; the task is the _ex task.
 * A task with a history on a RESUMABLE Lookback page -- Lookback on the primary variable in Classic, IntMult, FloatMult or FloatQuant mode, any table
 *   size the general kernel decodes, state_n <= 256, no delta'd secondary variable -- writes and accepts cursor KIND 4 (version 1):
 *     w[0..3]     as kind 1: version | kind = 4, row, bit position, page_n | dtype
 *     w[4..9]     the state indices of the delta variable (v = 0), the primary and the secondary, 0 for a variable the page does not have
 *     w[10..31]   0
 *   The verdict on a kind-4 `from` is kind 3's list: version, kind, page_n, dtype, at > first, at neither a multiple of 256 nor page_n, a bit
 *   position outside the page's body, a state index >= 2^ans_size_log, a walk of more batches than the host gave scratch for.
 * The history buffer: a 64-byte header -- the 64-bit words version = 1, row, page_n | dtype << 32, window_n_log, 0, 0, 0, 0 -- and a ring of
 *   window_n = 1 << window_n_log latents of the number's width.  The ring holds the primary-latent history F of delta/lookback.rs (in Classic mode
 *   the ordered latents of the numbers, in the other modes the primary latents), F[j] in slot j & (window_n - 1).  A buffer stamped row = r holds
 *   F[j] for every j in [max(0, r' - window_n), r'), r' = min(r + state_n, page_n): the decoder's output lags its deltas by state_n, so the state_n
 *   rows behind the cursor are computed already and live in the ring.  Slots no row has reached keep the caller's bytes.
 * The walk covers batches [at / 256, ceil((first + count) / 256)), into prefix scratch relative to `at`, as 4h's general reads do.  A lookback to a row
 *   in front of `at` reads the ring, one to a row inside the walk reads the scratch (its first state_n rows are seeded from the ring), one to a row
 *   before 0 adds nothing.  The ring is read-only during the walk.
 * The update: on PCO_GFX_OK with to != NULL the task writes `to` and then, out of the scratch, the last min(window_n, rows walked) rows of F it
 *   computed -- no slot twice -- and stamps the header with `to`'s row.  On any other status, or with to == NULL, neither `to` nor a byte of the
 *   history changes: the history moves if and only if `to` does, so a reader that reads part of a batch without moving its cursor keeps a consistent
 *   pair.  to == from and the update in place are legal.  Cursor and history bytes are a function of the page and the row only: identical whether the
 *   row was reached in one read or in many.  (In the two-variable modes the join is made in place in a second pass that repeats the first one's walk
 *   and cannot fail where that did not: there the pair moves between the passes, behind every check of the task.)
 * Starting a page: with from == NULL the page starts at row 0 and the header need not be valid; history_len is still checked, and the update
 *   initialises the buffer.
 * Device verdicts, made after the ChunkMeta and the page header are parsed, on ONE copy of the cursor and of the header; each is
 *   PCO_GFX_INVALID_ARGUMENT with nothing of dst, `to` or the history written: history_len < 64 + window_n * width; a kind-4 `from` whose header's
 *   version, page_n | dtype or window_n_log is not the page's, or whose header row is not the cursor's row; a kind-2 `from` together with a history
 *   on a resumable page; a kind-4 `from` with history == NULL.  These bound every address formed: ring slots are masked with window_n - 1 inside a
 *   checked length, scratch indices are bounded by the batches the host gave.  A stamped pair that belongs to ANOTHER page gives wrong numbers,
 *   PCO_GFX_INSUFFICIENT_DATA or PCO_GFX_CORRUPTION, never an access outside the page, the tables, the scratch or the ring.
 * Host checks, made before a device is asked for, `results` untouched: 4f's ten-field checks, an unknown flag bit, history != NULL with
 *   history_len == 0 or the reverse, a misaligned history.  n_tasks == 0 succeeds without a device.
 * Forms, streams, passes under PCO_GFX_WORKSPACE_GB: as 4h; a synchronous call sizes its scratch from the rows of the kind-4 `from` cursors as it
 *   does for kind 3.  A history a task updates must not be another task's history in the same call.
 * Not covered: Dict under Lookback, a delta'd secondary variable under Lookback and state_n > 256 are not resumable -- they keep kind 2 and 4f's
 *   behaviour (PCO_GFX_UNSUPPORTED where 4d gives it), and a history given with them is ignored; the host-buffer pco_page_decompressor_* handle. */
enum PcoError pco_gfx_decompress_page_reads_hist(size_t n_tasks, const PcoGfxPageReadHistTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                                 PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4j. Indexing a LOOKBACK page in one walk: a history snapshot beside each cursor.  4i's kind-4 cursor / history pairs come from a chain of reads, one
 *     history following one cursor; pco_gfx_index_pages_hist is 4h's index entry point with k history buffers per task, so that ONE walk of a page
 *     leaves the k pairs its segments are then decoded from side by side, in one pco_gfx_decompress_page_reads_hist call with to == NULL (which leaves
 *     a pair untouched: an index is reusable).  The older entry points are what they were.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxPageIndexHistTask {   /* 80 bytes: PcoGfxPageIndexTask's fields in its order, then the histories */
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes, as in PcoGfxPageTask */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one page; 16 readable bytes past page_len */
  uint64_t page_len;
  PcoGfxPageCursor* cursors;   /* DEVICE, 8-byte aligned: room for k = pco_gfx_page_index_len(page_n, every_rows) cursors */
  uint64_t page_n;       /* numbers in the WHOLE page */
  uint64_t every_rows;   /* a positive multiple of 256 */
  uint32_t dtype;
  uint32_t format_major;
  void* histories;          /* DEVICE, 8-byte aligned, or NULL: k history buffers, history i at histories + i * history_stride */
  uint64_t history_stride;  /* bytes between two histories: a multiple of 8; 0 iff histories == NULL */
} PcoGfxPageIndexHistTask;
/* flags: 0 or PCO_GFX_CURSOR_GENERAL, with 4h's meaning for the pages without Lookback; any other bit is PCO_GFX_INVALID_ARGUMENT before anything is
 *   launched.
 * A task with histories == NULL: cursors and result are bit-identical to pco_gfx_index_pages_ex with the same flags, Lookback pages included (kind 2,
 *   aux bit 0 = 1).
 * A task with histories on a page without Lookback, or on a Lookback page 4i calls not resumable (Dict under Lookback, a delta'd secondary variable,
 *   state_n > 256): the histories are neither read nor written; the task is the _ex task.
 * A task with histories on a RESUMABLE Lookback page: the page is walked ONCE over batches [0, k * every_rows / 256) -- tANS walk, offset unpack and
 *   the lookback decode of the primary latents; no mode join, no rows stored (in the two-variable modes 4i's first pass only: the secondary's states
 *   are walked, the cursor carries them).  cursors[i] is the KIND-4 cursor in front of row r_i = (i + 1) * every_rows; history i is stamped r_i and its
 *   ring holds F[j] for j in [max(0, r' - window_n), r'), r' = min(r_i + state_n, page_n), slots no row has reached keeping the caller's bytes.  Both
 *   are byte-identical to the pair a pco_gfx_decompress_page_reads_hist chain leaves when it reaches r_i, over the first 64 + window_n * width bytes
 *   of each history; the bytes of the stride behind those, and everything outside cursors[0..k) and the k history extents, are never written.  The
 *   result is {n_out k, consumed 0, PCO_GFX_OK, aux 0}.
 * Device verdict, made after the ChunkMeta and the page header are parsed, with nothing of the cursors or histories written:
 *   PCO_GFX_INVALID_ARGUMENT for history_stride < pco_gfx_lookback_history_bytes(window_n_log, dtype) on a resumable page (window_n_log lives in
 *   the ChunkMeta, on the device: the host cannot check it).
 * A page whose bytes end inside the walked prefix is PCO_GFX_INSUFFICIENT_DATA; one damaged behind its last cursor is PCO_GFX_OK.  On any status but
 *   PCO_GFX_OK or the refusal above the task's cursor slots and history extents hold unspecified bytes; bytes outside them stay untouched, and
 *   neighbouring tasks are unaffected.
 * k == 0: PCO_GFX_OK with n_out 0; nothing of the task is read, and `cursors` and `histories` may be NULL.
 * Host checks, made before a device is asked for, `results` untouched: 4g's list, an unknown flag bit, histories != NULL with history_stride == 0
 *   or the reverse, a stride that is no multiple of 8, misaligned histories.  n_tasks == 0 succeeds without a device.
 * Forms and streams: as 4g; the asynchronous form makes no host synchronisation.
 * Scratch: a task that snapshots needs F of its walked prefix -- k * every_rows + state_n rows of the number's width, in prefix scratch as a range
 *   task {0, k * every_rows} takes it -- and only the device knows which tasks are resumable Lookback pages.  The ASYNCHRONOUS form takes that
 *   scratch up front for every task with histories != NULL, whatever its page turns out to be.  The SYNCHRONOUS form gives every task 4g's two
 *   batches, gets the tasks that need more handed back, and runs those in passes under PCO_GFX_WORKSPACE_GB, as a range call does for its scratch
 *   route (a pass reserves twice a task's prefix: the round is the one that brings a delta'd secondary's history).  Tasks without histories keep their
 *   two batches in both forms.  The rings are copied out of the scratch by a kernel of its own behind the walk.
 * Not covered: Dict under Lookback, a delta'd secondary variable under Lookback and state_n > 256 (kind 2, as 4i), extending an index from its last
 *   pair. */
enum PcoError pco_gfx_index_pages_hist(size_t n_tasks, const PcoGfxPageIndexHistTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                       PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4k. Page reads and page indexes from a page directory in DEVICE memory: 4i's read entry point and 4j's index entry point behind 4e's directory.
 *     The entry points of 4f .. 4j take meta and page as pointers and lengths, which a host has only after it has read the directory back; these
 *     two name them by PIECE INDEX, as 4e's do, so that encode -> compact -> index -> decode every page as side-by-side segments (or read rows from
 *     the nearest cursor) is one stream-ordered pipeline with one synchronisation at its end.  It also leaves the cursors at WRITE time without
 *     touching an encode kernel.  The PcoGfxDirectory is 4e's; the older entry points are what they were.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxDirPageReadTask {   /* 80 bytes: PcoGfxDirPageRangeTask's fields in its order, then PcoGfxPageReadHistTask's last four */
  void* dst;             /* DEVICE: room for `count` numbers, nothing more */
  uint64_t page_n, first, count;   /* numbers in the WHOLE page; the rows wanted: first + count <= page_n */
  uint32_t meta_piece, page_piece, dtype, format_major;
  const PcoGfxPageCursor* from;   /* DEVICE or NULL */
  PcoGfxPageCursor* to;           /* DEVICE or NULL; may equal from */
  void* history;                  /* DEVICE, 8-byte aligned, or NULL */
  uint64_t history_len;           /* 0 iff history == NULL */
} PcoGfxDirPageReadTask;
typedef struct PcoGfxDirPageIndexTask {  /* 56 bytes */
  PcoGfxPageCursor* cursors;      /* DEVICE, 8-byte aligned: room for k = pco_gfx_page_index_len(page_n, every_rows) cursors */
  uint64_t page_n, every_rows;    /* numbers in the WHOLE page; a positive multiple of 256 */
  uint32_t meta_piece, page_piece, dtype, format_major;
  void* histories;                /* DEVICE, 8-byte aligned, or NULL */
  uint64_t history_stride;        /* multiple of 8; 0 iff histories == NULL */
} PcoGfxDirPageIndexTask;
/* pco_gfx_decompress_page_reads_hist / pco_gfx_index_pages_hist with each task's meta, meta_len, page and page_len taken from the directory ON THE
 *   DEVICE.  `tasks` and `*dir` are HOST memory; the library copies them, and they may be overwritten as soon as the call returns.
 * flags: 0 or PCO_GFX_CURSOR_GENERAL, with 4h's meaning; any other bit is PCO_GFX_INVALID_ARGUMENT on the host.
 * Equivalence: for a well-described task dst, `to`, the history, the cursors, the histories and the task's result are bit-identical to what the
 *   pointer form -- pco_gfx_decompress_page_reads_hist, pco_gfx_index_pages_hist -- writes under the same flags, given the pointers and lengths the
 *   directory describes: every kind of cursor (1, 2, 3, 4), every refusal of a cursor or a history, a page damaged behind or inside the walk, aux and
 *   consumed.  (A task without a history is 4f's / 4h's read, one without histories 4g's / 4h's index, as there.)
 * Directory verdicts are 4e's four, made on the device in 4e's order.  A task that fails one has the result {status, n_out 0, consumed 0, aux 0};
 *   nothing of the blob is read for it, and neither is its `from` cursor or its history's header; no byte is written of dst, `to`, the history, the
 *   task's cursor slots or its histories.  A kept page of 0 bytes is legal, as in 4e.  A read with count == 0, or an index task with k == 0, is
 *   PCO_GFX_OK and reads neither the directory's entries nor the blob, whatever its pieces look like.
 * Forms: results / d_results select the synchronous and the asynchronous form as everywhere in 4.  The asynchronous form makes no host
 *   synchronisation and reads nothing of the directory on the host.  The synchronous form may read the rows of the `from` cursors back, as the
 *   pointer form does: those are the caller's pointers, not the directory's.  Scratch, passes under PCO_GFX_WORKSPACE_GB, caller streams and two
 *   streams on one workspace: as in the pointer forms.  The work is the pointer form's kernels behind ONE small resolve kernel.
 * Host checks, made before a device is asked for, `results` untouched: an unknown flag bit; NULL tasks with n_tasks > 0; 4e's list (a NULL dir,
 *   d_blob or d_offsets; n_pieces >= 2^31; results and d_results both NULL; a piece index >= n_pieces; meta_piece == page_piece); 4f's / 4g's
 *   field checks and 4i's / 4j's history checks, in the order of those entry points.  PCO_GFX_CORRUPTION for format_major > 4, else
 *   PCO_GFX_INVALID_ARGUMENT.  (Like 4e's, they refuse a call without results even when it has no tasks.)
 * Not covered: a page_n that lives on the device, extending an index from its last pair.  (Standalone chunks behind pco_gfx_compact_chunks' offsets: 4l.) */
enum PcoError pco_gfx_decompress_page_reads_dir(size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);
enum PcoError pco_gfx_index_pages_dir(size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                      PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);
/* the window_n_log a Lookback chunk of n numbers gets from this library and from the reference's encoder (delta/mod.rs:37-48): what a caller sizes
 *   histories by before the ChunkMeta exists (pco_gfx_lookback_history_bytes).  4 ..= 15; 0 for n == 0 or n > 2^24 */
int pco_gfx_lookback_window_n_log(uint64_t n);

/* ------------------------------------------------------------------------------------------
 * 4l. STANDALONE chunks from a directory in DEVICE memory: 4e's and 4k's entry points behind pco_gfx_compact_chunks' offsets.  pco_gfx_compress_chunks
 *     (with d_results) + pco_gfx_compact_chunks (total == NULL) leave a blob and d_offsets on the device, as the wrapped writer does; these three
 *     entry points decode, read and index the chunks behind them without a host synchronisation, so that encode -> compact -> index -> decode is one
 *     stream-ordered pipeline on the standalone surface too.  A standalone chunk is `dtype byte | 24-bit n - 1 | ChunkMeta | one page of n numbers`
 *     (standalone/compressor.rs:191-203), and the ChunkMeta's length follows from a handful of its header fields, so ONE small resolve kernel splits
 *     each task's chunk into the (meta, meta_len, page, page_len) the pointer forms take, with a few loads per task.  Every decode kernel, cursor and
 *     history is what it was, and cursors and indexes are interchangeable between the forms.
 *     The structs are 4e's and 4k's, unchanged: the PcoGfxDirectory describes pco_gfx_compact_chunks' d_dst / d_offsets (n_pieces = that call's
 *     n_tasks; gap = bytes of the caller's own framing in front of each chunk, 0 for what the compactor writes); in a task, page_piece names the
 *     CHUNK's piece, meta_piece must equal it, and page_n is the chunk's n, which the caller who encoded it knows.
 * ---------------------------------------------------------------------------------------- */
/* pco_gfx_decompress_pages_dir / pco_gfx_decompress_page_reads_dir / pco_gfx_index_pages_dir with each task's one piece a standalone chunk.
 * Forms, flags (0 or PCO_GFX_CURSOR_GENERAL), histories, scratch and passes, caller streams, two streams on one workspace: as in 4e and 4k.  A read
 *   task with NULL cursors and no history is a row range (4d).  The asynchronous form makes no host synchronisation and reads nothing of the
 *   directory on the host.  The work is the pointer form's kernels behind ONE resolve kernel.
 * Equivalence: for a well-described task dst, the result, every cursor and every history are byte-identical to those of the pointer form --
 *   pco_gfx_decompress_pages, pco_gfx_decompress_page_reads_hist (_ex without a history), pco_gfx_index_pages_hist (_ex without histories) -- given
 *   meta = chunk + 4, meta_len, page = meta + meta_len, page_len = the rest of the chunk, and format_major.
 * Chunk verdicts are made on the device, in this order, with c0 = d_offsets[page_piece], c1 = d_offsets[page_piece + 1].  A task that fails one has
 *   the result {status, n_out 0, consumed 0, aux 0}; no byte is written of dst, `to`, the history, the task's cursor slots or its histories; its `from`
 *   cursor and its history's header are not read; and of the blob nothing is read but the 4 preamble bytes and the ChunkMeta's header fields the
 *   verdict itself looked at:
 *     d_offsets[n_pieces] == ~0 (the compactor's "destination too small")                     PCO_GFX_INVALID_ARGUMENT
 *     c0 > c1 or c1 > blob_len                                                                PCO_GFX_INVALID_ARGUMENT
 *     c1 == c0: the compactor dropped the chunk                                               PCO_GFX_INSUFFICIENT_DATA
 *     c1 - c0 < gap                                                                           PCO_GFX_INVALID_ARGUMENT
 *     fewer than 4 bytes behind the gap                                                       PCO_GFX_INSUFFICIENT_DATA
 *     preamble byte 0 != the task's dtype (a terminator's 0 included)                         PCO_GFX_CORRUPTION
 *     1 + the little-endian 24 bits of preamble bytes 1..3 != page_n                          PCO_GFX_INVALID_ARGUMENT
 *     the ChunkMeta's header names an unknown mode or delta encoding                          PCO_GFX_CORRUPTION
 *     the ChunkMeta's header, or the length it gives, runs past the chunk                     PCO_GFX_INSUFFICIENT_DATA
 *   Otherwise the page is what is left behind the ChunkMeta; 0 bytes are legal (a constant chunk).  Every other validation of the ChunkMeta is the
 *   decode kernels', with the pointer form's result.  A read with count == 0, or an index task with k == 0, is PCO_GFX_OK and reads neither the
 *   directory's entries nor the blob, whatever its pieces look like.
 * Host checks, made before a device is asked for, `results` untouched: those of 4e / 4k in their order, with ONE difference: meta_piece !=
 *   page_piece is PCO_GFX_INVALID_ARGUMENT here (the page entry points keep refusing meta_piece == page_piece).
 * Not covered: a page_n that lives on the device (nothing given by the caller), extending an index from its last pair.  (Files of many chunks
 *   without a directory: 4m scans one.) */
enum PcoError pco_gfx_decompress_chunks_dir(size_t n_tasks, const PcoGfxDirPageTask* tasks, const PcoGfxDirectory* dir,
                                            PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);
enum PcoError pco_gfx_decompress_chunk_reads_dir(size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                 PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);
enum PcoError pco_gfx_index_chunks_dir(size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                       PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);
/* The same split of ONE standalone chunk in HOST memory (a reader of a .pco file walks its chunks with it): chunk[0 .. len) starts with the chunk's
 *   preamble; *n = its count of numbers, *meta_len = the ChunkMeta's bytes behind the 4 preamble bytes, *page_len = len - 4 - *meta_len (pass the
 *   chunk's exact extent for the page's exact length).  The verdicts are the table's from "fewer than 4 bytes" on, without the page_n comparison:
 *   PcoDecompressionError with that status as the last status; PcoInvalidType for a NULL argument or an invalid dtype.  Nothing touches the device. */
enum PcoError pco_gfx_standalone_chunk_split(const void* chunk, size_t len, unsigned char dtype, uint8_t format_major, uint64_t* n,
                                             uint64_t* meta_len, uint64_t* page_len);

/* ------------------------------------------------------------------------------------------
 * 4m. The chunk directory of a standalone FILE, scanned on the device.  A .pco file that the reference's simple_compress or the pco CLI wrote is a
 *     header, chunks back to back and a terminator; it stores no chunk lengths, and a chunk's end follows only from walking its tANS chain.
 *     pco_gfx_scan_chunks walks many such streams side by side -- one wave per stream, no rows stored, no host round trip per chunk -- and
 *     leaves, in device memory, exactly the d_offsets a PcoGfxDirectory takes, and each chunk's count beside them.  Behind it everything 4l offers
 *     works on a foreign file: PcoGfxDirectory{src, src_len, d_offsets, n_out, gap 0}, with page_n = d_counts[k] and meta_piece == page_piece == k.
 *     A scan is paid once per file; its two arrays are the sidecar index a caller keeps.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxScanTask {   /* 48 bytes */
  const void* src;        /* DEVICE: [file header] chunk ... chunk [terminator]; 16 readable bytes past src_len */
  uint64_t src_len;
  uint64_t* d_offsets;    /* DEVICE: max_chunks + 1 entries */
  uint32_t* d_counts;     /* DEVICE: max_chunks entries, chunk k's n */
  uint32_t max_chunks;    /* 1 .. 2^31 - 1 */
  uint32_t dtype;
  uint32_t flags;         /* PCO_GFX_TASK_HAS_FILE_HEADER, or bits 8..15 = the format's major version as for PCO_GFX_TASK_ONE_CHUNK (0: the current one) */
  uint32_t reserved;      /* 0 */
} PcoGfxScanTask;
/* `tasks`: HOST array, copied.  results / d_results: the synchronous or the asynchronous form, as everywhere; the asynchronous form makes no host
 *   synchronisation.  Global table scratch for tANS tables beyond the kernel's LDS budget is taken up front in both forms (832 KB per block, at most
 *   4096 blocks), as an asynchronous decode takes it.
 * Per task the call leaves d_offsets[k], the byte offset in src of chunk k's preamble (its dtype byte), and d_counts[k], its n, for k < n_out;
 *   d_offsets[n_out], the byte behind the last chunk found -- where the terminator, the next chunk or the failing chunk lies; with a file header in
 *   front d_offsets[0] is the header's length, and 0 when the header itself is refused -- and nothing else of either array.
 * The result: n_out = the chunks found; consumed = d_offsets[n_out], plus 1 when the terminator was taken; status = the first verdict that is not
 *   PCO_GFX_OK, which keeps the chunks in front of it; aux bit 0 = another chunk follows (the scan stopped at max_chunks: continue at src + consumed
 *   with the version in flags and no header flag), bit 1 = the terminator was there and is consumed, both clear on a failure; aux bits 8..15 = the
 *   format's major version the scan used (the header's, the flags', or 4).  A stream with neither header nor terminator (pco_gfx_compact_chunks'
 *   blob) ends at src_len with PCO_GFX_OK and both bits clear.  A file of a header and a terminator: n_out 0, d_offsets[0] the terminator's offset,
 *   aux bit 1.
 * The contract: the scan equals the CHAIN of pco_gfx_decompress_chunks calls that pco_standalone_simple_decompress_into makes -- one task {src + off,
 *   src_len - off, room for 2^24 numbers, PCO_GFX_TASK_ONE_CHUNK}, the first with PCO_GFX_TASK_HAS_FILE_HEADER when the scan task has it, the later
 *   ones with the version, while aux bit 0 is set and fewer than max_chunks chunks are decoded.  n_out is the chain's count of steps that decoded a
 *   chunk, d_counts their n_out, d_offsets the running sums of their consumed (a terminator's byte belongs to consumed alone), status the first
 *   status that is not OK.  So a file that ends right behind its FIRST chunk is PCO_GFX_INSUFFICIENT_DATA with n_out 0, as the header step of the
 *   chain is, and one that ends behind a later chunk is PCO_GFX_OK without aux bit 1.  (One thing is said more plainly than the chain says it: its
 *   step on `header, terminator` reports the terminator's byte in consumed and no aux bit; the scan sets bit 1.)
 *   Everything the ChunkMeta's validation, the table construction and the bit stream's bounds decide agrees with the chain, status for status.
 *   NOT checked, because it needs a row's VALUE and the scan computes no rows -- the scan reports PCO_GFX_OK with the boundary the framing gives,
 *   and the decode that follows reports PCO_GFX_CORRUPTION:
 *     a Dict index beyond the dictionary.
 *   (A lookback beyond the window IS checked: the lookback variable's latents are no rows, and the scan unpacks them for that verdict alone.)
 * The file header's verdicts (pco_scan.h, the decode kernels' own in their order), on src[0 .. src_len):
 *     fewer than 4 bytes                                                                      PCO_GFX_INSUFFICIENT_DATA
 *     bytes 0..3 are not "pco!"                                                               PCO_GFX_CORRUPTION
 *     byte 4 < 2: no standalone version byte; byte 4 is the wrapped header's already
 *     byte 4 >= 3 and byte 5, the uniform type, neither 0 nor a number type                   PCO_GFX_CORRUPTION
 *     the n_hint varint (6 bits of power, power + 1 bits) ends in padding that is not zero,
 *       and the file holds its last byte                                                      PCO_GFX_CORRUPTION
 *     the file ends inside the varint                                                         PCO_GFX_INSUFFICIENT_DATA
 *     byte 4 > 3                                                                              PCO_GFX_CORRUPTION
 *     the format's major version > 4                                                          PCO_GFX_CORRUPTION
 *     the file ends in front of the major version, or of the minor one (major 4)              PCO_GFX_INSUFFICIENT_DATA
 *   then per chunk: the stream ends where a file's first preamble would stand, or inside a preamble: PCO_GFX_INSUFFICIENT_DATA; a type byte that is
 *   not the task's dtype (or, for a file's first chunk, not the header's uniform type): PCO_GFX_CORRUPTION.
 * Host checks, made before a device is asked for, PCO_GFX_INVALID_ARGUMENT, nothing launched, `results` untouched, in this order: NULL tasks with
 *   n_tasks > 0; results and d_results both NULL; then per task NULL src, d_offsets or d_counts; max_chunks 0 or >= 2^31; an invalid dtype;
 *   reserved != 0; flag bits other than PCO_GFX_TASK_HAS_FILE_HEADER and bits 8..15; d_offsets not 8-byte or d_counts not 4-byte aligned.
 *   n_tasks == 0 succeeds without a device.
 * Not covered: a page_n that lives on the device for 4l's entry points (a caller reads d_counts back once), extending an index from its last pair,
 *   a shorter chain (the format fixes it). */
enum PcoError pco_gfx_scan_chunks(size_t n_tasks, const PcoGfxScanTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream);

/* ------------------------------------------------------------------------------------------
 * 4n. Rows by ROW ID from indexed pages: the ids live on the device -- a filter on another column (late materialisation), a sampler, a join --
 *     and stay there.  The page is cut at its index's cursors (4g) into segments; a kernel decides from the ids which segments are walked and how
 *     far, the resume route of 4f decodes exactly those side by side, and a gather moves the wanted rows to dst.  Filter -> take is one
 *     stream-ordered pipeline: nothing of d_rows is read on the host.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxTakeTask {   /* 96 bytes */
  const void* meta;      /* DEVICE: the chunk's ChunkMeta bytes, as in PcoGfxPageReadTask */
  uint64_t meta_len;
  const void* page;      /* DEVICE: one wrapped page; 16 readable bytes past page_len */
  uint64_t page_len;
  uint64_t page_n;       /* numbers in the WHOLE page, 1 ..= 2^24 */
  uint64_t row_base;     /* the id of the page's row 0 in the caller's numbering (its chunk, its file) */
  const PcoGfxPageCursor* cursors;   /* DEVICE: what pco_gfx_index_pages[_ex] left for (page_n, every_rows); NULL: no index */
  uint64_t every_rows;   /* the index's stride; 0 iff cursors == NULL */
  const uint64_t* d_rows;   /* DEVICE, 8-byte aligned: n_rows row ids, any order, duplicates allowed */
  uint64_t n_rows;       /* < 2^32 */
  void* dst;             /* DEVICE: n_rows numbers, aligned to the number type */
  uint32_t dtype;
  uint32_t format_major;
} PcoGfxTakeTask;
/* Output: for every j with row_base <= d_rows[j] < row_base + page_n, dst[j] is row d_rows[j] - row_base of the page, bit-identical to what
 *   pco_gfx_decompress_pages writes there.  An id outside the page is NOT this task's: dst[j] is left untouched and the row is not counted --
 *   so the pages of one chunk share one d_rows / dst pair as several tasks with different row_base, and write disjoint entries.  No byte outside
 *   dst[0 .. n_rows * width) is ever written.
 * Segments: with an index the page is cut at the cursors' rows into pco_gfx_page_index_len(page_n, every_rows) + 1 segments; segment s >= 1
 *   starts from cursors[s - 1], segment 0 from the page's start.  Without one the page is one segment.  A segment none of whose rows is wanted is
 *   not walked, and nothing of the page is read for it.  A wanted segment is walked from its start to batch
 *   ceil((its largest wanted local row + 1) / 256) and no further: it is exactly the read task {first = s * every_rows, count = largest wanted
 *   row + 1 - first, from = its cursor, to = NULL} of 4f / 4h, and its verdicts, reach and cursor kinds are that task's -- kind 1; kind 3 under
 *   PCO_GFX_CURSOR_GENERAL in `flags`; a cursor of the wrong kind refused on the device; a page damaged behind the last wanted batch still
 *   PCO_GFX_OK.  The host states every segment's start row (s * every_rows) itself and reads no cursor back: a cursor that stands elsewhere -- an
 *   index of another stride -- is refused on the device (at > first, or a walk longer than the scratch: PCO_GFX_INVALID_ARGUMENT).  One thing
 *   differs from the read task: a segment s >= 1 behind a POSITION-ONLY cursor (kind 2: Lookback, and Conv1 / Dict / wide tables without the flag)
 *   would decode its whole prefix, and gets no scratch for it here: PCO_GFX_UNSUPPORTED.  Such pages are taken with cursors == NULL.
 * Results, per task.  On PCO_GFX_OK: n_out = the ids inside the page (a caller sums it over a chunk's pages and compares with n_rows to find ids
 *   no page owned), aux = the segments walked, consumed = the batches walked, summed over them -- a pure function of the ids, page_n and
 *   every_rows.  When a wanted segment fails, the status is that of the lowest failing one and n_out = consumed = aux = 0; the dst entries of
 *   this task's in-page rows are unspecified, everything else is untouched, and neighbouring tasks are unaffected.  n_rows == 0, or no id inside
 *   the page: PCO_GFX_OK, zeros, and nothing of the page, the meta or the cursors is read.
 * Forms, streams, two streams on one workspace: as pco_gfx_decompress_page_reads_ex.  The asynchronous form (results == NULL) makes no host
 *   synchronisation; the synchronous form synchronises once, to fetch the results, and a failing task sets the last error.
 * Host checks, made before a device is asked for, `results` untouched, PCO_GFX_INVALID_ARGUMENT, in this order: NULL tasks with n_tasks > 0;
 *   results and d_results both NULL; a flag bit other than PCO_GFX_CURSOR_GENERAL; then per task an invalid dtype; page_n == 0 or > 2^24; a NULL
 *   meta or page; row_base + page_n wrapping; every_rows not a multiple of 256; every_rows == 0 with cursors, or no cursors where the index has
 *   any; misaligned cursors; n_rows > 0 with a NULL or misaligned d_rows, then dst; n_rows >= 2^32; more than 2^31 segments in the call so far;
 *   and format_major > 4, which is PCO_GFX_CORRUPTION as everywhere.  n_tasks == 0 succeeds without a device.
 * Scratch, taken up front in both forms -- there are no passes:
 *     sum over tasks of page_n * width                                   the decoded-row areas (each rounded up to 256 bytes)
 *   + segments of the call * 3 * (W + 256), W = the longest segment's rows rounded up to a batch: min(every_rows, page_n), page_n without an index
 *                                                                        the symbols of the walks: per SEGMENT, not per page
 *   + the scratch route's extents, (a segment's batches + 1) * 256 numbers each: for segment 0 of every task, and under
 *     PCO_GFX_CURSOR_GENERAL for every segment
 *   A call beyond PCO_GFX_WORKSPACE_GB (default 80 % of the free device memory) is PCO_GFX_INVALID_ARGUMENT, "split the call".
 * Where another call is the better one (MI355X, 64 pages of 2^20 u64 indexed every 4096 rows): every task scans the WHOLE id
 *   list twice (mark, gather), so the cost grows with pages * ids.  Uniformly random ids touch every segment whatever their number, and then the
 *   segment-parallel pco_gfx_decompress_page_reads of the whole index followed by a gather of the caller's is faster at every fraction measured
 *   (0.96 against 1.02 ms at 0.1 %, 2.3 against 25.8 ms at 100 %); whole-page pco_gfx_decompress_pages + gather is faster from 10 % unsorted
 *   (4.4 against 4.5 ms) and at 100 % (5.6 against 25.8 ms unsorted, 4.5 against 15.3 ms sorted).  The take is the better call for CLUSTERED ids --
 *   a contiguous 1 % run: 0.64 ms against 0.96 and 4.1 -- for few pages per id list, and wherever a host synchronisation in mid-pipeline is the cost.
 * Not covered: Lookback pages with histories (4i / 4j) -- they are taken with cursors == NULL, one prefix walk to the last wanted row, as a
 *   range; the _dir forms; 32-bit row ids; passes under a budget. */
enum PcoError pco_gfx_take_rows(size_t n_tasks, const PcoGfxTakeTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results,
                                void* stream);

/* ChunkMeta accessors(wrapped/chunk_compressor.rs:549 ChunkCompressor::meta, wrapped/chunk_decompressor.rs:62 ChunkDecompressor::meta,
 * standalone/decompressor.rs:288): what the reference's `ChunkMeta` says about a chunk -- mode, delta encoding, and per latent variable the
 * tANS size and bin count -- read back from the metadata BYTES (the bytes pco_chunk_compressor_write_meta writes / the prefix
 * pco_chunk_decompressor_new consumed), so a host that wants the full `ChunkMeta` (every bin) can equally hand those bytes to the
 * reference's own ChunkMeta::read_from.  Dict mode and Conv1 delta report their kinds (Conv1's parameters: pco_gfx_chunk_meta_conv1); the
 * per-variable fields are filled as far as the layout is parsed (n_vars_parsed). */
typedef struct PcoGfxChunkMetaInfo {
  uint32_t mode_kind;            /* 0 Classic, 1 IntMult, 2 FloatMult, 3 FloatQuant, 4 Dict (metadata/mode.rs) */
  uint32_t mode_k;               /* FloatQuant: k */
  uint64_t mode_base_latent;     /* IntMult / FloatMult: the base as the number type's ordered latent (to_latent_ordered) */
  uint32_t delta_kind;           /* 0 None, 1 Consecutive, 2 Lookback, 3 Conv1 (metadata/delta_encoding.rs) */
  uint32_t delta_order;          /* Consecutive */
  uint32_t window_n_log, state_n_log;   /* Lookback */
  uint32_t secondary_uses_delta;
  uint32_t n_vars_parsed;        /* 3 when every present variable's header was reached */
  uint32_t present[3], ans_size_log[3], n_bins[3];   /* [0] delta variable, [1] primary, [2] secondary */
  uint64_t meta_bytes;           /* length of the ChunkMeta in bytes (when n_vars_parsed == 3) */
} PcoGfxChunkMetaInfo;
enum PcoError pco_gfx_chunk_meta_info(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, PcoGfxChunkMetaInfo* out);
enum PcoError pco_chunk_compressor_meta_info(const PcoGfxChunkCompressor*, unsigned char dtype, PcoGfxChunkMetaInfo* out);
enum PcoError pco_chunk_decompressor_meta_info(const PcoGfxChunkDecompressor*, PcoGfxChunkMetaInfo* out);
/* The Conv1 parameters of a ChunkMeta (metadata/delta_encoding.rs:239-252), read back from its bytes: quantization, bias, `*order` weights (weights
 * has room for 32).  A ChunkMeta whose delta encoding is not Conv1 gives *order = 0 and PcoSuccess. */
enum PcoError pco_gfx_chunk_meta_conv1(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, uint32_t* quantization,
                                       int64_t* bias, int32_t* weights, uint32_t* order);
/* The dictionary of a Dict-mode ChunkMeta (metadata/mode.rs:138-165), read back from its bytes: *n_unique entries, written to `values` as ordered
 * latents of the number type's width (dtype_bits / 8 bytes each) when they fit its `cap` entries (else PCO_GFX_INVALID_ARGUMENT, with *n_unique set).
 * A ChunkMeta whose mode is not Dict gives *n_unique = 0 and PcoSuccess. */
enum PcoError pco_gfx_chunk_meta_dict(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, uint32_t* n_unique, void* values,
                                      size_t cap);

/* ------------------------------------------------------------------------------------------
 * 5. Chunk-sharded files over RCCL / xGMI (one process per GPU).  Chunks are independent (standalone/simple.rs:62-91: header |
 *    chunk | chunk ... | 0x00), so ranks encode contiguous blocks of chunks with no collective on the data path; assembling ONE
 *    file is a gather-v of the ranks' compacted chunk bytes (pco_gfx_compact_chunks) to a root, decoding a file that lives on one
 *    rank the mirror-image scatter.  RCCL is loaded on first use.  All buffers are DEVICE buffers; `stream` as above.
 *
 *    Bootstrap like ncclCommInitRank: rank 0 calls pco_gfx_comm_unique_id and hands the 128 bytes to the other ranks by whatever
 *    channel the host has (MPI, TCP, a file); every rank then calls pco_gfx_comm_init on ITS device.
 * ---------------------------------------------------------------------------------------- */
typedef struct PcoGfxComm PcoGfxComm;
enum PcoError pco_gfx_comm_unique_id(void* id128);
enum PcoError pco_gfx_comm_init(const void* id128, int n_ranks, int rank, PcoGfxComm** out);
void pco_gfx_comm_free(PcoGfxComm*);
int pco_gfx_comm_rank(const PcoGfxComm*);
int pco_gfx_comm_size(const PcoGfxComm*);
/* Every rank passes its compacted chunk stream [d_stream, d_stream + n_bytes); on `root` the streams land in rank (= chunk) order
 * at d_file + file_offset.  offsets (HOST array of n_ranks + 1 entries, filled on EVERY rank) = where each rank's bytes start
 * relative to file_offset, the total last.  A 16-byte all-gather (every rank's size + the root's room), then one ncclGroup of
 * exact-size ncclSend / ncclRecv.  The call synchronises `stream` for the sizes; the byte transfers are asynchronous on it.
 * d_file / file_cap are ignored off the root.  Failure is COLLECTIVE: a root whose buffer is missing or too small for the gathered
 * bytes makes EVERY rank return INVALID_ARGUMENT (offsets filled) before any send or receive is posted -- nobody is left waiting.
 * The call makes the communicator's device current. */
enum PcoError pco_gfx_gather_chunks(PcoGfxComm*, int root, const void* d_stream, uint64_t n_bytes, void* d_file, uint64_t file_cap,
                                    uint64_t file_offset, uint64_t* offsets, void* stream);
/* The decode direction: `root` holds the chunk stream at d_file + file_offset; rank r receives bytes [offsets[r], offsets[r + 1])
 * into d_stream (capacity stream_cap, >= its share + the decoder's 16 bytes of slack).  *n_bytes = this rank's share.  Every rank
 * passes the SAME offsets table (the one pco_gfx_gather_chunks filled, or the root's, broadcast by the host).  Collective failure as
 * above: one rank whose buffer is too small (or a root without a file buffer, or tables that disagree on the total) makes every
 * rank return INVALID_ARGUMENT after a 16-byte all-gather and before any transfer. */
enum PcoError pco_gfx_scatter_chunks(PcoGfxComm*, int root, const void* d_file, uint64_t file_offset, const uint64_t* offsets,
                                     void* d_stream, uint64_t stream_cap, uint64_t* n_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * 6. Test hook (NOT part of the drop-in surface; exported so that the GPU tests can check the device's arithmetic operation by
 *    operation against an IEEE reference).  Stage 1 of ModeSpec::Auto detection on floats (mode/float_mult.rs:145-275,
 *    mode/float_quant.rs:73-118) run on a host array taken as the sample, in order.  out[0..66]: s_size, tz5, n_gcd, sim[3],
 *    hist[56], has_euclid, k, n_ints, base_c (lo, hi).  Returns a PcoGfxStatus.
 * ---------------------------------------------------------------------------------------- */
int pco_gfx_debug_float_screen(const void* values, size_t n, uint32_t dtype, uint32_t* out);
/* Which kernel decided each lookback page (DeltaSpec::TryLookback) of the calling thread's last encode pass (after a SYNCHRONOUS encode call
 * on the current device; a call beyond the workspace budget runs in several passes).  Waits for the device, then writes out[k] for the first `cap` lookback pages in the call's page order:
 * 0 = the four-wave pipeline, 1 = screened and decided by the element-by-element kernel, 2 = decided by the one-wave kernel (handed back
 * by the pipeline, or screened and declined by the element-by-element kernel).
 * Which of them decides a page changes no byte; the tests use this to see that a row reached the kernel it was built for.  Returns the
 * number of lookback pages of that pass (0: that pass had none, or the workspace was released since), or -PcoGfxStatus.  Reads only. */
int64_t pco_gfx_debug_lookback_routes(uint8_t* out, size_t cap);
/* The unoptimized histogram (histograms.rs) the device took of latent variable `var` (0 = delta, 1 = primary, 2 = secondary) of chunk `task`
 * in the calling thread's last encode pass (after a SYNCHRONOUS encode call on the current device; a call beyond the workspace budget runs in
 * several passes, and `task` counts within the last).  Waits for the device, then writes the first min(n_hist, cap) bins in order -- lower[k],
 * upper[k] (latents) and count[k] -- and info[0..3] = the variable's number of latents, its n_bins_log, EncVar::hist_path (0 = counted in
 * value space with compact 16-bit latents, 1 = rank queries at full width, 2 = what enc_hist_select_kernel handed to enc_hist_sort_kernel) and
 * the chunk's status.  The bins are what the histogram kernels left in the chunk's plan region: nothing behind them writes there (under
 * PCO_GFX_CFG_STRICT_HISTOGRAM they are the literal replay's).  Returns n_hist (0: no encode pass yet on this thread, the workspace was
 * released since, `task` is beyond that pass, or the chunk has no such variable), or -PcoGfxStatus.  Reads only. */
int64_t pco_gfx_debug_histogram(uint32_t task, uint32_t var, uint64_t* lower, uint64_t* upper, uint32_t* count, size_t cap, uint32_t* info /* [4] */);
/* Which pack kernel wrote each page of the calling thread's last encode pass (after a SYNCHRONOUS encode call on the current device; a call
 * beyond the workspace budget runs in several passes).  Waits for the device, then writes out[k] for the first `cap` pages in the pass's
 * page order: 0xff = the page was not fast (enc_page_kernel wrote it), 0xfe = the page did not fit its destination, else the nibble
 * enc_scan_kernel left for the pack kernels: 0 = the general kernel (enc_pack_kernel: three variables, full-width latents of the 8- / 16-bit
 * types, the shifted copy), mask | wide << 3 = a lean kernel (enc_pack1_kernel<mask, wide>: mask 2 primary, 6 primary + secondary, 3 lookback
 * variable + primary), 15 = packed under the walk (enc_walkp_kernel, moved into place by enc_place_kernel).  Which of them packs a page
 * changes no byte.  Returns the number of pages of that pass (0: no encode pass yet on this thread, or the workspace was released since),
 * or -PcoGfxStatus.  Reads only. */
int64_t pco_gfx_debug_pack_routes(uint8_t* out, size_t cap);
/* What ModeSpec::Auto detection saw and decided for each of the first PCO_GFX_AUTO_DEBUG_MAX chunks of the calling thread's last encode
 * call (any entry point; the last pass of a call that the workspace budget split; a call with an explicit mode leaves no records).  The records are copies of what the host step between the
 * detection kernels already held: the hook launches nothing, copies nothing from the device and waits for nothing.
 *   route      0 none (a sample, or for floats its normal not-too-large part, below 10 numbers), 1 decided from the integer kernels,
 *              2 decided from the float kernels, 3 host path by size or type (a sample above 6656 numbers, f16), 4 host path because the
 *              triple-GCD list overflowed (more than 192 values seen twice, or 2048 distinct values).  Routes 3 and 4 fill nothing else
 *              but n_entries / overflow.
 *   stage 1    n_entries / overflow of the GCD list; floats: s_size (kept numbers), tz5, n_ints, n_gcd, sim[3], has_euclid, k, base_c.
 *   candidates slot 0 = float mult by trailing zeros, 1 = float mult by Euclid, 2 = float quant, 3 = int mult.  Bit q of cand_mask: slot
 *              q went to stage 2.  base / inv: the float-mult base and inverse (bits), the int-mult base (slot 3); bk: the float-quant k;
 *              s_int / s_dbl: stage 2's sums (s_dbl as f64 bits).
 * Writes the first min(count, cap) records and returns the count (0: no Auto call yet on this thread).  Reads only. */
#define PCO_GFX_AUTO_DEBUG_MAX 256
typedef struct PcoGfxAutoModeRecord {
  uint32_t route, n_entries, overflow, s_size;
  uint32_t tz5, n_ints, n_gcd, has_euclid;
  uint32_t sim[3];
  int32_t k;
  uint32_t cand_mask, bk;
  uint64_t base_c;
  uint64_t base[4], inv[4];
  int64_t s_int[4];
  uint64_t s_dbl[4];
} PcoGfxAutoModeRecord;
int64_t pco_gfx_debug_auto_mode(PcoGfxAutoModeRecord* out, size_t cap);
/* What DeltaSpec::Auto resolution measured and decided for each of the first PCO_GFX_AUTO_DEBUG_MAX chunks of the calling thread's last encode
 * call (any entry point; the last pass of a call that the workspace budget split; a call with an explicit delta spec leaves no records).  The
 * records are copies of what the host replay of choose_auto_delta_encoding already held: the hook launches nothing, copies nothing from the
 * device and waits for nothing, and keeping the copies runs no trial that the decision did not run.
 *   sample_n     the latents of the chunk's delta sample (0: a chunk below 10 numbers, nothing else is filled)
 *   eval_mask    bit c: candidate c was trial-encoded for this chunk; c = 0 no delta, 1 lookback, 1 + k consecutive order k (k = 1..7)
 *   cost[c]      the size estimate of candidate c's trial in bytes (meta_size_hint + page_size_hint of the sample, the reference's f32); the
 *                lookback's WITHOUT its penalty of sample_n / 4.  0 where eval_mask has no bit.
 *   delta_kind   the plan's final choice: 0 none, 1 consecutive, 2 lookback; delta_order (consecutive) and window_n_log (lookback) with it
 * Writes the first min(count, cap) records and returns the count (0: no Auto-delta call yet on this thread).  Reads only. */
typedef struct PcoGfxAutoDeltaRecord {
  uint32_t sample_n, eval_mask;
  float cost[9];
  uint32_t delta_kind, delta_order, window_n_log;
} PcoGfxAutoDeltaRecord;
int64_t pco_gfx_debug_auto_delta(PcoGfxAutoDeltaRecord* out, size_t cap);

#if defined(__cplusplus)
}
#endif
#endif /* PCO_GFX_H */
