// pco_chunk_dir.h -- the verdict on one task of pco_gfx_decompress_chunks_dir / pco_gfx_decompress_chunk_reads_dir / pco_gfx_index_chunks_dir
// (include/pco_gfx.h section 4l): where the ChunkMeta and the one page of a STANDALONE chunk lie in the stream pco_gfx_compact_chunks left, or why
// the task is refused.  A standalone chunk is `dtype byte | 24-bit n - 1 | ChunkMeta | one page of n numbers` (standalone/compressor.rs:191-203), and
// the ChunkMeta's length is closed-form in a handful of its header fields (metadata/chunk_latent_var.rs:170-178, bin.rs:20), so one thread splits a
// chunk with a few dependent loads and every decode kernel behind it sees a wrapped page.  Plain C++ without a device header, like pco_dir.h, so
// that the resolve kernels (dir_resolve.hip), pco_gfx_standalone_chunk_split and a CPU test (tests/test_chunk_directory_abi.py compiles it with
// g++) run the same lines.
#pragma once
#include <stdint.h>

#include "pco_dir.h"

namespace pcogfx {

constexpr uint32_t kDirCorruption = 1;   // enum PcoGfxStatus: PCO_GFX_CORRUPTION (the three others: pco_dir.h)

// the bits of a number type's latent: include/pco_gfx.h's type bytes (1 u32, 2 u64, 3 i32, 4 i64, 5 f32, 6 f64, 7 u16, 8 i16, 9 f16, 10 u8, 11 i8); 0: no type
PCO_DIR_HD inline uint32_t chunk_dir_latent_bits(uint32_t dtype) {
  return dtype == 0 || dtype > 11 ? 0u : (dtype >= 10 ? 8u : (dtype >= 7 ? 16u : ((dtype & 1u) ? 32u : 64u)));
}
PCO_DIR_HD inline uint32_t chunk_dir_offset_bits_bits(uint32_t latent_bits) {   // bits.rs:24-26
  return latent_bits == 8 ? 4u : (latent_bits == 16 ? 5u : (latent_bits == 32 ? 6u : 7u));
}

// a little-endian bit stream over p[0 .. len) (bit_reader.rs): a field of up to 32 bits, byte by byte; a read beyond len gives zeros and sets `past`
struct ChunkDirBits {
  const uint8_t* p; uint64_t len; uint64_t bit; bool past;
  PCO_DIR_HD uint32_t read(uint32_t n) {
    uint64_t v = 0;
    const uint64_t first = bit >> 3, last = (bit + n + 7) >> 3;   // bytes [first, last): five at the most
    for (uint64_t b = first; b < last; b++) {
      if (b >= len) { past = true; break; }
      v |= (uint64_t)p[b] << (8 * (b - first));
    }
    v = (v >> (bit & 7)) & (((uint64_t)1 << n) - 1);
    bit += n;
    return (uint32_t)v;
  }
  PCO_DIR_HD void skip(uint64_t n) { bit += n; if (n != 0 && ((bit + 7) >> 3) > len) past = true; }
};

// The byte length of the ChunkMeta that starts at p (metadata/chunk.rs:127-174): the mode and its payload, the delta encoding and its payload, then
// per latent variable present 4 bits of ans_size_log, 15 bits of n_bins and n_bins * (ans_size_log + L + bits_to_encode_offset_bits) bits of bins,
// padded to a byte.  Header fields only: no bin is read, and the bins may lie beyond len (the caller compares the length with what it has).
// An unknown mode or delta variant is Corruption, a header field beyond len InsufficientData; every other validation stays with the decode kernels.
// Returns *meta_len (0 on failure).
PCO_DIR_HD inline uint64_t chunk_meta_extent(const uint8_t* p, uint64_t len, uint32_t dtype, uint32_t format_major, uint64_t* meta_len, uint32_t* status) {
  *meta_len = 0;
  const uint32_t lb = chunk_dir_latent_bits(dtype);
  if (lb == 0) { *status = kDirInvalidArgument; return 0; }
  ChunkDirBits r{p, len, 0, false};
  const uint32_t mode = r.read(4);
  if (r.past) { *status = kDirInsufficientData; return 0; }
  if (mode > 4) { *status = kDirCorruption; return 0; }
  if (mode == 1 || mode == 2) r.skip(lb);   // IntMult, FloatMult: the base (mode.rs:166-195)
  else if (mode == 3) r.skip(8);            // FloatQuant: k
  else if (mode == 4) {                     // Dict (mode.rs:138-165): 25 bits of length, zeros to the byte, the dictionary's latents
    const uint32_t dict_n = r.read(25);
    if (r.past) { *status = kDirInsufficientData; return 0; }
    r.bit = (r.bit + 7) & ~(uint64_t)7;
    r.skip((uint64_t)dict_n * lb);
  }
  if (r.past) { *status = kDirInsufficientData; return 0; }
  bool lookback = false;
  if (format_major < 3) r.skip(3);   // the order alone (delta_encoding.rs:120-141)
  else {
    const uint32_t variant = r.read(4);
    if (r.past) { *status = kDirInsufficientData; return 0; }
    if (variant > 3) { *status = kDirCorruption; return 0; }
    if (variant == 1) r.skip(3 + 1);                             // Consecutive: order, secondary_uses_delta
    else if (variant == 2) { r.skip(5 + 4 + 1); lookback = true; }   // Lookback: window_n_log - 1, state_n_log, secondary_uses_delta
    else if (variant == 3) {                                     // Conv1: quantization, bias, weight count - 1, the weights
      r.skip(5 + 64);
      const uint32_t n_weights = 1 + r.read(5);
      if (r.past) { *status = kDirInsufficientData; return 0; }
      r.skip((uint64_t)n_weights * 32);
    }
  }
  if (r.past) { *status = kDirInsufficientData; return 0; }
  // the delta variable (u32 latents) under Lookback, the primary (u32 dictionary indices in Dict mode), the secondary of the three two-variable modes
  const bool present[3] = {lookback, true, mode == 1 || mode == 2 || mode == 3};
  for (int v = 0; v < 3; v++) {
    if (!present[v]) continue;
    const uint32_t bits = v == 0 || (v == 1 && mode == 4) ? 32u : lb;
    const uint32_t ans_size_log = r.read(4), n_bins = r.read(15);
    if (r.past) { *status = kDirInsufficientData; return 0; }
    r.bit += (uint64_t)n_bins * (ans_size_log + bits + chunk_dir_offset_bits_bits(bits));   // (the bins themselves: not asked to lie inside len)
  }
  *status = kDirOk;
  *meta_len = (r.bit + 7) >> 3;
  return *meta_len;
}

// One standalone chunk of `avail` bytes at `chunk`: the preamble, then the ChunkMeta's extent.  page_n != 0: the preamble's n must equal it.  *n: the
// preamble's n once it is read.  A refusal points at `blob` with lengths of 0.
PCO_DIR_HD inline DirVerdict chunk_split_verdict(const uint8_t* blob, const uint8_t* chunk, uint64_t avail, uint32_t dtype, uint64_t page_n, uint32_t format_major, uint64_t* n) {
  DirVerdict v{blob, 0, blob, 0, kDirOk};
  if (avail < 4) { v.status = kDirInsufficientData; return v; }
  if (chunk[0] != dtype) { v.status = kDirCorruption; return v; }   // (a terminator's 0 byte included: decode_kernel.hip's preamble check)
  *n = 1 + ((uint64_t)chunk[1] | (uint64_t)chunk[2] << 8 | (uint64_t)chunk[3] << 16);
  if (page_n != 0 && *n != page_n) { v.status = kDirInvalidArgument; return v; }
  uint64_t meta_len = 0;
  chunk_meta_extent(chunk + 4, avail - 4, dtype, format_major, &meta_len, &v.status);
  if (v.status != kDirOk) return v;
  if (meta_len > avail - 4) { v.status = kDirInsufficientData; return v; }
  v.meta = chunk + 4; v.meta_len = meta_len;
  v.page = chunk + 4 + meta_len; v.page_len = avail - 4 - meta_len;   // (0 is legal: a constant chunk)
  return v;
}

// blob, blob_len, gap: PcoGfxDirectory's.  end: d_offsets[n_pieces].  c0, c1: d_offsets[k], d_offsets[k + 1] of the task's chunk.  dtype, page_n,
// format_major: the task's.  The checks in the order of the header's table (section 4l).
PCO_DIR_HD inline DirVerdict chunk_verdict(const uint8_t* blob, uint64_t blob_len, uint32_t gap, uint64_t end, uint64_t c0, uint64_t c1, uint32_t dtype, uint64_t page_n,
                                           uint32_t format_major) {
  DirVerdict v{blob, 0, blob, 0, kDirOk};
  if (end == ~(uint64_t)0) { v.status = kDirInvalidArgument; return v; }   // the compactor's "destination too small": nothing was copied
  if (c0 > c1 || c1 > blob_len) { v.status = kDirInvalidArgument; return v; }
  if (c1 == c0) { v.status = kDirInsufficientData; return v; }             // the compactor dropped the chunk
  if (c1 - c0 < gap) { v.status = kDirInvalidArgument; return v; }
  uint64_t n = 0;
  return chunk_split_verdict(blob, blob + c0 + gap, c1 - c0 - gap, dtype, page_n, format_major, &n);
}

}  // namespace pcogfx
