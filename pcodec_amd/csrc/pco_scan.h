// pco_scan.h -- the framing arithmetic of pco_gfx_scan_chunks (include/pco_gfx.h section 4m): a standalone file's header, a chunk's preamble and
// what stands behind a chunk, byte by byte (standalone/decompressor.rs:85-137, 190-231).  Plain C++ without a device header, like pco_dir.h, so that
// the scan kernel (scan.hip) and a CPU test (tests/test_scan_abi.py compiles it with g++) run the same lines.  The verdicts are the ones the decode
// kernels' own parser reaches on the same bytes, in its order; the table is in the header.
#pragma once
#include <stdint.h>

#include "pco_dir.h"

namespace pcogfx {

constexpr uint32_t kScanOk = 0, kScanCorruption = 1, kScanInsufficientData = 2;   // enum PcoGfxStatus: PCO_GFX_OK, _CORRUPTION, _INSUFFICIENT_DATA

// a number type's width in bits: include/pco_gfx.h's type bytes (1 u32, 2 u64, 3 i32, 4 i64, 5 f32, 6 f64, 7 u16, 8 i16, 9 f16, 10 u8, 11 i8); 0: no type
PCO_DIR_HD inline uint32_t scan_type_bits(uint32_t dtype) {
  return dtype == 0 || dtype > 11 ? 0u : (dtype >= 10 ? 8u : (dtype >= 7 ? 16u : ((dtype & 1u) ? 32u : 64u)));
}

// byte i of p[0 .. len), 0 beyond it (the bit reader's padding)
struct ScanBytes {
  const uint8_t* p; uint64_t len;
  PCO_DIR_HD uint32_t at(uint64_t i) const { return i < len ? (uint32_t)p[i] : 0u; }
};

// The file header.  len: the bytes in front of the first chunk (status kScanOk only); format_major: the wrapped format's major version;
// uniform_type: the type byte every chunk must carry, 0 = none named.
struct ScanHeader { uint32_t status, format_major, uniform_type; uint64_t len; };
template <class Bytes>
PCO_DIR_HD inline ScanHeader scan_file_header(const Bytes& b) {
  ScanHeader h{kScanOk, 4, 0, 0};
  if (b.len < 4) { h.status = kScanInsufficientData; return h; }
  if (b.at(0) != 'p' || b.at(1) != 'c' || b.at(2) != 'o' || b.at(3) != '!') { h.status = kScanCorruption; return h; }
  uint64_t pos = 4;
  const uint32_t sv = b.at(4);   // the standalone version; below 2 the byte is the wrapped header's already
  if (sv >= 2) {
    pos = 5;
    if (sv >= 3) {
      const uint32_t ub = b.at(pos++);
      if (ub != 0) { if (scan_type_bits(ub) == 0) { h.status = kScanCorruption; return h; } h.uniform_type = ub; }
    }
    // n_hint: a varint of 6 bits of power, then power + 1 bits, padded with zeros to the byte
    const uint32_t vbits = 6 + 1 + (b.at(pos) & 63u), vbytes = (vbits + 7) / 8;
    const bool pad_ok = (vbits & 7) == 0 || (b.at(pos + vbytes - 1) >> (vbits & 7)) == 0;
    pos += vbytes;
    if (!pad_ok && pos <= b.len) { h.status = kScanCorruption; return h; }
    if (pos > b.len) { h.status = kScanInsufficientData; return h; }
    if (sv > 3) { h.status = kScanCorruption; return h; }
  }
  h.format_major = b.at(pos++);
  if (h.format_major >= 4) pos++;   // the minor version
  if (h.format_major > 4) h.status = kScanCorruption;
  else if (pos > b.len) h.status = kScanInsufficientData;
  h.len = pos;
  return h;
}

// What stands at `pos`, where a chunk's preamble would: kind 0 = a chunk of n numbers (its ChunkMeta at pos + 4), 1 = the terminator, 2 = the stream's
// end (end_ok: a stream without file header may simply end).  uniform_type: the header's, for a file's first chunk; else 0.
struct ScanPreamble { uint32_t status, kind, n; };
constexpr uint32_t kScanChunk = 0, kScanTerminator = 1, kScanEnd = 2;
template <class Bytes>
PCO_DIR_HD inline ScanPreamble scan_chunk_preamble(const Bytes& b, uint64_t pos, uint32_t dtype, uint32_t uniform_type, bool end_ok) {
  ScanPreamble r{kScanOk, kScanChunk, 0};
  if (end_ok && pos >= b.len) { r.kind = kScanEnd; return r; }
  if (pos + 1 > b.len) { r.status = kScanInsufficientData; return r; }
  const uint32_t tb = b.at(pos);
  if (tb == 0) { r.kind = kScanTerminator; return r; }
  if ((uniform_type != 0 && uniform_type != tb) || tb != dtype) { r.status = kScanCorruption; return r; }
  r.n = 1 + (b.at(pos + 1) | (b.at(pos + 2) << 8) | (b.at(pos + 3) << 16));
  if (pos + 4 > b.len) r.status = kScanInsufficientData;
  return r;
}

// Behind a chunk that ended at `pos`: aux bit 0 = another chunk follows, bit 1 = the terminator is there (the caller consumes its byte).  A file's
// first chunk (in_file: the step that read the header) must be followed by one of the two.
struct ScanBehind { uint32_t status, aux; };
template <class Bytes>
PCO_DIR_HD inline ScanBehind scan_behind_chunk(const Bytes& b, uint64_t pos, bool in_file) {
  if (pos < b.len) return ScanBehind{kScanOk, b.at(pos) != 0 ? 1u : 2u};
  return ScanBehind{in_file ? kScanInsufficientData : kScanOk, 0u};
}

}  // namespace pcogfx
