// pco_dir.h -- the verdict on one task of pco_gfx_decompress_pages_dir / pco_gfx_decompress_page_ranges_dir (include/pco_gfx.h section 4e):
// where a task's ChunkMeta and page lie in a compacted stream, or why the task is refused.  Plain C++ without a device header, so that the
// resolve kernel (dir_resolve.hip) and a CPU test (tests/test_page_directory_abi.py compiles it with g++) run the same lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCO_DIR_HD __host__ __device__
#else
#define PCO_DIR_HD
#endif

namespace pcogfx {

constexpr uint32_t kDirOk = 0, kDirInsufficientData = 2, kDirInvalidArgument = 3;   // enum PcoGfxStatus: PCO_GFX_OK, _INSUFFICIENT_DATA, _INVALID_ARGUMENT

struct DirVerdict { const uint8_t* meta; uint64_t meta_len; const uint8_t* page; uint64_t page_len; uint32_t status; };

// blob, blob_len, gap: PcoGfxDirectory's.  end: d_offsets[n_pieces].  m0, m1 / p0, p1: d_offsets[k], d_offsets[k + 1] of the task's ChunkMeta
// piece / page piece.  The checks in the order of the header's table; a refused task points at the blob's first byte with lengths of 0, so
// that nothing of the blob is read for it (never nullptr: MetaRef.p == nullptr means "the ChunkMeta is in front of the page").
PCO_DIR_HD inline DirVerdict dir_verdict(const uint8_t* blob, uint64_t blob_len, uint32_t gap, uint64_t end, uint64_t m0, uint64_t m1, uint64_t p0, uint64_t p1) {
  DirVerdict v{blob, 0, blob, 0, kDirOk};
  if (end == ~(uint64_t)0) { v.status = kDirInvalidArgument; return v; }                               // the compactor's "destination too small": nothing was copied
  if (m0 > m1 || m1 > blob_len || p0 > p1 || p1 > blob_len) { v.status = kDirInvalidArgument; return v; }
  if (m1 == m0) { v.status = kDirInsufficientData; return v; }                                         // the chunk was dropped (a kept ChunkMeta is >= 1 byte); NOT asked of the page: a kept page may be 0 bytes
  if (m1 - m0 < gap || p1 - p0 < gap) { v.status = kDirInvalidArgument; return v; }
  v.meta = blob + m0 + gap; v.meta_len = m1 - m0 - gap;
  v.page = blob + p0 + gap; v.page_len = p1 - p0 - gap;
  return v;
}

}  // namespace pcogfx
