// pco_index.h -- the arithmetic of pco_gfx_index_pages (include/pco_gfx.h section 4g): how many cursors an index of a page has, and which of them a
// walk that has just finished a batch stands at.  Plain C++ without a device header, after pco_dir.h's and pco_cursor.h's pattern, so that the
// index kernels (decode_index.hip, through decode_fast.hip), the host checks and a CPU test (tests/test_page_index_abi.py compiles it with g++)
// run the same lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCO_IDX_HD __host__ __device__
#else
#define PCO_IDX_HD
#endif

namespace pcogfx {

constexpr uint64_t kIndexMaxPageN = 1ull << 24;   // a page holds 1 ..= 2^24 numbers
constexpr uint32_t kIndexNoSlot = 0xffffffffu;

// k: cursor i (0 <= i < k) stands in front of row (i + 1) * every_rows, and every one of them has rows behind it: k * every_rows < page_n.
// 0 for what the entry point refuses: page_n == 0 or > 2^24, every_rows == 0 or not a multiple of 256.
PCO_IDX_HD inline uint64_t index_len(uint64_t page_n, uint64_t every_rows) {
  if (page_n == 0 || page_n > kIndexMaxPageN || every_rows == 0 || (every_rows & 255u) != 0) return 0;
  return (page_n - 1) / every_rows;
}

// The cursor a walk stands at when `batches_done` batches of the page are behind it, or kIndexNoSlot: slot i at (i + 1) * every_batches batches,
// for i < k only.  A walk over batches [0, k * every_batches) meets the slots 0 .. k - 1, each once, in order.
PCO_IDX_HD inline uint32_t index_slot(uint32_t batches_done, uint32_t every_batches, uint32_t k) {
  if (every_batches == 0 || batches_done == 0 || batches_done % every_batches != 0) return kIndexNoSlot;
  const uint32_t slot = batches_done / every_batches - 1;
  return slot < k ? slot : kIndexNoSlot;
}

}  // namespace pcogfx
