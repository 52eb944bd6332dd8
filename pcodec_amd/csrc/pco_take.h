// pco_take.h -- the arithmetic of pco_gfx_take_rows (include/pco_gfx.h section 4n): which segment of an indexed page a row id falls into, the read
// task {first, count} of a segment from the largest row wanted in it, and the batches that task walks.  Plain C++ without a device header, after
// pco_index.h's pattern, so that the take kernels (take.hip), the host entry point and a CPU test (tests/test_take_rows_abi.py compiles it with g++)
// run the same lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCO_TAKE_HD __host__ __device__
#else
#define PCO_TAKE_HD
#endif

namespace pcogfx {

constexpr uint32_t kTakeNotMine = 0xffffffffu;   // take_local_row: the id is not a row of this page

// segments of a page of page_n rows cut every every_rows rows (0: no index, one segment): pco_gfx_page_index_len + 1
PCO_TAKE_HD inline uint32_t take_segments(uint64_t page_n, uint64_t every_rows) {
  if (page_n == 0 || every_rows == 0) return 1;
  return (uint32_t)((page_n - 1) / every_rows) + 1;
}

// the page's row an id names, or kTakeNotMine: row_base <= id < row_base + page_n (page_n <= 2^24, and row_base + page_n does not wrap)
PCO_TAKE_HD inline uint32_t take_local_row(uint64_t id, uint64_t row_base, uint64_t page_n) {
  if (id < row_base || id - row_base >= page_n) return kTakeNotMine;
  return (uint32_t)(id - row_base);
}

// the segment of a local row: segment s holds rows [s * every_rows, (s + 1) * every_rows)
PCO_TAKE_HD inline uint32_t take_segment_of(uint32_t local_row, uint64_t every_rows) { return every_rows == 0 ? 0u : (uint32_t)(local_row / every_rows); }

// what a segment's mark holds for a wanted local row: row + 1, so that 0 is "unmarked" and the largest mark names the largest wanted row
PCO_TAKE_HD inline uint32_t take_mark_of(uint32_t local_row) { return local_row + 1; }

// segment s's read task from its mark: {first = s * every_rows, count = largest wanted row + 1 - first}, count 0 when unmarked
PCO_TAKE_HD inline uint64_t take_first(uint32_t s, uint64_t every_rows) { return (uint64_t)s * every_rows; }
PCO_TAKE_HD inline uint64_t take_count(uint32_t s, uint64_t every_rows, uint32_t mark) { return mark == 0 ? 0 : (uint64_t)mark - take_first(s, every_rows); }

// the batches that task walks: from the segment's start (a multiple of 256) to batch ceil((largest wanted row + 1) / 256)
PCO_TAKE_HD inline uint64_t take_batches(uint64_t count) { return (count + 255) / 256; }

// the whole segment, the range the host sizes everything by: rows [s * every_rows, min((s + 1) * every_rows, page_n))
PCO_TAKE_HD inline uint64_t take_segment_rows(uint32_t s, uint64_t page_n, uint64_t every_rows) {
  if (every_rows == 0) return page_n;
  const uint64_t first = take_first(s, every_rows);
  return page_n - first < every_rows ? page_n - first : every_rows;
}

}  // namespace pcogfx
