// pco_history.h -- the layout of a Lookback page's HISTORY buffer (include/pco_gfx.h section 4i): the slot arithmetic of its ring, the rows a read
// writes back into it, and the verdict on a header a task resumes from.  Plain C++ without a device header, after pco_cursor.h's pattern, so
// that the general kernel (decode_kernel.hip, kHist) and a CPU test (tests/test_lookback_history_abi.py compiles it with g++) run the same lines.
//
// F is the primary-latent history of delta/lookback.rs: F[j] = the primary latent of row j (in Classic mode the ordered latent of number j).  The
// decoder's output lags its deltas by state_n = 1 << state_n_log: a walk that has decoded every batch in front of row r has computed F up to
// reach(r) = min(r + state_n, page_n).  A buffer stamped `row = r` holds F[j] for every j in [max(0, reach(r) - window_n), reach(r)).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCO_HIST_HD __host__ __device__
#else
#define PCO_HIST_HD
#endif

namespace pcogfx {

// header, 8 words: version | row | page_n (bits 0..31), dtype (bits 32..63) | window_n_log | 0 0 0 0; then the ring: window_n latents
constexpr uint32_t kHistoryVersion = 1;
constexpr uint32_t kHistoryHeaderBytes = 64, kHistoryHeaderWords = 8;
constexpr uint32_t kHistoryMinWindowLog = 1, kHistoryMaxWindowLog = 24;   // the format's window_n_log (metadata/delta_encoding.rs)
constexpr uint32_t kHistOk = 0, kHistInvalidArgument = 3;   // enum PcoGfxStatus: PCO_GFX_OK, PCO_GFX_INVALID_ARGUMENT

// bytes of a history buffer; 0 for a window_n_log outside the format's or a width that is no number's
PCO_HIST_HD inline uint64_t history_bytes(uint32_t window_n_log, uint32_t width) {
  if (window_n_log < kHistoryMinWindowLog || window_n_log > kHistoryMaxWindowLog) return 0;
  if (width != 1 && width != 2 && width != 4 && width != 8) return 0;
  return (uint64_t)kHistoryHeaderBytes + ((uint64_t)width << window_n_log);
}

// the ring slot of F[j]: always inside the window_n latents that history_verdict found room for
PCO_HIST_HD inline uint64_t history_slot(uint64_t j, uint32_t window_n_log) { return j & (((uint64_t)1 << window_n_log) - 1); }

// how far F is computed once the walk stands in front of `row`
PCO_HIST_HD inline uint64_t history_reach(uint64_t row, uint64_t state_n, uint64_t page_n) { return row + state_n < page_n ? row + state_n : page_n; }

PCO_HIST_HD inline uint64_t history_header_word(uint32_t i, uint64_t row, uint64_t page_n, uint32_t dtype, uint32_t window_n_log) {
  if (i == 0) return kHistoryVersion;
  if (i == 1) return row;
  if (i == 2) return (page_n & 0xffffffffu) | ((uint64_t)dtype << 32);
  if (i == 3) return window_n_log;
  return 0;
}

// The rows [lo, hi) of F a read writes into the ring when it moves the pair from `from_row` to `to_row`: the last min(window_n, rows walked) of the
// rows it computed, so that no slot is written twice and, with what the ring held, the stamp `to_row` is true.  fresh: the read started without a
// cursor (at row 0, the ring holding nothing): the rows walked are all of [0, reach(to_row)), the page header's state included.
struct HistoryRows { uint64_t lo, hi; };
PCO_HIST_HD inline HistoryRows history_update_rows(bool fresh, uint64_t from_row, uint64_t to_row, uint64_t state_n, uint64_t page_n, uint32_t window_n_log) {
  const uint64_t window_n = (uint64_t)1 << window_n_log;
  const uint64_t old_reach = fresh ? 0 : history_reach(from_row, state_n, page_n), new_reach = history_reach(to_row, state_n, page_n);
  const uint64_t walked = new_reach > old_reach ? new_reach - old_reach : 0;
  return HistoryRows{new_reach - (walked < window_n ? walked : window_n), new_reach};
}

// The rows [lo, hi) of F an INDEX walk (pco_gfx_index_pages_hist; include/pco_gfx.h section 4j) copies into the history it stamps `row`: all the stamp
// promises, [max(0, reach - window_n), reach) -- the union of what a chain of reads from row 0 to `row` writes (history_update_rows), each slot once.
// hi - lo <= window_n, so the slots j & (window_n - 1) are at most two contiguous runs.
PCO_HIST_HD inline HistoryRows history_snapshot_rows(uint64_t row, uint64_t state_n, uint64_t page_n, uint32_t window_n_log) {
  const uint64_t window_n = (uint64_t)1 << window_n_log, reach = history_reach(row, state_n, page_n);
  return HistoryRows{reach > window_n ? reach - window_n : 0, reach};
}

// history i of an index task: k buffers `stride` bytes apart
PCO_HIST_HD inline uint8_t* history_at(void* histories, uint64_t stride, uint64_t i) { return (uint8_t*)histories + i * stride; }

// The verdict on a task's history.  hdr: a COPY of the header's words 0 .. 3 (read only when the task resumes); history_len: the task's;
// resumes: the task has a `from` cursor, standing at from_row; page_n, dtype, window_n_log, width: the page's.  A buffer too short for the page's
// window is refused whether the task resumes or starts the page; a resumed one must be stamped for this page and for the cursor's row.
PCO_HIST_HD inline uint32_t history_verdict(const uint64_t* hdr, uint64_t history_len, bool resumes, uint64_t from_row, uint64_t page_n, uint32_t dtype,
                                            uint32_t window_n_log, uint32_t width) {
  const uint64_t need = history_bytes(window_n_log, width);
  if (need == 0 || history_len < need) return kHistInvalidArgument;
  if (!resumes) return kHistOk;
  if (hdr[0] != kHistoryVersion) return kHistInvalidArgument;
  if (hdr[2] != ((page_n & 0xffffffffu) | ((uint64_t)dtype << 32))) return kHistInvalidArgument;
  if (hdr[3] != window_n_log) return kHistInvalidArgument;
  if (hdr[1] != from_row) return kHistInvalidArgument;
  return kHistOk;
}

}  // namespace pcogfx
