// pco_cursor.h -- the layout of PcoGfxPageCursor (include/pco_gfx.h section 4f) and the verdict on a cursor a task reads from: the one
// function that decides whether the walker may start from what a cursor in device memory says.  Plain C++ without a device header, after
// pco_dir.h's pattern, so that the resume kernels (decode_resume.hip) and a CPU test (tests/test_page_reads_abi.py compiles it with g++) run
// the same lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCO_CUR_HD __host__ __device__
#else
#define PCO_CUR_HD
#endif

namespace pcogfx {

// word 0      version (bits 0..31) | kind (bits 32..63)
// word 1      row: the cursor stands in front of this row of the page
// word 2      bit position in the page of the row's batch (0 in a position-only cursor)
// word 3      page_n (bits 0..31) | dtype (bits 32..63)
// words 4..9  states[3][4]: the tANS state INDEX of chain j of latent variable v in bits 32 (j & 1) .. of word 4 + 2 v + j / 2
// words 10..25 moments[2][8]: the consecutive-delta moments of the primary and the secondary variable, zero beyond the order
// words 26..31 zero
constexpr uint32_t kCursorVersion = 1;
constexpr uint32_t kCursorFull = 1, kCursorPosition = 2;   // every field / version, kind, row, page_n and dtype only (the rest is zero)
constexpr uint32_t kCursorWords = 32, kCursorStateWord = 4, kCursorMomentWord = 10;
constexpr uint32_t kCurOk = 0, kCurInvalidArgument = 3;   // enum PcoGfxStatus: PCO_GFX_OK, PCO_GFX_INVALID_ARGUMENT

PCO_CUR_HD inline uint32_t cursor_state(const uint64_t* w, uint32_t v, uint32_t j) { return (uint32_t)(w[kCursorStateWord + 2 * v + (j >> 1)] >> (32 * (j & 1))); }

// Word i of the cursor in front of `row`.  states / moments: nullptr in a position-only cursor.
PCO_CUR_HD inline uint64_t cursor_word(uint32_t i, uint32_t kind, uint64_t row, uint64_t bit, uint64_t page_n, uint32_t dtype, const uint32_t* states /* [12] */,
                                       const uint64_t* moments /* [16] */) {
  if (i == 0) return (uint64_t)kCursorVersion | ((uint64_t)kind << 32);
  if (i == 1) return row;
  if (i == 2) return kind == kCursorFull ? bit : 0;
  if (i == 3) return (page_n & 0xffffffffu) | ((uint64_t)dtype << 32);
  if (kind != kCursorFull) return 0;
  if (i < kCursorMomentWord) return (uint64_t)states[2 * (i - kCursorStateWord)] | ((uint64_t)states[2 * (i - kCursorStateWord) + 1] << 32);
  if (i < kCursorMomentWord + 16) return moments[i - kCursorMomentWord];
  return 0;
}

// w: the cursor's words 0 .. 9 (a COPY: what is judged here is what is used).  want_kind: kCursorFull for a page the two-kernel route takes,
// kCursorPosition for the others.  page_n, dtype, first: the task's.  body_first_bit: the first bit behind the page's header (the states and
// moments the page itself stores); page_bits: page_len * 8.  asl[v]: ans_size_log of latent variable v, 0 for a variable the page does not have.
// The checks bound everything the walker forms from a cursor: its start batch (row <= first <= page_n), its window position (inside the
// page) and its table addresses (an index inside each variable's table).  position-only cursors carry a row and nothing else.
PCO_CUR_HD inline uint32_t cursor_verdict(const uint64_t* w, uint32_t want_kind, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit,
                                          uint64_t page_bits, const uint32_t* asl /* [3] */) {
  if ((uint32_t)w[0] != kCursorVersion || (uint32_t)(w[0] >> 32) != want_kind) return kCurInvalidArgument;
  if (w[3] != ((page_n & 0xffffffffu) | ((uint64_t)dtype << 32))) return kCurInvalidArgument;
  const uint64_t at = w[1];
  if (at > first) return kCurInvalidArgument;
  if ((at & 255u) != 0 && at != page_n) return kCurInvalidArgument;
  if (want_kind != kCursorFull) return kCurOk;
  if (w[2] < body_first_bit || w[2] > page_bits) return kCurInvalidArgument;
  for (uint32_t v = 0; v < 3; v++)
    for (uint32_t j = 0; j < 4; j++)
      if (cursor_state(w, v, j) >= (1u << asl[v])) return kCurInvalidArgument;
  return kCurOk;
}

// ---- kind 3: the full state of a page the GENERAL kernel decodes (PCO_GFX_CURSOR_GENERAL; decode_general.hip) ----
// words 0..9 as kind 1.  words 10..25: under no delta or a consecutive one moments[2][8] as kind 1; under Conv1 the `order` residuals in front of
// the row as u32, residual i in bits 32 (i % 2) .. of word 10 + i / 2, zero beyond the order.  words 26..31 zero.
constexpr uint32_t kCursorGeneral = 3;
constexpr uint32_t kCursorConv1Max = 32;   // residuals a cursor has room for: the format's largest Conv1 order

PCO_CUR_HD inline uint64_t cursor_conv1_word(uint32_t even, uint32_t odd) { return (uint64_t)even | ((uint64_t)odd << 32); }
PCO_CUR_HD inline uint32_t cursor_conv1_residual(const uint64_t* w, uint32_t i) { return (uint32_t)(w[kCursorMomentWord + (i >> 1)] >> (32 * (i & 1))); }
// residuals[order] -> the cursor's words 10 .. 25
PCO_CUR_HD inline void cursor_conv1_pack(const uint32_t* residuals, uint32_t order, uint64_t* tail /* [16] */) {
  for (uint32_t k = 0; k < 16; k++)
    tail[k] = cursor_conv1_word(2 * k < order ? residuals[2 * k] : 0u, 2 * k + 1 < order ? residuals[2 * k + 1] : 0u);
}

// Word i of the kind-3 cursor in front of `row`.  state_pair: the word's two state indices (i in 4 .. 9), tail: the word's moment or its two
// Conv1 residuals (i in 10 .. 25); each is read for its own words only.
PCO_CUR_HD inline uint64_t cursor_word_general(uint32_t i, uint64_t row, uint64_t bit, uint64_t page_n, uint32_t dtype, uint64_t state_pair, uint64_t tail) {
  if (i == 0) return (uint64_t)kCursorVersion | ((uint64_t)kCursorGeneral << 32);
  if (i == 1) return row;
  if (i == 2) return bit;
  if (i == 3) return (page_n & 0xffffffffu) | ((uint64_t)dtype << 32);
  if (i < kCursorMomentWord) return state_pair;
  if (i < kCursorMomentWord + 16) return tail;
  return 0;
}

// The verdict on a kind-3 cursor.  w: a COPY of the cursor's words 0 .. 9; the other arguments as cursor_verdict's, and end_batch =
// ceil((first + count) / 256), walk_cap = the batches of prefix scratch the host gave the task.  What is bounded is every address the general
// kernel forms from a cursor: its start batch and the scratch it fills from there (at <= first, the batches to walk within walk_cap), its window
// position (the bit position inside the page) and its table entries (a state index inside each variable's table; 0 for an absent variable).
// Words 10 .. 25 are not judged: moments and Conv1 residuals are summands of the numbers and (in Dict mode) of an index that is compared with the
// dictionary's length before it is used -- no address is formed from them.
PCO_CUR_HD inline uint32_t cursor_verdict_general(const uint64_t* w, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits,
                                                  const uint32_t* asl /* [3] */, uint64_t end_batch, uint64_t walk_cap) {
  if ((uint32_t)w[0] != kCursorVersion || (uint32_t)(w[0] >> 32) != kCursorGeneral) return kCurInvalidArgument;
  if (w[3] != ((page_n & 0xffffffffu) | ((uint64_t)dtype << 32))) return kCurInvalidArgument;
  const uint64_t at = w[1];
  if (at > first) return kCurInvalidArgument;
  if ((at & 255u) != 0 && at != page_n) return kCurInvalidArgument;
  if (w[2] < body_first_bit || w[2] > page_bits) return kCurInvalidArgument;
  for (uint32_t v = 0; v < 3; v++)
    for (uint32_t j = 0; j < 4; j++)
      if (cursor_state(w, v, j) >= (1u << asl[v])) return kCurInvalidArgument;
  if (end_batch < (at >> 8) || end_batch - (at >> 8) > walk_cap) return kCurInvalidArgument;
  return kCurOk;
}

// ---- kind 4: the state of a LOOKBACK page that is read beside a history ring (pco_gfx_decompress_page_reads_hist; pco_history.h) ----
// words 0..9 as kind 1: the states of the delta variable (v = 0), the primary and the secondary.  words 10..31 zero: what Lookback carries besides
// them is its window, and that lives in the caller's history buffer.
constexpr uint32_t kCursorLookback = 4;

// Word i of the kind-4 cursor in front of `row`.  state_pair: the word's two state indices (i in 4 .. 9).
PCO_CUR_HD inline uint64_t cursor_word_lookback(uint32_t i, uint64_t row, uint64_t bit, uint64_t page_n, uint32_t dtype, uint64_t state_pair) {
  if (i == 0) return (uint64_t)kCursorVersion | ((uint64_t)kCursorLookback << 32);
  if (i == 1) return row;
  if (i == 2) return bit;
  if (i == 3) return (page_n & 0xffffffffu) | ((uint64_t)dtype << 32);
  if (i < kCursorMomentWord) return state_pair;
  return 0;
}

// The verdict on a kind-4 cursor: kind 3's list, on a COPY of the words 0 .. 9.  It bounds the start batch and the scratch filled from there, the
// window position and the table entries; the ring slots a walk forms from `at` are masked into a length that history_verdict (pco_history.h) checks.
PCO_CUR_HD inline uint32_t cursor_verdict_lookback(const uint64_t* w, uint64_t page_n, uint32_t dtype, uint64_t first, uint64_t body_first_bit, uint64_t page_bits,
                                                   const uint32_t* asl /* [3] */, uint64_t end_batch, uint64_t walk_cap) {
  if ((uint32_t)w[0] != kCursorVersion || (uint32_t)(w[0] >> 32) != kCursorLookback) return kCurInvalidArgument;
  if (w[3] != ((page_n & 0xffffffffu) | ((uint64_t)dtype << 32))) return kCurInvalidArgument;
  const uint64_t at = w[1];
  if (at > first) return kCurInvalidArgument;
  if ((at & 255u) != 0 && at != page_n) return kCurInvalidArgument;
  if (w[2] < body_first_bit || w[2] > page_bits) return kCurInvalidArgument;
  for (uint32_t v = 0; v < 3; v++)
    for (uint32_t j = 0; j < 4; j++)
      if (cursor_state(w, v, j) >= (1u << asl[v])) return kCurInvalidArgument;
  if (end_batch < (at >> 8) || end_batch - (at >> 8) > walk_cap) return kCurInvalidArgument;
  return kCurOk;
}

}  // namespace pcogfx
