// take.hip -- the kernels of pco_gfx_take_rows (include/pco_gfx.h section 4n): rows of indexed pages chosen by row ids that live on the device.
//
// A take task's page is cut at its index's cursors into segments, and every segment is one read task of decode_resume.hip whose {first, count}
// the DEVICE decides from the ids: the host lays the read tasks out for whole segments (the upper bound of every size), and
//   take_mark_kernel     one pass over the id lists: per segment the largest wanted row + 1 (0: unmarked), per take task the ids inside its page;
//   take_plan_kernel     one thread per segment: its read task's RangeRef, {first, count} or {first, 0}, and the task's segments and batches;
//   (the resume route)   decodes the marked segments side by side into the task's row area, as any read call;
//   take_gather_kernel   dst[j] = row area[id - row_base] for the ids inside the page whose segment ended PCO_GFX_OK;
//   take_finish_kernel   folds the segments' results into one result per take task.
// The arithmetic is pco_take.h's.  Every address formed from an id is bounded by the in-page test: local row < page_n, segment < n_seg.
#pragma once
#include "decode_resume.hip"
#include "pco_take.h"

namespace pcogfx {

struct TakeDev {   // one take task as the kernels take it
  const uint64_t* rows; uint64_t n_rows;
  void* dst; const uint8_t* area;          // area: the task's page_n decoded rows in workspace scratch, segment s at row s * every_rows
  uint64_t row_base, page_n, every_rows;
  uint32_t seg0, n_seg;                    // its segments are the call's read tasks [seg0, seg0 + n_seg)
  uint32_t width, pad;
};
struct TakeTally { uint32_t in_page, aux; uint64_t consumed; };   // zeroed by the host: ids inside the page (mark) | segments and batches walked (plan)

constexpr uint32_t kTakeBlock = 256;
constexpr uint32_t kTakePairTile = kTakeBlock;          // the mark kernel: a thread takes two ids, one 16-byte load
constexpr uint32_t kTakeIdTile = 4 * kTakeBlock;        // the gather kernel: ids of one block's turn

// One id of a wave's lanes into the marks.  Every lane of the wave calls it (mine == false: no id).  When the lanes that have one fall into ONE
// segment -- sorted or clustered ids -- the wave reduces its largest mark across the lanes and makes one atomic; else each lane makes its own.
// Returns the lanes that had an id inside the page.
__device__ inline uint32_t take_mark_wave(uint32_t* seg_marks, bool mine, uint32_t seg, uint32_t mark) {
  const uint64_t have = __ballot(mine);
  if (have == 0) return 0;
  const int lead = __ffsll((unsigned long long)have) - 1;
  const uint32_t lead_seg = (uint32_t)__shfl((int)seg, lead, 64);
  if (__ballot(mine && seg == lead_seg) == have) {
    uint32_t m = mine ? mark : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)m, d, 64); m = o > m ? o : m; }
    if ((int)lane_id() == lead) atomicMax(seg_marks + lead_seg, m);
  } else if (mine) {
    atomicMax(seg_marks + seg, mark);
  }
  return (uint32_t)__popcll((unsigned long long)have);
}

// grid (tiles of id pairs, take tasks).  marks: one zeroed u32 per segment of the call; tally: one zeroed TakeTally per take task.
__global__ __launch_bounds__(kTakeBlock) void take_mark_kernel(const TakeDev* takes, uint32_t n_takes, uint32_t* marks, TakeTally* tally) {
  for (uint32_t t = blockIdx.y; t < n_takes; t += gridDim.y) {
    const TakeDev tk = takes[t];
    const uint64_t n = tk.n_rows;
    if (n == 0) continue;
    // ids are 8-byte aligned; pair p is elements 2p - head and 2p - head + 1, so that every whole pair is one aligned 16-byte load
    const uint64_t head = ((uintptr_t)tk.rows >> 3) & 1u;
    const uint64_t n_pairs = (n + head + 1) >> 1;
    uint32_t* seg_marks = marks + tk.seg0;
    uint32_t counted = 0;
    for (uint64_t p0 = (uint64_t)blockIdx.x * kTakePairTile; p0 < n_pairs; p0 += (uint64_t)gridDim.x * kTakePairTile) {   // (uniform over the block: every lane shuffles)
      const uint64_t p = p0 + threadIdx.x;
      uint64_t id[2] = {0, 0}; bool has[2] = {false, false};
      if (p < n_pairs) {
        const uint64_t e1 = 2 * p + 1 - head;        // the pair's second element; its first is e1 - 1, absent for p == 0 under head
        has[0] = e1 >= 1; has[1] = e1 < n;
        if (has[0] && has[1]) { const ulonglong2 v = *(const ulonglong2*)(tk.rows + e1 - 1); id[0] = v.x; id[1] = v.y; }
        else if (has[0]) id[0] = tk.rows[e1 - 1];
        else if (has[1]) id[1] = tk.rows[e1];
      }
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const uint32_t local = has[k] ? take_local_row(id[k], tk.row_base, tk.page_n) : kTakeNotMine;
        const bool mine = local != kTakeNotMine;
        counted += take_mark_wave(seg_marks, mine, mine ? take_segment_of(local, tk.every_rows) : 0u, mine ? take_mark_of(local) : 0u);
      }
    }
    if ((threadIdx.x & 63u) == 0 && counted) atomicAdd(&tally[t].in_page, counted);
  }
}

// one thread per segment of the call: seg_take[g] is the take task of read task g
__global__ __launch_bounds__(kTakeBlock) void take_plan_kernel(const TakeDev* takes, const uint32_t* seg_take, const uint32_t* marks, uint32_t n_segs, RangeRef* ranges,
                                                              TakeTally* tally) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_segs) return;
  const uint32_t t = seg_take[g];
  const uint64_t every_rows = takes[t].every_rows;
  const uint32_t s = g - takes[t].seg0, mark = marks[g];
  const uint64_t count = take_count(s, every_rows, mark);
  ranges[g] = RangeRef{take_first(s, every_rows), count};
  if (mark == 0) return;
  atomicAdd(&tally[t].aux, 1u);
  atomicAdd((unsigned long long*)&tally[t].consumed, (unsigned long long)take_batches(count));
}

template <class L>
__device__ inline void take_gather_task(const TakeDev& tk, const PcoGfxTaskResult* seg_results) {
  const L* area = (const L*)tk.area;
  L* dst = (L*)tk.dst;
  for (uint64_t j = (uint64_t)blockIdx.x * kTakeBlock + threadIdx.x; j < tk.n_rows; j += (uint64_t)gridDim.x * kTakeBlock) {
    const uint32_t local = take_local_row(tk.rows[j], tk.row_base, tk.page_n);
    if (local == kTakeNotMine) continue;
    if (seg_results[tk.seg0 + take_segment_of(local, tk.every_rows)].status != PCO_GFX_OK) continue;
    dst[j] = area[local];
  }
}

// grid (tiles of ids, take tasks): coalesced loads of the ids and stores of dst, the row area read at the id's local row
__global__ __launch_bounds__(kTakeBlock) void take_gather_kernel(const TakeDev* takes, uint32_t n_takes, const PcoGfxTaskResult* seg_results) {
  for (uint32_t t = blockIdx.y; t < n_takes; t += gridDim.y) {
    const TakeDev tk = takes[t];
    switch (tk.width) {
      case 8: take_gather_task<uint64_t>(tk, seg_results); break;
      case 4: take_gather_task<uint32_t>(tk, seg_results); break;
      case 2: take_gather_task<uint16_t>(tk, seg_results); break;
      default: take_gather_task<uint8_t>(tk, seg_results); break;
    }
  }
}

// One wave per take task: the lowest marked segment that did not end PCO_GFX_OK gives the task's status; else its tallies.  A segment left with the
// walkers' hand-back status had no place on the scratch route (the call gives prefix scratch to segment 0 alone without PCO_GFX_CURSOR_GENERAL): one whose
// walk failed in the page's body is PCO_GFX_INSUFFICIENT_DATA, as the read task reports it; one that stands behind a position-only cursor is
// PCO_GFX_UNSUPPORTED.
__global__ __launch_bounds__(64) void take_finish_kernel(const TakeDev* takes, uint32_t n_takes, const uint32_t* marks, const PcoGfxTaskResult* seg_results, const ReadRec* recs,
                                                         const TakeTally* tally, PcoGfxTaskResult* out) {
  for (uint32_t t = blockIdx.x; t < n_takes; t += gridDim.x) {
    const uint32_t seg0 = takes[t].seg0, n_seg = takes[t].n_seg;
    uint32_t bad = 0xffffffffu;
    for (uint32_t s = threadIdx.x; s < n_seg; s += 64)
      if (marks[seg0 + s] != 0 && seg_results[seg0 + s].status != PCO_GFX_OK) { bad = s; break; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)bad, d, 64); bad = o < bad ? o : bad; }
    if (threadIdx.x != 0) continue;
    PcoGfxTaskResult r; r.n_out = 0; r.consumed = 0; r.status = PCO_GFX_OK; r.aux = 0;
    if (bad != 0xffffffffu) {
      uint32_t st = seg_results[seg0 + bad].status;
      if (st >= kStatusRetryLegacy) st = recs[seg0 + bad].route == 3 ? (uint32_t)PCO_GFX_INSUFFICIENT_DATA : (uint32_t)PCO_GFX_UNSUPPORTED;
      r.status = st;
    } else {
      r.n_out = tally[t].in_page; r.consumed = tally[t].consumed; r.aux = tally[t].aux;
    }
    out[t] = r;
  }
}

}  // namespace pcogfx
