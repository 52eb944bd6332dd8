// decode_resume.hip -- the kernels of pco_gfx_decompress_page_reads (include/pco_gfx.h section 4f): rows [first, first + count) of a wrapped page,
// starting from a cursor an earlier read left instead of from the page's first batch, and leaving a cursor for the next read.
//
// What has to survive between two reads of a page the two-kernel route takes is what dec_walk_body holds between two batches -- row, bit
// position, four tANS states per latent variable -- and the delta moments dec_expand_body carries in LDS.  The kernels are the range ones
// compiled with kResume = true (decode_fast.hip): new instantiations under new names, the ones the other entry points launch are what they were.
//   route 1: dec_walk_resume_kernel<L, 8>, <L, 4>   parse the ChunkMeta and the page header and build the tables as every walker does, judge the `from`
//                                                   cursor (pco_cursor.h), walk batches [at / 256, ceil((first + count) / 256)) and leave where
//                                                   they ended in the task's ReadRec;
//            dec_expand_resume_kernel<L>            starts with the cursor's moments at the cursor's batch under a delta, at first / 256 without
//                                                   one, and writes the `to` cursor of a task that ends PCO_GFX_OK.
//   route 2 (lookback, Conv1, Dict, tables the walkers hand back): the prefix and copy kernels of decode_range.hip from row 0, as a range task;
//            reads_finish_kernel                    writes their position-only `to` cursors.
#pragma once
#include "decode_range.hip"

namespace pcogfx {

template <class L, uint32_t kWQ>
__global__ __launch_bounds__(256) void dec_walk_resume_kernel(const PcoGfxDecodeTask* tasks, const uint32_t* task_ids, uint32_t n_ids, DecPlan* plans,
                                                             uint8_t* bins_area, uint8_t* sym_area, uint64_t sym_stride, uint64_t* offpos_area, uint64_t offpos_stride,
                                                             uint32_t accept_status, PcoGfxTaskResult* results, const MetaRef* metas, const RangeRef* ranges,
                                                             ResumeArgs rz) {
  dec_walk_body<L, kWQ, false, true, true>(tasks, task_ids, n_ids, plans, bins_area, sym_area, sym_stride, offpos_area, offpos_stride, accept_status, results, nullptr, metas, ranges, rz);
}

template <class L>
__global__ __launch_bounds__(256) void dec_expand_resume_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids, uint32_t n_ids,
                                                                const DecPlan* plans, const uint8_t* bins_area, const uint8_t* sym_area, uint64_t sym_stride,
                                                                const uint64_t* offpos_area, uint64_t offpos_stride, const RangeRef* ranges, ResumeArgs rz) {
  dec_expand_body<L, false, true, true>(tasks, results, task_ids, n_ids, plans, bins_area, sym_area, sym_stride, offpos_area, offpos_stride, nullptr, nullptr, ranges, rz);
}

// The synchronous form sizes its symbol scratch by the batches the tasks WALK: the rows their `from` cursors stand at, for the host (0 without one).
// Only a size is derived from them; the walker judges the cursor itself and refuses a task that would walk more than the scratch holds.
__global__ void reads_rows_kernel(const ReadRef* refs, uint32_t n_tasks, uint64_t* rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_tasks) rows[i] = refs[i].from != nullptr ? refs[i].from[1] : 0ull;
}

// After the scratch route: the position-only `to` cursor of a task of route 2 that ended PCO_GFX_OK.  A task that came there because its walk
// failed in the page's body (route 3) keeps the scratch route's error; should that route decode what the walk could not, the cursor the walk
// started from did not describe this page, and the task is PCO_GFX_INSUFFICIENT_DATA.
__global__ void reads_finish_kernel(const PcoGfxDecodeTask* tasks, const RangeRef* ranges, const ReadRef* refs, const ReadRec* recs, PcoGfxTaskResult* results, uint32_t n_tasks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tasks || ranges[i].count == 0) return;
  const uint32_t route = recs[i].route;
  if (route != 2 && route != 3) return;
  if (results[i].status != PCO_GFX_OK) return;
  if (route == 3) { PcoGfxTaskResult r; r.n_out = 0; r.consumed = 0; r.status = PCO_GFX_INSUFFICIENT_DATA; r.aux = 0; results[i] = r; return; }
  uint64_t* to = refs[i].to;
  if (to == nullptr) return;
  const uint64_t page_n = tasks[i].dst_cap, end = range_end_batch(ranges[i].first, ranges[i].count) * kBatchN;
  for (uint32_t k = 0; k < kCursorWords; k++) to[k] = cursor_word(k, kCursorPosition, end < page_n ? end : page_n, 0, page_n, tasks[i].dtype, nullptr, nullptr);
}

}  // namespace pcogfx
