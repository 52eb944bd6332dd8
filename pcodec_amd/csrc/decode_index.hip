// decode_index.hip -- the kernels of pco_gfx_index_pages (include/pco_gfx.h section 4g): the cursors in front of rows every_rows, 2 every_rows, ...
// of a wrapped page from ONE walk of it, where a chain of pco_gfx_decompress_page_reads calls walks it once per cursor (or, on the scratch route,
// once per cursor from row 0).  No rows are stored and no dst exists.
//
// The kernels are the range ones compiled with kIndex = true (decode_fast.hip): new instantiations under new names, the ones the other entry
// points launch are what they were.  A cursor has two authors:
//   route 1: dec_walk_index_kernel<L, 8>, <L, 4>   a range walk over batches [0, k every_rows / 256); behind every batch whose end row is a multiple
//                                                  of every_rows it writes the cursor's words 1, 2 and 4 .. 9 -- row, bit position, state indices,
//                                                  entry address back to index as the resume walker does at its end;
//            dec_expand_index_kernel<L>            the sum-only mode range tasks run in front of their range, over the same batches: under a delta it
//                                                  unpacks and sums and writes words 0, 3 and 10 .. 31 at the same boundaries; without one it skips
//                                                  the batches and writes those words (zero moments) for all k cursors at once.
//   route 2 (lookback, Conv1, Dict, tables the walkers hand back): the prefix kernel of decode_range.hip over the page's first batch, for the
//            verdict a range task {first 0, count 1} gets;
//            index_finish_kernel                   then writes the k position-only cursors and the result of a task that ended PCO_GFX_OK.
// Nothing here has one thread per cursor: k reaches 65535.
#pragma once
#include "decode_range.hip"

namespace pcogfx {

template <class L, uint32_t kWQ>
__global__ __launch_bounds__(256) void dec_walk_index_kernel(const PcoGfxDecodeTask* tasks, const uint32_t* task_ids, uint32_t n_ids, DecPlan* plans,
                                                            uint8_t* bins_area, uint8_t* sym_area, uint64_t sym_stride, uint64_t* offpos_area, uint64_t offpos_stride,
                                                            uint32_t accept_status, PcoGfxTaskResult* results, const MetaRef* metas, const RangeRef* ranges,
                                                            IndexArgs ix) {
  dec_walk_body<L, kWQ, false, true, false, true>(tasks, task_ids, n_ids, plans, bins_area, sym_area, sym_stride, offpos_area, offpos_stride, accept_status, results, nullptr, metas, ranges,
                                                  ResumeArgs{nullptr, nullptr, 0}, ix);
}

template <class L>
__global__ __launch_bounds__(256) void dec_expand_index_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids, uint32_t n_ids,
                                                               const DecPlan* plans, const uint8_t* bins_area, const uint8_t* sym_area, uint64_t sym_stride,
                                                               const uint64_t* offpos_area, uint64_t offpos_stride, const RangeRef* ranges, IndexArgs ix) {
  dec_expand_body<L, false, true, false, true>(tasks, results, task_ids, n_ids, plans, bins_area, sym_area, sym_stride, offpos_area, offpos_stride, nullptr, nullptr, ranges,
                                               ResumeArgs{nullptr, nullptr, 0}, ix);
}

// After the scratch route, one block per task: a page the walkers handed back (its plan still says so) whose first batch decoded PCO_GFX_OK gets
// its k position-only cursors -- the words reads_finish_kernel writes, for rows every_rows, 2 every_rows, ... -- and the result {k, 0, OK, aux 1}.
// Every other status the scratch route left stands, with n_out 0.
__global__ __launch_bounds__(256) void index_finish_kernel(const PcoGfxDecodeTask* tasks, const DecPlan* plans, const IndexRef* refs, PcoGfxTaskResult* results, uint32_t n_tasks) {
  for (uint32_t i = blockIdx.x; i < n_tasks; i += gridDim.x) {
    const IndexRef ir = refs[i];
    if (ir.k == 0 || plans[i].status != kStatusRetryLegacy) continue;   // (uniform over the block)
    const uint32_t status = results[i].status;
    __syncthreads();   // every thread has read the status before thread 0 replaces the result
    if (status != PCO_GFX_OK) {
      if (threadIdx.x == 0) results[i].n_out = 0;
      continue;
    }
    const uint64_t page_n = tasks[i].dst_cap, every_rows = (uint64_t)ir.every_batches * kBatchN;
    const uint32_t dtype = tasks[i].dtype;
    for (uint64_t w = threadIdx.x; w < (uint64_t)ir.k * kCursorWords; w += 256)
      ir.cursors[w] = cursor_word((uint32_t)(w % kCursorWords), kCursorPosition, (w / kCursorWords + 1) * every_rows, 0, page_n, dtype, nullptr, nullptr);
    if (threadIdx.x == 0) { PcoGfxTaskResult r; r.n_out = ir.k; r.consumed = 0; r.status = PCO_GFX_OK; r.aux = 1; results[i] = r; }
  }
}

}  // namespace pcogfx
