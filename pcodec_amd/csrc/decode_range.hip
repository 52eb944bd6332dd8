// decode_range.hip -- the kernels of pco_gfx_decompress_page_ranges: rows [first, first + count) of a wrapped page without the rest.
//
// A page decodes strictly forwards (tANS states, bit position, delta state), so a range needs the walk up to the batch that holds its last
// row and nothing behind it.  The kernels are the whole-page ones compiled with kRange = true (decode_fast.hip, decode_kernel.hip): new
// instantiations under new names, the ones the other entry points launch are what they were.
//   route 1, pages the two-kernel path takes (no delta or a consecutive delta, tables inside the walkers' LDS slices):
//     dec_walk_range_kernel<L, 8>, <L, 4>   the ordinary walkers, ending with batch ceil((first + count) / 256);
//     dec_expand_range_kernel<L>            starts at batch first / 256 without a delta; with one it sums the batches in front for their
//                                           moments and neither joins nor stores them.  Stores are rebased by `first`.
//   route 2, everything that keeps its history in dst (lookback, Conv1, Dict) or has tables the walkers hand back:
//     pco_decode_prefix_kernel<L>           the single-kernel decoder over batches [0, ceil((first + count) / 256)) into workspace scratch;
//     range_copy_kernel<L>                  the range out of the scratch, and the task's result.
#pragma once
#include "decode_fast.hip"

namespace pcogfx {

template <class L, uint32_t kWQ>
__global__ __launch_bounds__(256) void dec_walk_range_kernel(const PcoGfxDecodeTask* tasks, const uint32_t* task_ids, uint32_t n_ids, DecPlan* plans,
                                                            uint8_t* bins_area, uint8_t* sym_area, uint64_t sym_stride, uint64_t* offpos_area, uint64_t offpos_stride,
                                                            uint32_t accept_status, PcoGfxTaskResult* results, const MetaRef* metas, const RangeRef* ranges) {
  dec_walk_body<L, kWQ, false, true>(tasks, task_ids, n_ids, plans, bins_area, sym_area, sym_stride, offpos_area, offpos_stride, accept_status, results, nullptr, metas, ranges);
}

template <class L>
__global__ __launch_bounds__(256) void dec_expand_range_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids, uint32_t n_ids,
                                                               const DecPlan* plans, const uint8_t* bins_area, const uint8_t* sym_area, uint64_t sym_stride,
                                                               const uint64_t* offpos_area, uint64_t offpos_stride, const RangeRef* ranges) {
  dec_expand_body<L, false, true>(tasks, results, task_ids, n_ids, plans, bins_area, sym_area, sym_stride, offpos_area, offpos_stride, nullptr, nullptr, ranges);
}

// numbers of scratch a task of route 2 takes: the batches it walks, and one more for lookback's output, which lags by the state (decode_page_body)
__host__ __device__ inline uint64_t range_scratch_numbers(uint64_t page_n, uint64_t first, uint64_t count) {
  const uint64_t want = range_end_batch(first, count) * kBatchN + kBatchN;
  return want < page_n ? want : page_n;
}

// One wave per task, as pco_decode_kernel's wrapped-page branch: the page's prefix goes to scratch_base + scratch_off[bi].
template <class L>
__global__ __launch_bounds__(64, kDecMinWaves) void pco_decode_prefix_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids,
                                                        uint32_t n_ids, uint32_t lds_table_budget, uint8_t* tbl_ws_base,
                                                        const uint32_t* only_if_status, uint32_t status_stride_u32, uint32_t status_value,
                                                        uint8_t* scratch_base, const uint64_t* scratch_off, uint8_t* hist_base, uint32_t need_hist_status,
                                                        const MetaRef* metas, const RangeRef* ranges) {
  const uint32_t lane = lane_id();
  for (uint32_t bi = blockIdx.x; bi < n_ids; bi += gridDim.x) {
    const uint32_t ti = task_ids ? task_ids[bi] : bi;
    if (only_if_status && uni(only_if_status[(uint64_t)ti * status_stride_u32]) != status_value) continue;
    const uint64_t first = uni(ranges[ti].first), count = uni(ranges[ti].count);
    if (count == 0) continue;
    const PcoGfxDecodeTask task = tasks[ti];
    gcptr_u8 src = (gcptr_u8)task.src;
    const uint64_t src_len = uni((uint64_t)task.src_len);
    const uint32_t dtype = uni(task.dtype), flags = uni(task.flags);
    const uint32_t n = (uint32_t)uni((uint64_t)task.dst_cap);   // (the page's count: 1 ..= 2^24, checked by the host)
    const uint64_t lim64 = range_end_batch(first, count) * kBatchN;
    const uint32_t limit = lim64 < n ? (uint32_t)lim64 : n;
    uint32_t status = dtype_bits(dtype) != (int)LBits<L>::v ? (uint32_t)PCO_GFX_INVALID_ARGUMENT : (uint32_t)PCO_GFX_OK;
    gcptr_u8 meta_p = (gcptr_u8)metas[ti].p;
    const uint64_t meta_len = uni((uint64_t)metas[ti].len);
    MetaReader mr{meta_p, meta_len, 0};
    if (!status) {
      gptr_u8 tbl_ws = tbl_ws_base ? (gptr_u8)tbl_ws_base + (uint64_t)blockIdx.x * kTblWsBytes : (gptr_u8) nullptr;
      decode_chunk<L, true>(meta_p, meta_len, mr, lds_table_budget, tbl_ws, (flags >> 8) & 0xffu, dtype, n, (L PCO_GLOBAL*)(scratch_base + scratch_off[bi]), status, false,
                            hist_base ? (void PCO_GLOBAL*)(hist_base + scratch_off[bi]) : (void PCO_GLOBAL*)nullptr, need_hist_status, nullptr, src, src_len, limit);
      status = uni(status);
    }
    if (lane == 0) {
      PcoGfxTaskResult r; r.n_out = status ? 0 : count; r.consumed = (!status && limit >= n) ? (mr.bit >> 3) : 0; r.status = status; r.aux = 0;
      results[ti] = r;
    }
    wave_sync_lds();
  }
}

// grid (tasks, slices): block (x, y) copies every gridDim.y-th stretch of 4096 numbers of task x's range
template <class L>
__global__ __launch_bounds__(256) void range_copy_kernel(const PcoGfxDecodeTask* tasks, const PcoGfxTaskResult* results, const uint32_t* task_ids, uint32_t n_ids,
                                                         const uint32_t* only_if_status, uint32_t status_stride_u32, uint32_t status_value,
                                                         const uint8_t* scratch_base, const uint64_t* scratch_off, const RangeRef* ranges) {
  for (uint32_t bi = blockIdx.x; bi < n_ids; bi += gridDim.x) {
    const uint32_t ti = task_ids ? task_ids[bi] : bi;
    if (only_if_status && only_if_status[(uint64_t)ti * status_stride_u32] != status_value) continue;
    if (results[ti].status != PCO_GFX_OK) continue;
    const uint64_t first = ranges[ti].first, count = ranges[ti].count;
    const L* from = (const L*)(scratch_base + scratch_off[bi]) + first;
    L* to = (L*)tasks[ti].dst;
    for (uint64_t at = (uint64_t)blockIdx.y * 4096; at < count; at += (uint64_t)gridDim.y * 4096) {
      const uint64_t end = at + 4096 < count ? at + 4096 : count;
      for (uint64_t i = at + threadIdx.x; i < end; i += 256) to[i] = from[i];
    }
  }
}

}  // namespace pcogfx
