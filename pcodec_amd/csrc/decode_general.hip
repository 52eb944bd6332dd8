// decode_general.hip -- the kernels of PCO_GFX_CURSOR_GENERAL (include/pco_gfx.h section 4h): full-state cursors for the pages the GENERAL
// kernel decodes -- Conv1, Dict under None / Consecutive / Conv1, tables beyond the walkers' LDS slices -- so that a read of such a page starts at
// its `from` cursor's batch and an index of it is one walk.
//
// What the single-kernel decoder carries between two batches of a page without Lookback is the bit position, four tANS states per variable, the
// count of numbers left, and either the consecutive moments or Conv1's `order` <= 32 residuals: the kind-3 cursor (pco_cursor.h).  Lookback's
// history is the output itself; those pages keep position-only cursors and the prefix decode.  The kernels are decode_chunk and the two page
// bodies compiled with kResume or kIndex (decode_kernel.hip): new instantiations under new names, the ones the other entry points launch are what
// they were.  A flagged call runs them on the scratch route in place of pco_decode_prefix_kernel:
//   pco_decode_general_resume_kernel<L>   a read task the walkers handed back: parses the ChunkMeta and the page header and builds the tables as always,
//                                         copies and judges the `from` cursor, walks batches [at / 256, ceil((first + count) / 256)) into the
//                                         task's scratch relative to its start batch, writes the kind-3 `to` cursor on PCO_GFX_OK and says in
//                                         rel_ranges where range_copy_kernel finds the rows.  A Lookback page, or a task whose two-kernel walk failed
//                                         in the page's body, is the prefix decode from row 0.
//   pco_decode_general_index_kernel<L>    an index task: walks batches [0, k * every_batches) without join, dictionary lookup or store and writes a
//                                         kind-3 cursor behind every batch index_slot() names; a Lookback page gets the first batch's verdict as
//                                         before, and index_finish_kernel its position-only cursors.
//   reads_shadow_kernel                   the two-kernel route's kernels are launched unchanged, and their expander judges the `from` cursor of a
//                                         handed-back task as position-only.  It is given a SHADOW of every kind-3 cursor -- version, row,
//                                         page_n | dtype under kind 2 -- so that a page on the two-kernel route refuses a kind-3 cursor and a
//                                         handed-back one comes here, where the real cursor is copied and judged.
//
// pco_gfx_decompress_page_reads_hist (section 4i) runs the same resume kernel compiled with kHist = true: it takes one history buffer per task and the
// call's flag behind the other arguments, and a resumable Lookback page then starts at its kind-4 cursor's batch with the rows in front of it read from
// the buffer's ring (decode_kernel.hip, pco_history.h).  reads_shadow_hist_kernel is that call's reads_shadow_kernel.
//
// pco_gfx_index_pages_hist (section 4j) runs the index kernel compiled with kHist, pco_decode_general_index_hist_kernel: a resumable Lookback page whose
// task brought histories is walked once into prefix scratch and gets kind-4 cursors, and index_history_snapshot_kernel then copies the k rings out of
// the scratch and stamps them (pco_history.h: history_snapshot_rows, history_at).
#pragma once
#include "decode_resume.hip"
#include "decode_index.hip"

namespace pcogfx {

// walk_caps[bi]: the batches of prefix scratch the host gave list entry bi; rel_ranges[ti]: out, the task's rows relative to its scratch
struct GeneralResumeArgs { const ReadRef* refs; ReadRec* recs; const uint32_t* walk_caps; RangeRef* rel_ranges; };
// pco_gfx_decompress_page_reads_hist (section 4i): hrefs[ti] is the task's history buffer, or {nullptr, 0}; allow_general the call's PCO_GFX_CURSOR_GENERAL.
// Only the kernel compiled with kHist takes them; the other's argument list is what it was.
struct HistRef { void* p; uint64_t len; };
struct HistArgs { const HistRef* hrefs; uint32_t allow_general; };
template <bool kHist> using hist_args = std::conditional_t<kHist, HistArgs, NoGeneralIO>;

template <class L, bool kHist = false>
__global__ __launch_bounds__(64, kDecMinWaves) void pco_decode_general_resume_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids,
                                                        uint32_t n_ids, uint32_t lds_table_budget, uint8_t* tbl_ws_base,
                                                        const uint32_t* only_if_status, uint32_t status_stride_u32, uint32_t status_value,
                                                        uint8_t* scratch_base, const uint64_t* scratch_off, uint8_t* hist_base, uint32_t need_hist_status,
                                                        const MetaRef* metas, const RangeRef* ranges, GeneralResumeArgs ga, hist_args<kHist> ha = {}) {
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
    // route 2: the expander passed the task's cursor (or its shadow) as a position; route 3: the two-kernel walk failed in the page's body and
    // had its verdict -- the prefix from row 0 gives the error, and no cursor is read or written
    const bool own = uni(ga.recs[ti].route) == 2u;
    std::conditional_t<kHist, HistIO, GeneralIO> gio{};
    static_cast<GeneralIO&>(gio) = GeneralIO{own ? ga.refs[ti].from : nullptr, own ? ga.refs[ti].to : nullptr, first, count, uni(ga.walk_caps[bi]), dtype, nullptr, 0, 0, 0, 0};
    if constexpr (kHist) {   // (a task that came for its error -- route 3 -- reads no history either)
      gio.history = own ? ha.hrefs[ti].p : nullptr; gio.history_len = own ? uni(ha.hrefs[ti].len) : 0; gio.allow_general = ha.allow_general;
    }
    if (!status) {
      gptr_u8 tbl_ws = tbl_ws_base ? (gptr_u8)tbl_ws_base + (uint64_t)blockIdx.x * kTblWsBytes : (gptr_u8) nullptr;
      decode_chunk<L, true, true, false, kHist>(meta_p, meta_len, mr, lds_table_budget, tbl_ws, (flags >> 8) & 0xffu, dtype, n, (L PCO_GLOBAL*)(scratch_base + scratch_off[bi]), status, false,
                                         hist_base ? (void PCO_GLOBAL*)(hist_base + scratch_off[bi]) : (void PCO_GLOBAL*)nullptr, need_hist_status, nullptr, src, src_len, limit, &gio);
      status = uni(status);
    }
    if (lane == 0) {
      PcoGfxTaskResult r; r.n_out = status ? 0 : count; r.consumed = (!status && limit >= n) ? (mr.bit >> 3) : 0; r.status = status; r.aux = 0;
      results[ti] = r;
      ga.rel_ranges[ti] = RangeRef{first - uni(gio.start_row), count};
      if (own && uni(gio.general)) ga.recs[ti].route = 0;   // its `to` cursor is written: nothing for reads_finish_kernel
    }
    wave_sync_lds();
  }
}

template <class L>
__global__ __launch_bounds__(64, kDecMinWaves) void pco_decode_general_index_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids,
                                                        uint32_t n_ids, uint32_t lds_table_budget, uint8_t* tbl_ws_base,
                                                        const uint32_t* only_if_status, uint32_t status_stride_u32, uint32_t status_value,
                                                        uint8_t* scratch_base, const uint64_t* scratch_off, uint8_t* hist_base, uint32_t need_hist_status,
                                                        const MetaRef* metas, const RangeRef* ranges, IndexArgs ix, DecPlan* plans) {
  const uint32_t lane = lane_id();
  for (uint32_t bi = blockIdx.x; bi < n_ids; bi += gridDim.x) {
    const uint32_t ti = task_ids ? task_ids[bi] : bi;
    if (only_if_status && uni(only_if_status[(uint64_t)ti * status_stride_u32]) != status_value) continue;
    const uint64_t first = uni(ranges[ti].first), count = uni(ranges[ti].count);   // (the range {0, 1} a Lookback page decodes for its verdict)
    if (count == 0) continue;
    const PcoGfxDecodeTask task = tasks[ti];
    gcptr_u8 src = (gcptr_u8)task.src;
    const uint64_t src_len = uni((uint64_t)task.src_len);
    const uint32_t dtype = uni(task.dtype), flags = uni(task.flags);
    const uint32_t n = (uint32_t)uni((uint64_t)task.dst_cap);
    const uint64_t lim64 = range_end_batch(first, count) * kBatchN;
    const uint32_t limit = lim64 < n ? (uint32_t)lim64 : n;
    uint32_t status = dtype_bits(dtype) != (int)LBits<L>::v ? (uint32_t)PCO_GFX_INVALID_ARGUMENT : (uint32_t)PCO_GFX_OK;
    gcptr_u8 meta_p = (gcptr_u8)metas[ti].p;
    const uint64_t meta_len = uni((uint64_t)metas[ti].len);
    MetaReader mr{meta_p, meta_len, 0};
    const IndexRef ir = ix.refs[ti];
    GeneralIO gio{nullptr, nullptr, 0, 0, 0, dtype, ir.cursors, uni(ir.every_batches), uni(ir.k), 0, 0};
    if (!status) {
      gptr_u8 tbl_ws = tbl_ws_base ? (gptr_u8)tbl_ws_base + (uint64_t)blockIdx.x * kTblWsBytes : (gptr_u8) nullptr;
      decode_chunk<L, true, false, true>(meta_p, meta_len, mr, lds_table_budget, tbl_ws, (flags >> 8) & 0xffu, dtype, n, (L PCO_GLOBAL*)(scratch_base + scratch_off[bi]), status, false,
                                         hist_base ? (void PCO_GLOBAL*)(hist_base + scratch_off[bi]) : (void PCO_GLOBAL*)nullptr, need_hist_status, nullptr, src, src_len, limit, &gio);
      status = uni(status);
    }
    if (lane == 0) {
      PcoGfxTaskResult r; r.consumed = 0; r.status = status; r.aux = 0;
      if (uni(gio.general)) {   // walked here: the result is final, and index_finish_kernel, which goes by the plan's status, passes the task by
        r.n_out = status ? 0 : (uint64_t)gio.k;
        plans[ti].status = status;
      } else { r.n_out = status ? 0 : count; r.consumed = (!status && limit >= n) ? (mr.bit >> 3) : 0; }
      results[ti] = r;
    }
    wave_sync_lds();
  }
}

// pco_gfx_index_pages_hist (section 4j): histories[ti] / stride of the task, or {nullptr, 0}.  recs[ti], zeroed by the host before the call's first launch, is
// what the walk tells index_history_snapshot_kernel: snap = 1 -- F of the walked prefix stands in the task's scratch.
struct IndexHistRef { void* histories; uint64_t stride; };
struct IndexHistRec { uint32_t snap, state_n, window_n_log, raw, num_kind, pad; };
struct IndexHistArgs { const IndexHistRef* hrefs; IndexHistRec* recs; const uint32_t* walk_caps; uint32_t allow_general; };

// pco_decode_general_index_kernel compiled with kHist: a resumable Lookback page whose task brought histories is walked ONCE over batches
// [0, k * every_batches) into walk_caps[bi] + 1 batches of prefix scratch and gets kind-4 cursors; every other task is that kernel's, or -- without the
// call's flag -- the prefix kernel's over its first batch.
template <class L>
__global__ __launch_bounds__(64, kDecMinWaves) void pco_decode_general_index_hist_kernel(const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results, const uint32_t* task_ids,
                                                        uint32_t n_ids, uint32_t lds_table_budget, uint8_t* tbl_ws_base,
                                                        const uint32_t* only_if_status, uint32_t status_stride_u32, uint32_t status_value,
                                                        uint8_t* scratch_base, const uint64_t* scratch_off, uint8_t* hist_base, uint32_t need_hist_status,
                                                        const MetaRef* metas, const RangeRef* ranges, IndexArgs ix, DecPlan* plans, IndexHistArgs ha) {
  const uint32_t lane = lane_id();
  for (uint32_t bi = blockIdx.x; bi < n_ids; bi += gridDim.x) {
    const uint32_t ti = task_ids ? task_ids[bi] : bi;
    if (only_if_status && uni(only_if_status[(uint64_t)ti * status_stride_u32]) != status_value) continue;
    const uint64_t count = uni(ranges[ti].count);   // (0 or 1: the first batch, for the verdict of a page that keeps position-only cursors)
    if (count == 0) continue;
    const PcoGfxDecodeTask task = tasks[ti];
    gcptr_u8 src = (gcptr_u8)task.src;
    const uint64_t src_len = uni((uint64_t)task.src_len);
    const uint32_t dtype = uni(task.dtype), flags = uni(task.flags);
    const uint32_t n = (uint32_t)uni((uint64_t)task.dst_cap);
    const uint32_t limit = kBatchN < n ? kBatchN : n;
    uint32_t status = dtype_bits(dtype) != (int)LBits<L>::v ? (uint32_t)PCO_GFX_INVALID_ARGUMENT : (uint32_t)PCO_GFX_OK;
    gcptr_u8 meta_p = (gcptr_u8)metas[ti].p;
    const uint64_t meta_len = uni((uint64_t)metas[ti].len);
    MetaReader mr{meta_p, meta_len, 0};
    const IndexRef ir = ix.refs[ti];
    IndexHistIO gio{};
    static_cast<GeneralIO&>(gio) = GeneralIO{nullptr, nullptr, 0, 0, uni(ha.walk_caps[bi]), dtype, ir.cursors, uni(ir.every_batches), uni(ir.k), 0, 0};
    gio.history = ha.hrefs[ti].histories; gio.history_len = uni(ha.hrefs[ti].stride); gio.allow_general = ha.allow_general; gio.hand_back = need_hist_status;
    if (!status) {
      gptr_u8 tbl_ws = tbl_ws_base ? (gptr_u8)tbl_ws_base + (uint64_t)blockIdx.x * kTblWsBytes : (gptr_u8) nullptr;
      decode_chunk<L, true, false, true, true>(meta_p, meta_len, mr, lds_table_budget, tbl_ws, (flags >> 8) & 0xffu, dtype, n, (L PCO_GLOBAL*)(scratch_base + scratch_off[bi]), status, false,
                                               hist_base ? (void PCO_GLOBAL*)(hist_base + scratch_off[bi]) : (void PCO_GLOBAL*)nullptr, need_hist_status, nullptr, src, src_len, limit, &gio);
      status = uni(status);
    }
    if (lane == 0) {
      PcoGfxTaskResult r; r.consumed = 0; r.status = status; r.aux = 0;
      if (uni(gio.general)) {   // walked here, or refused for its stride: the result is final, and index_finish_kernel passes the task by
        r.n_out = status ? 0 : (uint64_t)gio.k;
        plans[ti].status = status;
        if (!status && uni(gio.snap)) ha.recs[ti] = IndexHistRec{1u, uni(gio.state_n), uni(gio.window_n_log), uni(gio.raw), uni(gio.num_kind), 0u};
      } else r.n_out = status ? 0 : count;
      results[ti] = r;
    }
    wave_sync_lds();
  }
}

// After the walk, the rings out of the scratch: history i of a task whose record says `snap` takes F[lo_i, hi_i) (history_snapshot_rows) into the slots
// j & (window_n - 1) behind its 64-byte header, and the stamp `row (i + 1) * every_rows`.  blockIdx.y strides the list's tasks, blockIdx.x the task's
// (cursor, stretch of kSnapRows rows) pairs.  A thread moves 8 bytes at a time: the scratch is 256-byte aligned and a history 8-byte aligned, so a
// group of 8 / sizeof(L) rows that starts at a multiple of that many is one aligned load and one aligned store (the ring wraps at a multiple of it
// too); the ragged ends of a history's rows, and a ring shorter than 8 bytes, go row by row.  The rings are not read again here: non-temporal stores.
constexpr uint32_t kSnapRows = 2048;
template <class L>
__global__ __launch_bounds__(256) void index_history_snapshot_kernel(const PcoGfxDecodeTask* tasks, const PcoGfxTaskResult* results, const uint32_t* task_ids, uint32_t n_ids,
                                                                     const uint8_t* scratch_base, const uint64_t* scratch_off, const IndexRef* irefs, IndexHistArgs ha) {
  constexpr uint32_t kGroup = 8 / (uint32_t)sizeof(L);
  for (uint32_t bi = blockIdx.y; bi < n_ids; bi += gridDim.y) {
    const uint32_t ti = task_ids ? task_ids[bi] : bi;
    const IndexHistRec rec = ha.recs[ti];   // (the walk of THIS launch's list wrote it, or nobody: the plan's status, which the walk has replaced, is no filter here)
    if (!rec.snap || results[ti].status != PCO_GFX_OK) continue;
    const IndexRef ir = irefs[ti];
    const IndexHistRef hr = ha.hrefs[ti];
    const uint64_t page_n = tasks[ti].dst_cap, every_rows = (uint64_t)ir.every_batches * kBatchN;
    const uint32_t dtype = tasks[ti].dtype, wlog = rec.window_n_log;
    const L* F = (const L*)(scratch_base + scratch_off[bi]);
    // the longest history is the last cursor's: every cursor gets that many stretches, and passes by the ones behind its rows
    const HistoryRows last = history_snapshot_rows((uint64_t)ir.k * every_rows, rec.state_n, page_n, wlog);
    const uint64_t n_stretch = (last.hi - last.lo + kGroup + kSnapRows - 1) / kSnapRows;
    for (uint64_t item = blockIdx.x; item < (uint64_t)ir.k * n_stretch; item += gridDim.x) {
      const uint64_t i = item / n_stretch, s = item % n_stretch, row = (i + 1) * every_rows;
      const HistoryRows rows = history_snapshot_rows(row, rec.state_n, page_n, wlog);
      uint8_t* h = history_at(hr.histories, hr.stride, i);
      L* ring = (L*)(h + kHistoryHeaderBytes);
      auto latent = [&](L v) -> L { return rec.raw ? v : to_latent_ordered<L>(v, rec.num_kind); };
      const uint64_t at = (rows.lo & ~(uint64_t)(kGroup - 1)) + s * kSnapRows;
      const uint64_t end = at + kSnapRows < rows.hi ? at + kSnapRows : rows.hi;
      for (uint64_t j0 = at + (uint64_t)threadIdx.x * kGroup; j0 < end; j0 += 256 * kGroup) {
        if (j0 >= rows.lo && j0 + kGroup <= rows.hi && wlog >= 3 - __builtin_ctz(sizeof(L))) {
          const uint64_t in = *(const uint64_t*)(F + j0);
          uint64_t out = 0;
#pragma unroll
          for (uint32_t e = 0; e < kGroup; e++) out |= (uint64_t)latent((L)(in >> (8 * sizeof(L) * e))) << (8 * sizeof(L) * e);
          __builtin_nontemporal_store(out, (uint64_t*)(ring + history_slot(j0, wlog)));
        } else {
          for (uint64_t j = j0 < rows.lo ? rows.lo : j0; j < j0 + kGroup && j < rows.hi; j++) ring[history_slot(j, wlog)] = latent(F[j]);
        }
      }
      if (s == 0 && threadIdx.x < kHistoryHeaderWords) ((uint64_t*)h)[threadIdx.x] = history_header_word(threadIdx.x, row, page_n, dtype, wlog);
    }
  }
}

// One thread per read task of a flagged call, before anything else: the refs the two-kernel route's kernels get, and the rows the host sizes by.
// shadow_refs[i] is refs[i] with a kind-3 `from` replaced by its position-only shadow in shadow_words[32 i ..]; rows[i] the row `from` stands at
// (what reads_rows_kernel gives), general_rows[i] that row for a kind-3 cursor and 0 for every other -- a position-only cursor starts no walk.
// A task without rows reads nothing, its `from` included.
__global__ void reads_shadow_kernel(const ReadRef* refs, const RangeRef* ranges, uint32_t n_tasks, ReadRef* shadow_refs, uint64_t* shadow_words, uint64_t* rows,
                                    uint64_t* general_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tasks) return;
  ReadRef r = refs[i];
  uint64_t row = 0, grow = 0;
  if (ranges[i].count == 0) r.from = nullptr;
  if (r.from != nullptr) {
    const uint64_t w0 = r.from[0];
    row = r.from[1];
    if ((uint32_t)(w0 >> 32) == kCursorGeneral) {
      uint64_t* sw = shadow_words + (uint64_t)i * kCursorWords;
      sw[0] = (w0 & 0xffffffffull) | ((uint64_t)kCursorPosition << 32); sw[1] = row; sw[2] = 0; sw[3] = r.from[3];
      for (uint32_t k = 4; k < kCursorWords; k++) sw[k] = 0;
      r.from = sw; grow = row;
    }
  }
  shadow_refs[i] = r; rows[i] = row; general_rows[i] = grow;
}

// reads_shadow_kernel for a call of pco_gfx_decompress_page_reads_hist: a kind-3 `from` gets its shadow under the call's flag only, a kind-4 one when its
// task brought a history -- every other cursor goes to the expander as it is, which refuses what is not position-only, as in a call without either.
__global__ void reads_shadow_hist_kernel(const ReadRef* refs, const RangeRef* ranges, const HistRef* hrefs, uint32_t allow_general, uint32_t n_tasks, ReadRef* shadow_refs,
                                         uint64_t* shadow_words, uint64_t* rows, uint64_t* general_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tasks) return;
  ReadRef r = refs[i];
  uint64_t row = 0, grow = 0;
  if (ranges[i].count == 0) r.from = nullptr;
  if (r.from != nullptr) {
    const uint64_t w0 = r.from[0];
    const uint32_t kind = (uint32_t)(w0 >> 32);
    row = r.from[1];
    if ((kind == kCursorGeneral && allow_general) || (kind == kCursorLookback && hrefs[i].p != nullptr)) {
      uint64_t* sw = shadow_words + (uint64_t)i * kCursorWords;
      sw[0] = (w0 & 0xffffffffull) | ((uint64_t)kCursorPosition << 32); sw[1] = row; sw[2] = 0; sw[3] = r.from[3];
      for (uint32_t k = 4; k < kCursorWords; k++) sw[k] = 0;
      r.from = sw; grow = row;
    }
  }
  shadow_refs[i] = r; rows[i] = row; general_rows[i] = grow;
}

}  // namespace pcogfx
