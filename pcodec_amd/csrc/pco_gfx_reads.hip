// pco_gfx_reads.hip -- pco_gfx_decompress_page_reads (include/pco_gfx.h section 4f): a translation unit of its own, so that the kernels the other
// entry points launch are compiled exactly as before.  The kernels are in decode_resume.hip (route 1) and decode_range.hip (route 2); the launch
// sequence is pco_gfx_ranges.hip's with the cursors' arrays beside the tasks', scratch sized by the batches walked, and a finishing kernel.
#include "pco_host.h"
#include "pco_half.h"

#include <cstring>
#include <string>
#include <vector>

#include "decode_resume.hip"

static_assert(sizeof(PcoGfxPageCursor) == 8 * pcogfx::kCursorWords, "PcoGfxPageCursor");
static_assert(sizeof(PcoGfxPageReadTask) == 88, "PcoGfxPageReadTask");

namespace pcogfx {

hipEvent_t profile_span_begin(const char* name, hipStream_t stream);   // pco_gfx.hip: pco_gfx_profile_begin / _end time this unit's launches too

namespace {

struct ReadTimer {
  hipStream_t s; hipEvent_t b;
  ReadTimer(const char* name, hipStream_t stream) : s(stream), b(profile_span_begin(name, stream)) {}
  ~ReadTimer() { if (b) (void)hipEventRecord(b, s); }
};
#define PCO_READ_LAUNCH(name, stream, ...) do { ReadTimer _t(name, stream); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

constexpr uint32_t kReadDecodeLdsBytes = 16 * 1024;   // the single-kernel decoder's dynamic LDS (fixed area + tANS tables), as in launch_decode
constexpr size_t kReadGeneralGrid = 4096;             // ... and its grid bound: each block owns kTblWsBytes of table scratch

// what the scratch of one synchronous pass may take: PCO_GFX_WORKSPACE_GB, default 80 % of the free device memory (plus what the buffer holds)
size_t read_budget_bytes(const Workspace& ws) {
  const char* env = std::getenv("PCO_GFX_WORKSPACE_GB");
  if (env && *env) return (size_t)(std::atof(env) * 1e9);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ~(size_t)0;
  return (size_t)((free_b + ws.dec_hist.cap) * 0.8);
}

int width_group(uint32_t dtype) { const int b = dtype_bits(dtype); return b == 64 ? 0 : (b == 32 ? 1 : (b == 16 ? 2 : (b == 8 ? 3 : -1))); }

template <class L>
void launch_fast_read(const char* const (&names)[3], hipStream_t stream, uint32_t cnt, uint32_t grid, const PcoGfxDecodeTask* d_tasks, const uint32_t* idp, DecPlan* d_plans,
                      uint8_t* d_bins, uint8_t* d_sym, uint64_t sym_stride, uint64_t* d_offpos, uint64_t offpos_stride, PcoGfxTaskResult* d_results, const MetaRef* d_metas,
                      const RangeRef* d_ranges, ResumeArgs rz) {
  static const bool walk_ok = hipFuncSetAttribute((const void*)dec_walk_resume_kernel<L, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * WalkCfg<8>::kWalkLdsBytes)) == hipSuccess &&
                              hipFuncSetAttribute((const void*)dec_walk_resume_kernel<L, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * WalkCfg<4>::kWalkLdsBytes)) == hipSuccess;
  if (!walk_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for dec_walk_resume_kernel"};
  const uint32_t n_wb = (cnt + 7) / 8;
  PCO_READ_LAUNCH(names[0], stream, (dec_walk_resume_kernel<L, 8>), dim3((n_wb + 3) / 4), dim3(256), 4 * WalkCfg<8>::kWalkLdsBytes, stream,
                  d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, 0u, d_results, d_metas, d_ranges, rz);
  PCO_READ_LAUNCH(names[1], stream, (dec_walk_resume_kernel<L, 4>), dim3((cnt + 15) / 16), dim3(256), 4 * WalkCfg<4>::kWalkLdsBytes, stream,
                  d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, kStatusRetryK4, d_results, d_metas, d_ranges, rz);
  PCO_READ_LAUNCH(names[2], stream, (dec_expand_resume_kernel<L>), dim3(grid), dim3(256), kExpLdsBytes, stream,
                  d_tasks, d_results, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_ranges, rz);
}

template <class L>
void launch_scratch_read(const char* const (&names)[2], hipStream_t stream, uint32_t cnt, uint32_t grid, uint32_t copy_slices, const PcoGfxDecodeTask* d_tasks,
                         PcoGfxTaskResult* d_results, const uint32_t* idp, uint8_t* tbl, const uint32_t* filt, uint32_t fstride, uint8_t* d_scratch, const uint64_t* d_off,
                         uint8_t* d_hist, uint32_t need_hist, const MetaRef* d_metas, const RangeRef* d_ranges) {
  PCO_READ_LAUNCH(names[0], stream, pco_decode_prefix_kernel<L>, dim3(grid), dim3(64), kReadDecodeLdsBytes, stream, d_tasks, d_results, idp, cnt,
                  kReadDecodeLdsBytes - kLdsFixed, tbl, filt, fstride, kStatusRetryLegacy, d_scratch, d_off, d_hist, need_hist, d_metas, d_ranges);
  PCO_READ_LAUNCH(names[1], stream, range_copy_kernel<L>, dim3(std::min<uint32_t>(cnt, 16384u), copy_slices), dim3(256), 0, stream, d_tasks,
                  (const PcoGfxTaskResult*)d_results, idp, cnt, filt, fstride, kStatusRetryLegacy, (const uint8_t*)d_scratch, d_off, d_ranges);
}

const char* const kFastNames[4][3] = {{"dec_walk_resume_kernel<u64>", "dec_walk4_resume_kernel<u64>", "dec_expand_resume_kernel<u64>"},
                                      {"dec_walk_resume_kernel<u32>", "dec_walk4_resume_kernel<u32>", "dec_expand_resume_kernel<u32>"},
                                      {"dec_walk_resume_kernel<u16>", "dec_walk4_resume_kernel<u16>", "dec_expand_resume_kernel<u16>"},
                                      {"dec_walk_resume_kernel<u8>", "dec_walk4_resume_kernel<u8>", "dec_expand_resume_kernel<u8>"}};
const char* const kScratchNames[4][2] = {{"pco_decode_prefix_kernel<u64>", "range_copy_kernel<u64>"}, {"pco_decode_prefix_kernel<u32>", "range_copy_kernel<u32>"},
                                         {"pco_decode_prefix_kernel<u16>", "range_copy_kernel<u16>"}, {"pco_decode_prefix_kernel<u8>", "range_copy_kernel<u8>"}};

void launch_decode_reads(size_t n_tasks, const PcoGfxPageReadTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results_user, hipStream_t stream) {
  if (n_tasks == 0) return;
  if (n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: too many tasks"};
  Workspace& ws = workspace();
  std::vector<PcoGfxDecodeTask> dt(n_tasks); std::vector<MetaRef> refs(n_tasks); std::vector<RangeRef> rr(n_tasks); std::vector<ReadRef> cr(n_tasks);
  std::vector<uint32_t> flat; size_t id_off[5] = {0, 0, 0, 0, 0};
  uint64_t max_count = 0; bool any_from = false;
  {
    std::vector<uint32_t> ids[4];
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageReadTask& t = tasks[i];
      dt[i] = PcoGfxDecodeTask{t.page, t.page_len, t.dst, t.page_n, t.dtype, PCO_GFX_TASK_WRAPPED_PAGE | (t.format_major << 8)};
      refs[i] = MetaRef{t.meta, t.meta_len}; rr[i] = RangeRef{t.first, t.count};
      cr[i] = ReadRef{t.from ? t.from->w : nullptr, t.to ? t.to->w : nullptr};
      any_from = any_from || (t.from != nullptr && t.count != 0);
      ids[width_group(t.dtype)].push_back((uint32_t)i);
      max_count = std::max<uint64_t>(max_count, t.count);
    }
    for (int g = 0; g < 4; g++) { id_off[g] = flat.size(); flat.insert(flat.end(), ids[g].begin(), ids[g].end()); }
    id_off[4] = flat.size();
  }
  // device arrays: tasks | ids (grouped by number width) | ChunkMeta references | ranges | cursor references | per-task records | cursor rows
  const size_t task_bytes = n_tasks * sizeof(PcoGfxDecodeTask);
  const size_t ids_off = (task_bytes + 15) & ~(size_t)15, metas_off = (ids_off + n_tasks * sizeof(uint32_t) + 15) & ~(size_t)15;
  const size_t ranges_off = (metas_off + n_tasks * sizeof(MetaRef) + 15) & ~(size_t)15;
  const size_t curs_off = (ranges_off + n_tasks * sizeof(RangeRef) + 15) & ~(size_t)15;
  const size_t recs_off = (curs_off + n_tasks * sizeof(ReadRef) + 15) & ~(size_t)15;
  const size_t rows_off = (recs_off + n_tasks * sizeof(ReadRec) + 15) & ~(size_t)15;
  uint8_t* d_base = (uint8_t*)ws.tasks.ensure(rows_off + n_tasks * sizeof(uint64_t) + 64);
  const PcoGfxDecodeTask* d_tasks = (const PcoGfxDecodeTask*)d_base;
  const uint32_t* d_ids = (const uint32_t*)(d_base + ids_off);
  const MetaRef* d_metas = (const MetaRef*)(d_base + metas_off);
  const RangeRef* d_ranges = (const RangeRef*)(d_base + ranges_off);
  const ReadRef* d_curs = (const ReadRef*)(d_base + curs_off);
  ReadRec* d_recs = (ReadRec*)(d_base + recs_off);
  PCO_HIP_CHECK(hipMemcpyAsync(d_base, dt.data(), task_bytes, hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + ids_off, flat.data(), n_tasks * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + metas_off, refs.data(), n_tasks * sizeof(MetaRef), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + ranges_off, rr.data(), n_tasks * sizeof(RangeRef), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + curs_off, cr.data(), n_tasks * sizeof(ReadRef), hipMemcpyHostToDevice, stream));
  // symbols and section starts: sized by the most batches a task of the call WALKS, ceil((first + count) / 256) - at / 256.  `at` lives in the `from`
  // cursor on the device: a synchronous call reads the rows back; an asynchronous one cannot, and sizes by the end batch as a range call does.
  std::vector<uint64_t> rows(n_tasks, 0);
  if (results && any_from) {
    uint64_t* d_rows = (uint64_t*)(d_base + rows_off);
    PCO_READ_LAUNCH("reads_rows_kernel", stream, reads_rows_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_curs, (uint32_t)n_tasks, d_rows);
    PCO_HIP_CHECK(hipMemcpyAsync(rows.data(), d_rows, n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  uint64_t max_walk = 0;
  for (size_t i = 0; i < n_tasks; i++) {
    if (!tasks[i].count) continue;
    const uint64_t b_end = range_end_batch(tasks[i].first, tasks[i].count);
    max_walk = std::max<uint64_t>(max_walk, b_end - std::min<uint64_t>(rows[i] >> 8, b_end - 1));   // (a cursor behind `first` is refused on the device)
  }
  PcoGfxTaskResult* d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)ws.results.ensure(n_tasks * sizeof(PcoGfxTaskResult));
  const uint64_t sym_stride = max_walk * kBatchN + 256, offpos_stride = sym_stride / 256 + 2;
  if (n_tasks * 3 * sym_stride > ((size_t)48 << 30)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: the batches one call walks may take 48 GiB of symbol scratch at most; split the call"};
  const ResumeArgs rz{d_curs, d_recs, (uint32_t)max_walk};
  DecPlan* d_plans = nullptr;
  {
    d_plans = (DecPlan*)ws.dec_plans.ensure(n_tasks * sizeof(DecPlan));
    uint8_t* d_bins = (uint8_t*)ws.dec_bins.ensure(n_tasks * kBinsAreaPerTask);
    uint8_t* d_sym = (uint8_t*)ws.dec_sym.ensure(n_tasks * 3 * sym_stride + 64);
    uint64_t* d_offpos = (uint64_t*)ws.dec_offpos.ensure(n_tasks * 3 * offpos_stride * 8);
    for (int g = 0; g < 4; g++) {
      const uint32_t cnt = (uint32_t)(id_off[g + 1] - id_off[g]);
      if (!cnt) continue;
      const uint32_t grid = (uint32_t)std::min<size_t>(cnt, kReadGeneralGrid);
      const uint32_t* idp = d_ids + id_off[g];
      if (g == 0) launch_fast_read<uint64_t>(kFastNames[0], stream, cnt, grid, d_tasks, idp, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_results, d_metas, d_ranges, rz);
      else if (g == 1) launch_fast_read<uint32_t>(kFastNames[1], stream, cnt, grid, d_tasks, idp, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_results, d_metas, d_ranges, rz);
      else if (g == 2) launch_fast_read<uint16_t>(kFastNames[2], stream, cnt, grid, d_tasks, idp, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_results, d_metas, d_ranges, rz);
      else launch_fast_read<uint8_t>(kFastNames[3], stream, cnt, grid, d_tasks, idp, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_results, d_metas, d_ranges, rz);
      PCO_HIP_CHECK(hipGetLastError());
    }
  }
  const uint32_t copy_slices = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (max_count + 4095) / 4096));
  // Route 2 over the tasks `list` (task ids grouped by width, group g at [goff[g], goff[g + 1])): their prefixes into scratch, their ranges out of it.
  // filt: run over every task of the call and let the device pick the ones the walkers handed back (the asynchronous form).
  auto run_scratch = [&](const std::vector<uint32_t>& list, const size_t (&goff)[5], bool with_hist, const uint32_t* filt, uint32_t need_hist) {
    std::vector<uint64_t> offs(list.size()); uint64_t bytes = 0;
    for (size_t k = 0; k < list.size(); k++) {
      const PcoGfxPageReadTask& t = tasks[list[k]];
      offs[k] = bytes;
      if (t.count) bytes += (range_scratch_numbers(t.page_n, t.first, t.count) * (uint64_t)(dtype_bits(t.dtype) / 8) + 255) & ~(uint64_t)255;
    }
    const uint64_t hist_at = (bytes + 255) & ~(uint64_t)255, tail_at = hist_at + (with_hist ? hist_at : 0);
    uint8_t* d_scratch = (uint8_t*)ws.dec_hist.ensure(tail_at + list.size() * 12 + 256);
    uint64_t* d_off = (uint64_t*)(d_scratch + tail_at);
    uint32_t* d_list = (uint32_t*)(d_off + list.size());
    PCO_HIP_CHECK(hipMemcpyAsync(d_off, offs.data(), list.size() * 8, hipMemcpyHostToDevice, stream));
    PCO_HIP_CHECK(hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, stream));
    size_t max_grid = 0;
    for (int g = 0; g < 4; g++) max_grid = std::max(max_grid, std::min<size_t>(goff[g + 1] - goff[g], kReadGeneralGrid));
    uint8_t* tbl = (uint8_t*)ws.tbl_ws.ensure(max_grid * kTblWsBytes);
    const uint32_t fstride = (uint32_t)(sizeof(DecPlan) / 4);
    for (int g = 0; g < 4; g++) {
      const uint32_t cnt = (uint32_t)(goff[g + 1] - goff[g]);
      if (!cnt) continue;
      const uint32_t grid = (uint32_t)std::min<size_t>(cnt, kReadGeneralGrid);
      const uint32_t* idp = d_list + goff[g]; const uint64_t* op = d_off + goff[g];
      uint8_t* d_hist = with_hist ? d_scratch + hist_at : nullptr;
      if (g == 0) launch_scratch_read<uint64_t>(kScratchNames[0], stream, cnt, grid, copy_slices, d_tasks, d_results, idp, tbl, filt, fstride, d_scratch, op, d_hist, need_hist, d_metas, d_ranges);
      else if (g == 1) launch_scratch_read<uint32_t>(kScratchNames[1], stream, cnt, grid, copy_slices, d_tasks, d_results, idp, tbl, filt, fstride, d_scratch, op, d_hist, need_hist, d_metas, d_ranges);
      else if (g == 2) launch_scratch_read<uint16_t>(kScratchNames[2], stream, cnt, grid, copy_slices, d_tasks, d_results, idp, tbl, filt, fstride, d_scratch, op, d_hist, need_hist, d_metas, d_ranges);
      else launch_scratch_read<uint8_t>(kScratchNames[3], stream, cnt, grid, copy_slices, d_tasks, d_results, idp, tbl, filt, fstride, d_scratch, op, d_hist, need_hist, d_metas, d_ranges);
      PCO_HIP_CHECK(hipGetLastError());
    }
  };
  auto finish = [&]() {   // the position-only `to` cursors of route 2
    PCO_READ_LAUNCH("reads_finish_kernel", stream, reads_finish_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_tasks, d_ranges, d_curs,
                    (const ReadRec*)d_recs, d_results, (uint32_t)n_tasks);
    PCO_HIP_CHECK(hipGetLastError());
  };
  if (!results) {
    // asynchronous: the call cannot come back, so every task takes its prefix scratch up front and the device picks the tasks of route 2 (the history of
    // a delta'd secondary variable under lookback stays the one thing such a call does not have: PCO_GFX_UNSUPPORTED, as in pco_gfx_decompress_pages)
    run_scratch(flat, id_off, false, (const uint32_t*)d_plans, (uint32_t)PCO_GFX_UNSUPPORTED);
    finish();
    return;
  }
  // synchronous: the tasks the walkers handed back go through route 2 in passes whose scratch fits the budget; the ones that then ask for a second
  // history buffer once more, with it
  auto read_results = [&]() {
    PCO_HIP_CHECK(hipMemcpyAsync(results, d_results, n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  };
  read_results();
  bool any_scratch = false;
  for (int round = 0; round < 2; round++) {
    const uint32_t want = round == 0 ? kStatusRetryLegacy : kStatusNeedHist;
    const size_t budget = read_budget_bytes(ws);
    bool any = false;
    size_t at = 0;
    while (at < n_tasks) {   // (task order: a pass is a stretch of the call's tasks)
      std::vector<uint32_t> ids[4]; uint64_t bytes = 0; size_t taken = 0;
      for (; at < n_tasks; at++) {
        if (results[at].status != want) continue;
        const PcoGfxPageReadTask& t = tasks[at];
        const uint64_t b = ((range_scratch_numbers(t.page_n, t.first, t.count) * (uint64_t)(dtype_bits(t.dtype) / 8) + 255) & ~(uint64_t)255) * (round ? 2 : 1);
        if (taken && bytes + b > budget) break;
        ids[width_group(t.dtype)].push_back((uint32_t)at); bytes += b; taken++;
      }
      if (!taken) break;
      std::vector<uint32_t> list; size_t goff[5];
      for (int g = 0; g < 4; g++) { goff[g] = list.size(); list.insert(list.end(), ids[g].begin(), ids[g].end()); }
      goff[4] = list.size();
      run_scratch(list, goff, round == 1, nullptr, round == 0 ? kStatusNeedHist : (uint32_t)PCO_GFX_UNSUPPORTED);
      PCO_HIP_CHECK(hipStreamSynchronize(stream));   // (the next pass writes the same scratch, and may move it)
      any = true;
    }
    if (!any) break;
    any_scratch = true;
    read_results();
  }
  if (any_scratch) { finish(); read_results(); }
}

}  // namespace
}  // namespace pcogfx

using namespace pcogfx;

extern "C" enum PcoError pco_gfx_decompress_page_reads(size_t n_tasks, const PcoGfxPageReadTask* tasks, PcoGfxTaskResult* results,
                                                       PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    // every argument is checked before anything is launched (and before a device is asked for)
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: results and d_results are both null"};
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageReadTask& t = tasks[i];
      const std::string who = "page read task " + std::to_string(i);
      if (t.format_major > 4) throw HostError{PCO_GFX_CORRUPTION, who + ": the file's format version definitely cannot be decompressed"};   // wrapped/file_decompressor.rs:31-36
      if (t.meta == nullptr || t.page == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null ChunkMeta or page"};
      if (width_group(t.dtype) < 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
      if (t.page_n == 0 || t.page_n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a page holds 1 ..= 2^24 numbers"};
      if (t.first > t.page_n || t.count > t.page_n - t.first) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": rows beyond the page"};
      if (t.count > 0 && t.dst == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null dst"};
    }
    if (n_tasks == 0) return PcoSuccess;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_decode_reads(n_tasks, tasks, results, d_results, (hipStream_t)stream); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "page read task " + std::to_string(i) + " failed");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}
