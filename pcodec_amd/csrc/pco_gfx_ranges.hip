// pco_gfx_ranges.hip -- the entry points that decode PART of a wrapped page: pco_gfx_decompress_page_ranges (include/pco_gfx.h section 4d), its
// device-directory form pco_gfx_decompress_page_ranges_dir (4e), pco_gfx_decompress_page_reads (4f) and pco_gfx_index_pages (4g), which walks a
// prefix for its cursors alone.  A translation unit of its own, so that the kernels the whole-page entry points launch (pco_gfx.hip) are compiled
// exactly as before.  The kernels are in decode_range.hip, decode_resume.hip, decode_index.hip and dir_resolve.hip; the host side is ONE driver,
// launch_partial<kForm>, whose form parameter supplies what a read or an index does differently from a range.  A read or an index call flagged
// PCO_GFX_CURSOR_GENERAL (the _ex entry points) runs the kernels of decode_general.hip on the scratch route in place of the prefix kernel.
// pco_gfx_decompress_page_reads_hist (4i) and pco_gfx_index_pages_hist (4j) are the same driver with a history reference per task, and
// pco_gfx_decompress_page_reads_dir / pco_gfx_index_pages_dir (4k) those two behind 4e's device directory.  pco_gfx_scan_chunks (4m), which finds a
// standalone file's chunk directory with the kernel of scan.hip, has a small driver of its own at the end.
#include "pco_host.h"
#include "pco_half.h"

#include <cstring>
#include <string>
#include <vector>

#include "decode_resume.hip"   // (and, through it, decode_range.hip)
#include "decode_index.hip"
#include "decode_general.hip"
#include "dir_resolve.hip"
#include "scan.hip"       // pco_gfx_scan_chunks (section 4m): its driver is at the end of this file
#include "pco_launch.h"   // the timed launch, the LDS reservation, width_group / launch_width / flatten_groups, Layout, the scratch budget

static_assert(sizeof(PcoGfxPageCursor) == 8 * pcogfx::kCursorWords, "PcoGfxPageCursor");
static_assert(sizeof(PcoGfxPageRangeTask) == 72 && sizeof(PcoGfxPageReadTask) == 88, "PcoGfxPageReadTask: PcoGfxPageRangeTask, then the two cursors");
static_assert(sizeof(PcoGfxPageIndexTask) == 64, "PcoGfxPageIndexTask");
static_assert(sizeof(PcoGfxPageIndexHistTask) == 80, "PcoGfxPageIndexHistTask: PcoGfxPageIndexTask, then the histories");
static_assert(sizeof(PcoGfxPageReadHistTask) == 104 && PCO_GFX_HISTORY_HEADER_BYTES == pcogfx::kHistoryHeaderBytes, "PcoGfxPageReadHistTask: PcoGfxPageReadTask, then the history");

namespace pcogfx {

namespace {

constexpr uint32_t kPartialDecodeLdsBytes = 16 * 1024;   // the single-kernel decoder's dynamic LDS (fixed area + tANS tables), as in launch_decode
constexpr size_t kPartialGeneralGrid = 4096;             // ... and its grid bound: each block owns kTblWsBytes of table scratch

// what the scratch of one synchronous pass may take: PCO_GFX_WORKSPACE_GB, default 80 % of the free device memory (plus what the buffer holds).
// Read at every call: a test narrows it in mid-process.
size_t partial_budget_bytes(const Workspace& ws) { return scratch_budget_bytes(std::getenv("PCO_GFX_WORKSPACE_GB"), ws.dec_hist.cap); }

constexpr int kFormRange = 0, kFormResume = 1, kFormIndex = 2;   // launch_partial's forms

// the names pco_gfx_profile_* reports: [form][width group]
const char* const kFastNames[3][4][3] = {{{"dec_walk_range_kernel<u64>", "dec_walk4_range_kernel<u64>", "dec_expand_range_kernel<u64>"},
                                          {"dec_walk_range_kernel<u32>", "dec_walk4_range_kernel<u32>", "dec_expand_range_kernel<u32>"},
                                          {"dec_walk_range_kernel<u16>", "dec_walk4_range_kernel<u16>", "dec_expand_range_kernel<u16>"},
                                          {"dec_walk_range_kernel<u8>", "dec_walk4_range_kernel<u8>", "dec_expand_range_kernel<u8>"}},
                                         {{"dec_walk_resume_kernel<u64>", "dec_walk4_resume_kernel<u64>", "dec_expand_resume_kernel<u64>"},
                                          {"dec_walk_resume_kernel<u32>", "dec_walk4_resume_kernel<u32>", "dec_expand_resume_kernel<u32>"},
                                          {"dec_walk_resume_kernel<u16>", "dec_walk4_resume_kernel<u16>", "dec_expand_resume_kernel<u16>"},
                                          {"dec_walk_resume_kernel<u8>", "dec_walk4_resume_kernel<u8>", "dec_expand_resume_kernel<u8>"}},
                                         {{"dec_walk_index_kernel<u64>", "dec_walk4_index_kernel<u64>", "dec_expand_index_kernel<u64>"},
                                          {"dec_walk_index_kernel<u32>", "dec_walk4_index_kernel<u32>", "dec_expand_index_kernel<u32>"},
                                          {"dec_walk_index_kernel<u16>", "dec_walk4_index_kernel<u16>", "dec_expand_index_kernel<u16>"},
                                          {"dec_walk_index_kernel<u8>", "dec_walk4_index_kernel<u8>", "dec_expand_index_kernel<u8>"}}};
const char* const kScratchNames[4][2] = {{"pco_decode_prefix_kernel<u64>", "range_copy_kernel<u64>"}, {"pco_decode_prefix_kernel<u32>", "range_copy_kernel<u32>"},
                                         {"pco_decode_prefix_kernel<u16>", "range_copy_kernel<u16>"}, {"pco_decode_prefix_kernel<u8>", "range_copy_kernel<u8>"}};

const char* const kGeneralNames[4][2] = {{"pco_decode_general_resume_kernel<u64>", "pco_decode_general_index_kernel<u64>"},
                                         {"pco_decode_general_resume_kernel<u32>", "pco_decode_general_index_kernel<u32>"},
                                         {"pco_decode_general_resume_kernel<u16>", "pco_decode_general_index_kernel<u16>"},
                                         {"pco_decode_general_resume_kernel<u8>", "pco_decode_general_index_kernel<u8>"}};
const char* const kIndexHistNames[4][2] = {{"pco_decode_general_index_hist_kernel<u64>", "index_history_snapshot_kernel<u64>"},
                                           {"pco_decode_general_index_hist_kernel<u32>", "index_history_snapshot_kernel<u32>"},
                                           {"pco_decode_general_index_hist_kernel<u16>", "index_history_snapshot_kernel<u16>"},
                                           {"pco_decode_general_index_hist_kernel<u8>", "index_history_snapshot_kernel<u8>"}};

// What a call flagged PCO_GFX_CURSOR_GENERAL adds to its scratch route.  form: kFormResume or kFormIndex.  A read call: the tasks' own cursor references
// (the two-kernel route got shadows), their records, where the general kernel says which rows of the scratch are the task's, and -- synchronous
// calls only, else null -- the rows the kind-3 `from` cursors stand at, for the scratch's size.  An index call: the cursor references and the plans.
// A call of pco_gfx_decompress_page_reads_hist (section 4i) besides: the tasks' history references on the device and the call's flag -- d_hrefs == nullptr is
// every other call, whose kernels and arguments are what they were.
// A call of pco_gfx_index_pages_hist (section 4j): the tasks' history references and the records its walk leaves the snapshot kernel, and that kernel's
// grid.x -- d_ihrefs == nullptr is every other index call.
struct GeneralCall { int form; const ReadRef* d_refs; ReadRec* d_recs; RangeRef* d_rel_ranges; const uint64_t* rows; const IndexRef* d_irefs; DecPlan* d_plans;
                     const HistRef* d_hrefs = nullptr; uint32_t allow_general = 1;
                     const IndexHistRef* d_ihrefs = nullptr; IndexHistRec* d_ihrecs = nullptr; uint32_t snap_grid = 1; };

// Route 1 over one width group: the 8-chunk walker, the 4-chunk walker over what that one handed back, the expander.  The form chooses the kernels;
// the resume ones take `rz` behind the range ones' arguments, the index ones `ix`.
template <int kForm>
struct FastStep {
  const char* const* names; hipStream_t stream; uint32_t cnt, grid; const PcoGfxDecodeTask* d_tasks; const uint32_t* idp; DecPlan* d_plans; uint8_t* d_bins;
  uint8_t* d_sym; uint64_t sym_stride; uint64_t* d_offpos; uint64_t offpos_stride; PcoGfxTaskResult* d_results; const MetaRef* d_metas; const RangeRef* d_ranges;
  ResumeArgs rz; IndexArgs ix;

  template <class L>
  void launch() const {
    if constexpr (kForm == kFormIndex) run<L>("dec_walk_index_kernel", dec_walk_index_kernel<L, 8>, dec_walk_index_kernel<L, 4>, dec_expand_index_kernel<L>, ix);
    else if constexpr (kForm == kFormResume) run<L>("dec_walk_resume_kernel", dec_walk_resume_kernel<L, 8>, dec_walk_resume_kernel<L, 4>, dec_expand_resume_kernel<L>, rz);
    else run<L>("dec_walk_range_kernel", dec_walk_range_kernel<L, 8>, dec_walk_range_kernel<L, 4>, dec_expand_range_kernel<L>);
  }
  template <class L, class Walk, class Expand, class... Tail>
  void run(const char* walk_name, Walk* walk8, Walk* walk4, Expand* expand, Tail... tail) const {
    PCO_RESERVE_LDS(walk8, 4 * WalkCfg<8>::kWalkLdsBytes, walk_name);
    PCO_RESERVE_LDS(walk4, 4 * WalkCfg<4>::kWalkLdsBytes, walk_name);
    const uint32_t n_wb = (cnt + 7) / 8;
    PCO_TIMED_LAUNCH(names[0], stream, walk8, dim3((n_wb + 3) / 4), dim3(256), 4 * WalkCfg<8>::kWalkLdsBytes, stream,
                     d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, 0u, d_results, d_metas, d_ranges, tail...);
    PCO_TIMED_LAUNCH(names[1], stream, walk4, dim3((cnt + 15) / 16), dim3(256), 4 * WalkCfg<4>::kWalkLdsBytes, stream,
                     d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, kStatusRetryK4, d_results, d_metas, d_ranges, tail...);
    PCO_TIMED_LAUNCH(names[2], stream, expand, dim3(grid), dim3(256), kExpLdsBytes, stream,
                     d_tasks, d_results, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_ranges, tail...);
  }
};

// Route 2 over one width group: the tasks' prefixes into scratch, their rows out of it.  The same two kernels in every form; an index call, which
// wants the verdict and no rows, has copy_slices == 0 and leaves the second out.
struct ScratchStep {
  const char* const* names; hipStream_t stream; uint32_t cnt, grid, copy_slices; const PcoGfxDecodeTask* d_tasks; PcoGfxTaskResult* d_results; const uint32_t* idp; uint8_t* tbl;
  const uint32_t* filt; uint32_t fstride; uint8_t* d_scratch; const uint64_t* d_off; uint8_t* d_hist; uint32_t need_hist; const MetaRef* d_metas; const RangeRef* d_ranges;
  const GeneralCall* gen = nullptr; const char* const* gen_names = nullptr; const uint32_t* d_wcap = nullptr;   // a flagged call: the general kernels in the prefix kernel's place
  const char* const* ihist_names = nullptr;

  template <class L>
  void launch() const {
    if (gen && gen->form == kFormIndex && gen->d_ihrefs) {   // the index kernel compiled with kHist, then the rings out of the scratch it left
      const IndexHistArgs ha{gen->d_ihrefs, gen->d_ihrecs, d_wcap, gen->allow_general};
      PCO_TIMED_LAUNCH(ihist_names[0], stream, pco_decode_general_index_hist_kernel<L>, dim3(grid), dim3(64), kPartialDecodeLdsBytes, stream, d_tasks, d_results, idp, cnt,
                       kPartialDecodeLdsBytes - kLdsFixed, tbl, filt, fstride, kStatusRetryLegacy, d_scratch, d_off, d_hist, need_hist, d_metas, d_ranges, IndexArgs{gen->d_irefs}, gen->d_plans, ha);
      PCO_TIMED_LAUNCH(ihist_names[1], stream, index_history_snapshot_kernel<L>, dim3(gen->snap_grid, std::min<uint32_t>(cnt, 1024u)), dim3(256), 0, stream, d_tasks,
                       (const PcoGfxTaskResult*)d_results, idp, cnt, (const uint8_t*)d_scratch, d_off, gen->d_irefs, ha);
      return;
    }
    if (gen && gen->form == kFormIndex) {
      PCO_TIMED_LAUNCH(gen_names[1], stream, pco_decode_general_index_kernel<L>, dim3(grid), dim3(64), kPartialDecodeLdsBytes, stream, d_tasks, d_results, idp, cnt,
                       kPartialDecodeLdsBytes - kLdsFixed, tbl, filt, fstride, kStatusRetryLegacy, d_scratch, d_off, d_hist, need_hist, d_metas, d_ranges, IndexArgs{gen->d_irefs}, gen->d_plans);
      return;   // (an index call copies no rows)
    }
    if (gen && gen->d_hrefs) {   // the same kernel compiled with kHist: it takes the tasks' histories and the call's flag behind the other's arguments
      PCO_TIMED_LAUNCH(gen_names[0], stream, (pco_decode_general_resume_kernel<L, true>), dim3(grid), dim3(64), kPartialDecodeLdsBytes, stream, d_tasks, d_results, idp, cnt,
                       kPartialDecodeLdsBytes - kLdsFixed, tbl, filt, fstride, kStatusRetryLegacy, d_scratch, d_off, d_hist, need_hist, d_metas, d_ranges,
                       GeneralResumeArgs{gen->d_refs, gen->d_recs, d_wcap, gen->d_rel_ranges}, HistArgs{gen->d_hrefs, gen->allow_general});
      PCO_TIMED_LAUNCH(names[1], stream, range_copy_kernel<L>, dim3(std::min<uint32_t>(cnt, 16384u), copy_slices), dim3(256), 0, stream, d_tasks,
                       (const PcoGfxTaskResult*)d_results, idp, cnt, filt, fstride, kStatusRetryLegacy, (const uint8_t*)d_scratch, d_off, (const RangeRef*)gen->d_rel_ranges);
      return;
    }
    if (gen) {
      PCO_TIMED_LAUNCH(gen_names[0], stream, pco_decode_general_resume_kernel<L>, dim3(grid), dim3(64), kPartialDecodeLdsBytes, stream, d_tasks, d_results, idp, cnt,
                       kPartialDecodeLdsBytes - kLdsFixed, tbl, filt, fstride, kStatusRetryLegacy, d_scratch, d_off, d_hist, need_hist, d_metas, d_ranges,
                       GeneralResumeArgs{gen->d_refs, gen->d_recs, d_wcap, gen->d_rel_ranges});
      PCO_TIMED_LAUNCH(names[1], stream, range_copy_kernel<L>, dim3(std::min<uint32_t>(cnt, 16384u), copy_slices), dim3(256), 0, stream, d_tasks,
                       (const PcoGfxTaskResult*)d_results, idp, cnt, filt, fstride, kStatusRetryLegacy, (const uint8_t*)d_scratch, d_off, (const RangeRef*)gen->d_rel_ranges);
      return;
    }
    PCO_TIMED_LAUNCH(names[0], stream, pco_decode_prefix_kernel<L>, dim3(grid), dim3(64), kPartialDecodeLdsBytes, stream, d_tasks, d_results, idp, cnt,
                     kPartialDecodeLdsBytes - kLdsFixed, tbl, filt, fstride, kStatusRetryLegacy, d_scratch, d_off, d_hist, need_hist, d_metas, d_ranges);
    if (copy_slices == 0) return;
    PCO_TIMED_LAUNCH(names[1], stream, range_copy_kernel<L>, dim3(std::min<uint32_t>(cnt, 16384u), copy_slices), dim3(256), 0, stream, d_tasks,
                     (const PcoGfxTaskResult*)d_results, idp, cnt, filt, fstride, kStatusRetryLegacy, (const uint8_t*)d_scratch, d_off, d_ranges);
  }
};

// what the scratch passes of one call share
struct PartialCall {
  Workspace& ws; const PcoGfxPageRangeTask* tasks; size_t n_tasks; hipStream_t stream; const PcoGfxDecodeTask* d_tasks; PcoGfxTaskResult* d_results; const MetaRef* d_metas;
  const RangeRef* d_ranges; uint32_t copy_slices; const GeneralCall* gen;
};

// (a flagged read) the batch a task's walk starts at, as far as the host knows: the batch of its kind-3 `from` cursor in a synchronous call, else 0
uint64_t start_batch(const PartialCall& c, size_t i) { return c.gen && c.gen->rows ? std::min<uint64_t>(c.gen->rows[i] >> 8, c.tasks[i].first >> 8) : 0; }
// the scratch a task takes on route 2: the batches it walks and one more, or what the page has from there
uint64_t scratch_bytes(const PartialCall& c, size_t i) {
  const PcoGfxPageRangeTask& t = c.tasks[i];
  const uint64_t b0 = start_batch(c, i);
  const uint64_t numbers = std::min<uint64_t>((range_end_batch(t.first, t.count) - b0 + 1) * kBatchN, t.page_n - b0 * kBatchN);   // (b0 == 0: range_scratch_numbers)
  return (numbers * (uint64_t)(dtype_bits(t.dtype) / 8) + 255) & ~(uint64_t)255;
}

// Route 2 over the tasks `list` (task ids grouped by width, group g at [goff[g], goff[g + 1])): their prefixes into scratch, their ranges out of it.
// filt: run over every task of the call and let the device pick the ones the walkers handed back (the asynchronous form).
void run_scratch(const PartialCall& c, const std::vector<uint32_t>& list, const size_t (&goff)[5], bool with_hist, const uint32_t* filt, uint32_t need_hist) {
  std::vector<uint64_t> offs(list.size()); uint64_t bytes = 0;
  std::vector<uint32_t> wcap(c.gen ? list.size() : 0);   // (a flagged call) the batches of scratch each task has from its start batch
  for (size_t k = 0; k < list.size(); k++) {
    offs[k] = bytes;
    const PcoGfxPageRangeTask& t = c.tasks[list[k]];
    if (t.count) bytes += scratch_bytes(c, list[k]);
    if (c.gen) wcap[k] = t.count ? (uint32_t)(range_end_batch(t.first, t.count) - start_batch(c, list[k])) : 0u;
  }
  const uint64_t hist_at = (bytes + 255) & ~(uint64_t)255, tail_at = hist_at + (with_hist ? hist_at : 0);
  uint8_t* d_scratch = (uint8_t*)c.ws.dec_hist.ensure(tail_at + list.size() * 16 + 256);
  uint64_t* d_off = (uint64_t*)(d_scratch + tail_at);
  uint32_t* d_list = (uint32_t*)(d_off + list.size());
  uint32_t* d_wcap = d_list + list.size();
  PCO_HIP_CHECK(hipMemcpyAsync(d_off, offs.data(), list.size() * 8, hipMemcpyHostToDevice, c.stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, c.stream));
  if (c.gen && !list.empty()) PCO_HIP_CHECK(hipMemcpyAsync(d_wcap, wcap.data(), list.size() * 4, hipMemcpyHostToDevice, c.stream));
  size_t max_grid = 0;
  for (int g = 0; g < 4; g++) max_grid = std::max(max_grid, std::min<size_t>(goff[g + 1] - goff[g], kPartialGeneralGrid));
  uint8_t* tbl = (uint8_t*)c.ws.tbl_ws.ensure(max_grid * kTblWsBytes);
  for (int g = 0; g < 4; g++) {
    const uint32_t cnt = (uint32_t)(goff[g + 1] - goff[g]);
    if (!cnt) continue;
    launch_width(g, ScratchStep{kScratchNames[g], c.stream, cnt, (uint32_t)std::min<size_t>(cnt, kPartialGeneralGrid), c.copy_slices, c.d_tasks, c.d_results, d_list + goff[g], tbl,
                                filt, (uint32_t)(sizeof(DecPlan) / 4), d_scratch, d_off + goff[g], with_hist ? d_scratch + hist_at : nullptr, need_hist, c.d_metas, c.d_ranges,
                                c.gen, kGeneralNames[g], d_wcap + goff[g], kIndexHistNames[g]});
    PCO_HIP_CHECK(hipGetLastError());
  }
}

void read_results(const PartialCall& c, PcoGfxTaskResult* results) {
  PCO_HIP_CHECK(hipMemcpyAsync(results, c.d_results, c.n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, c.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(c.stream));
}

// The driver of all four entry points.  kFormResume: the tasks are reads -- `cursors` holds their from / to, route 1 runs the resume kernels from the
// `from` cursors, and a finishing kernel writes the `to` cursors of route 2; else `cursors` is null.  kFormIndex: the tasks are the ranges
// {first 0, count k * every_rows} without a dst and `index` says where their cursors go -- route 1 runs the index kernels over that range, route 2
// gets the range {0, 1} (two batches of scratch, the verdict and no copy), and a finishing kernel writes its position-only cursors.
// dir (the _dir entry points, or nullptr): the tasks' meta / page are null, and dir_resolve_kernel -- for reads dir_resolve_reads_kernel -- fills the
// device tasks' sources and ChunkMeta references from the directory and dir->pieces (dir_resolve.hip).  An index task's device range is
// {0, k * every_rows}, so the kernel's "count == 0 takes no verdict" is the k == 0 of an index task.
// flags (reads and index calls): PCO_GFX_CURSOR_GENERAL -- the scratch route runs the kernels of decode_general.hip, which take and leave kind-3 cursors
// on the pages without Lookback; a read call's two-kernel route gets shadows of the kind-3 `from` cursors (reads_shadow_kernel).  0: nothing differs.
// hist (reads only, or nullptr): pco_gfx_decompress_page_reads_hist -- one history reference per task.  The scratch route runs the general resume kernel
// compiled with kHist whatever the flags are (without the flag it keeps the pages without Lookback on position-only cursors), and the shadows are
// reads_shadow_hist_kernel's: of kind-3 cursors under the flag, of kind-4 cursors for the tasks with a history.
// ihist (index calls only, or nullptr): pco_gfx_index_pages_hist -- one IndexHistRef per task.  The scratch route runs the general index kernel compiled with
// kHist whatever the flags are, then index_history_snapshot_kernel.  A task with histories may walk its whole prefix into scratch, and only the device
// knows which do: an asynchronous call gives every such task that scratch up front; a synchronous one gives two batches as ever, gets the tasks that
// need more back with the status a second history buffer is asked for with, and runs them in the passes of that round.
template <int kForm>
void launch_partial(size_t n_tasks, const PcoGfxPageRangeTask* tasks, const ReadRef* cursors, const IndexRef* index, const DirLaunch* dir, uint32_t flags,
                    PcoGfxTaskResult* results, PcoGfxTaskResult* d_results_user, hipStream_t stream, const HistRef* hist = nullptr, const IndexHistRef* ihist = nullptr) {
  constexpr bool kResume = kForm == kFormResume, kIndex = kForm == kFormIndex;
  const uint32_t allow_general = (flags & PCO_GFX_CURSOR_GENERAL) != 0 ? 1u : 0u;
  const bool general = kForm != kFormRange && (allow_general || (kResume && hist != nullptr) || (kIndex && ihist != nullptr));
  const std::string form = kIndex ? "page index: " : (kResume ? "page reads: " : "page ranges: ");
  if (n_tasks == 0) return;
  if (n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, form + "too many tasks"};
  Workspace& ws = workspace();
  std::vector<PcoGfxDecodeTask> dt(n_tasks); std::vector<MetaRef> refs(n_tasks); std::vector<RangeRef> rr(n_tasks);
  std::vector<PcoGfxPageRangeTask> first_row(kIndex ? n_tasks : 0); std::vector<RangeRef> rr1(kIndex ? n_tasks : 0);   // (an index call) what route 2 decodes
  std::vector<PcoGfxPageRangeTask> prefix_row(kIndex && ihist ? n_tasks : 0);   // ... and what its scratch is sized by where a task with histories gets its whole prefix
  uint64_t snap_grid = 1;
  std::vector<uint32_t> flat; size_t id_off[5] = {0, 0, 0, 0, 0};
  uint64_t max_count = 0; bool any_from = false;
  {
    std::vector<uint32_t> ids[4];
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageRangeTask& t = tasks[i];
      dt[i] = PcoGfxDecodeTask{t.page, t.page_len, t.dst, t.page_n, t.dtype, PCO_GFX_TASK_WRAPPED_PAGE | (t.format_major << 8)};
      refs[i] = MetaRef{t.meta, t.meta_len}; rr[i] = RangeRef{t.first, t.count};
      if constexpr (kResume) any_from = any_from || (cursors[i].from != nullptr && t.count != 0);
      if constexpr (kIndex) { first_row[i] = t; first_row[i].count = t.count ? 1 : 0; rr1[i] = RangeRef{0, first_row[i].count}; }
      if (kIndex && ihist) {
        prefix_row[i] = ihist[i].histories && t.count ? t : first_row[i];
        if (!results) first_row[i] = prefix_row[i];   // (the device ranges stay {0, 1}: the kernel sizes a snapshot walk by the index reference and its scratch's cap)
        if (ihist[i].histories && t.count)   // (cursor, stretch) pairs of the longest history this task can have
          snap_grid = std::max<uint64_t>(snap_grid, (t.count / index[i].every_batches / kBatchN) * ((std::min<uint64_t>(t.count + kBatchN, t.page_n) + 8 + kSnapRows - 1) / kSnapRows));
      }
      ids[width_group(t.dtype)].push_back((uint32_t)i);
      max_count = std::max<uint64_t>(max_count, t.count);
    }
    flatten_groups(ids, flat, id_off);
  }
  // device arrays: tasks | ids (grouped by number width) | ChunkMeta references | ranges, then a read call's cursor references | per-task records |
  // cursor rows, or a directory call's piece pairs, or an index call's cursor references | route 2's ranges
  Layout at;
  const size_t tasks_off = at.place(n_tasks * sizeof(PcoGfxDecodeTask)), ids_off = at.place(n_tasks * sizeof(uint32_t)), metas_off = at.place(n_tasks * sizeof(MetaRef));
  const size_t ranges_off = at.place(n_tasks * sizeof(RangeRef));
  const size_t curs_off = kResume ? at.place(n_tasks * sizeof(ReadRef)) : 0, recs_off = kResume ? at.place(n_tasks * sizeof(ReadRec)) : 0;
  const size_t rows_off = kResume ? at.place(n_tasks * sizeof(uint64_t)) : 0, pieces_off = dir ? at.place(n_tasks * sizeof(DirPieces)) : 0;
  const size_t bad_meta_off = dir && dir->chunks ? at.place(16) : 0;   // (a chunk directory call: the one-byte ChunkMeta of a refusal by Corruption, dir_resolve.hip)
  const size_t irefs_off = kIndex ? at.place(n_tasks * sizeof(IndexRef)) : 0, ranges1_off = kIndex ? at.place(n_tasks * sizeof(RangeRef)) : 0;
  // (a flagged read call) the two-kernel route's cursor references | the shadows of the kind-3 `from` cursors | their rows | the rows' places in the scratch
  const bool shadows = kResume && general;
  const size_t srefs_off = shadows ? at.place(n_tasks * sizeof(ReadRef)) : 0, swords_off = shadows ? at.place(n_tasks * sizeof(PcoGfxPageCursor)) : 0;
  const size_t grows_off = shadows ? at.place(n_tasks * sizeof(uint64_t)) : 0, rel_off = shadows ? at.place(n_tasks * sizeof(RangeRef)) : 0;
  const size_t hrefs_off = hist ? at.place(n_tasks * sizeof(HistRef)) : 0;   // (a call with histories) the tasks' history references
  const size_t ihrefs_off = ihist ? at.place(n_tasks * sizeof(IndexHistRef)) : 0, ihrecs_off = ihist ? at.place(n_tasks * sizeof(IndexHistRec)) : 0;
  uint8_t* d_base = (uint8_t*)ws.tasks.ensure(at.end + 64);
  const PcoGfxDecodeTask* d_tasks = (const PcoGfxDecodeTask*)(d_base + tasks_off);
  const uint32_t* d_ids = (const uint32_t*)(d_base + ids_off);
  const MetaRef* d_metas = (const MetaRef*)(d_base + metas_off);
  const RangeRef* d_ranges = (const RangeRef*)(d_base + ranges_off);
  const ReadRef* d_curs = (const ReadRef*)(d_base + curs_off);   // (a read call's three)
  ReadRec* d_recs = (ReadRec*)(d_base + recs_off);
  uint64_t* d_rows = (uint64_t*)(d_base + rows_off);
  const IndexRef* d_irefs = (const IndexRef*)(d_base + irefs_off);   // (an index call's two)
  const RangeRef* d_ranges1 = (const RangeRef*)(d_base + ranges1_off);
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + tasks_off, dt.data(), n_tasks * sizeof(PcoGfxDecodeTask), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + ids_off, flat.data(), n_tasks * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + metas_off, refs.data(), n_tasks * sizeof(MetaRef), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_base + ranges_off, rr.data(), n_tasks * sizeof(RangeRef), hipMemcpyHostToDevice, stream));
  if constexpr (kResume) PCO_HIP_CHECK(hipMemcpyAsync(d_base + curs_off, cursors, n_tasks * sizeof(ReadRef), hipMemcpyHostToDevice, stream));
  if (hist) PCO_HIP_CHECK(hipMemcpyAsync(d_base + hrefs_off, hist, n_tasks * sizeof(HistRef), hipMemcpyHostToDevice, stream));
  if (ihist) {
    PCO_HIP_CHECK(hipMemcpyAsync(d_base + ihrefs_off, ihist, n_tasks * sizeof(IndexHistRef), hipMemcpyHostToDevice, stream));
    PCO_HIP_CHECK(hipMemsetAsync(d_base + ihrecs_off, 0, n_tasks * sizeof(IndexHistRec), stream));
  }
  if constexpr (kIndex) {
    PCO_HIP_CHECK(hipMemcpyAsync(d_base + irefs_off, index, n_tasks * sizeof(IndexRef), hipMemcpyHostToDevice, stream));
    PCO_HIP_CHECK(hipMemcpyAsync(d_base + ranges1_off, rr1.data(), n_tasks * sizeof(RangeRef), hipMemcpyHostToDevice, stream));
  }
  if (dir) {
    PCO_HIP_CHECK(hipMemcpyAsync(d_base + pieces_off, dir->pieces, n_tasks * sizeof(DirPieces), hipMemcpyHostToDevice, stream));
    if (dir->chunks) {   // (section 4l: the pieces are standalone chunks)
      if constexpr (kResume)
        PCO_TIMED_LAUNCH("dir_resolve_chunks_reads_kernel", stream, dir_resolve_chunks_reads_kernel<true>, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream,
                         (PcoGfxDecodeTask*)(d_base + tasks_off), (MetaRef*)(d_base + metas_off), (const DirPieces*)(d_base + pieces_off), d_ranges, (uint32_t)n_tasks, dir->args,
                         d_base + bad_meta_off, (DirCursorPair*)(d_base + curs_off));
      else
        PCO_TIMED_LAUNCH("dir_resolve_chunks_kernel", stream, dir_resolve_chunks_kernel<true>, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream,
                         (PcoGfxDecodeTask*)(d_base + tasks_off), (MetaRef*)(d_base + metas_off), (const DirPieces*)(d_base + pieces_off), d_ranges, (uint32_t)n_tasks, dir->args,
                         d_base + bad_meta_off);
    } else if constexpr (kResume)   // (a refused read task loses the device copy of its cursor pair as well: dir_resolve.hip)
      PCO_TIMED_LAUNCH("dir_resolve_reads_kernel", stream, dir_resolve_reads_kernel<true>, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, (PcoGfxDecodeTask*)(d_base + tasks_off),
                       (MetaRef*)(d_base + metas_off), (const DirPieces*)(d_base + pieces_off), d_ranges, (uint32_t)n_tasks, dir->args, (DirCursorPair*)(d_base + curs_off));
    else
      PCO_TIMED_LAUNCH("dir_resolve_kernel", stream, dir_resolve_kernel<true>, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, (PcoGfxDecodeTask*)(d_base + tasks_off),
                       (MetaRef*)(d_base + metas_off), (const DirPieces*)(d_base + pieces_off), d_ranges, (uint32_t)n_tasks, dir->args);
    PCO_HIP_CHECK(hipGetLastError());
  }
  // symbols and section starts: sized by the most batches a task of the call WALKS, not by its longest page.  A range walks its PREFIX, batches
  // [0, ceil((first + count) / 256)).  A read walks from batch at / 256, and `at` lives in the `from` cursor on the device: a synchronous call reads
  // the rows back; an asynchronous one cannot, and sizes by the end batch as a range call does.
  std::vector<uint64_t> rows(kResume ? n_tasks : 0, 0), grows(shadows ? n_tasks : 0, 0);
  if (shadows) {
    if (hist)
      PCO_TIMED_LAUNCH("reads_shadow_hist_kernel", stream, reads_shadow_hist_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_curs, d_ranges,
                       (const HistRef*)(d_base + hrefs_off), allow_general, (uint32_t)n_tasks, (ReadRef*)(d_base + srefs_off), (uint64_t*)(d_base + swords_off), d_rows,
                       (uint64_t*)(d_base + grows_off));
    else
      PCO_TIMED_LAUNCH("reads_shadow_kernel", stream, reads_shadow_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_curs, d_ranges, (uint32_t)n_tasks,
                       (ReadRef*)(d_base + srefs_off), (uint64_t*)(d_base + swords_off), d_rows, (uint64_t*)(d_base + grows_off));
    PCO_HIP_CHECK(hipGetLastError());
    if (results && any_from) {
      PCO_HIP_CHECK(hipMemcpyAsync(rows.data(), d_rows, n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipMemcpyAsync(grows.data(), d_base + grows_off, n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipStreamSynchronize(stream));
    }
  } else if (kResume && results && any_from) {
    PCO_TIMED_LAUNCH("reads_rows_kernel", stream, reads_rows_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_curs, (uint32_t)n_tasks, d_rows);
    PCO_HIP_CHECK(hipMemcpyAsync(rows.data(), d_rows, n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  uint64_t max_walk = 0;
  for (size_t i = 0; i < n_tasks; i++) {
    if (!tasks[i].count) continue;
    const uint64_t b_end = range_end_batch(tasks[i].first, tasks[i].count);
    max_walk = std::max<uint64_t>(max_walk, b_end - (kResume ? std::min<uint64_t>(rows[i] >> 8, b_end - 1) : 0));   // (a cursor behind `first` is refused on the device)
  }
  PcoGfxTaskResult* d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)ws.results.ensure(n_tasks * sizeof(PcoGfxTaskResult));
  const uint64_t sym_stride = max_walk * kBatchN + 256, offpos_stride = sym_stride / 256 + 2;
  if (n_tasks * 3 * sym_stride > ((size_t)48 << 30))
    throw HostError{PCO_GFX_INVALID_ARGUMENT, form + (kResume ? "the batches one call walks" : "the prefixes of one call") + " may take 48 GiB of symbol scratch at most; split the call"};
  DecPlan* d_plans = (DecPlan*)ws.dec_plans.ensure(n_tasks * sizeof(DecPlan));
  {
    uint8_t* d_bins = (uint8_t*)ws.dec_bins.ensure(n_tasks * kBinsAreaPerTask);
    uint8_t* d_sym = (uint8_t*)ws.dec_sym.ensure(n_tasks * 3 * sym_stride + 64);
    uint64_t* d_offpos = (uint64_t*)ws.dec_offpos.ensure(n_tasks * 3 * offpos_stride * 8);
    for (int g = 0; g < 4; g++) {
      const uint32_t cnt = (uint32_t)(id_off[g + 1] - id_off[g]);
      if (!cnt) continue;
      launch_width(g, FastStep<kForm>{kFastNames[kForm][g], stream, cnt, (uint32_t)std::min<size_t>(cnt, kPartialGeneralGrid), d_tasks, d_ids + id_off[g], d_plans, d_bins, d_sym,
                                        sym_stride, d_offpos, offpos_stride, d_results, d_metas, d_ranges,
                                        ResumeArgs{shadows ? (const ReadRef*)(d_base + srefs_off) : d_curs, d_recs, (uint32_t)max_walk}, IndexArgs{d_irefs}});
      PCO_HIP_CHECK(hipGetLastError());
    }
  }
  const GeneralCall gen{kForm, d_curs, d_recs, (RangeRef*)(d_base + rel_off), kResume && results && any_from ? grows.data() : nullptr, d_irefs, d_plans,
                        hist ? (const HistRef*)(d_base + hrefs_off) : nullptr, allow_general,
                        ihist ? (const IndexHistRef*)(d_base + ihrefs_off) : nullptr, ihist ? (IndexHistRec*)(d_base + ihrecs_off) : nullptr,
                        (uint32_t)std::min<uint64_t>(snap_grid, 8192)};
  const PartialCall call{ws, kIndex ? first_row.data() : tasks, n_tasks, stream, d_tasks, d_results, d_metas, kIndex ? d_ranges1 : d_ranges,
                         kIndex ? 0u : (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (max_count + 4095) / 4096)), general ? &gen : nullptr};
  PartialCall pass_call = call;   // the passes of a synchronous call: an index call with histories sizes them by the whole prefixes
  if (kIndex && ihist) pass_call.tasks = prefix_row.data();
  bool scratch_ran = true;
  if (!results || kIndex) {
    // asynchronous: the call cannot come back, so every task takes its prefix scratch up front and the device picks the tasks of route 2 (the history of
    // a delta'd secondary variable under lookback stays the one thing such a call does not have: PCO_GFX_UNSUPPORTED, as in pco_gfx_decompress_pages).
    // An index call does so in both forms: two batches a task need no passes, and its synchronous form comes back for that history alone
    run_scratch(call, flat, id_off, false, (const uint32_t*)d_plans, results ? kStatusNeedHist : (uint32_t)PCO_GFX_UNSUPPORTED);
  }
  if (results) {
    // synchronous: the tasks the walkers handed back go through route 2 in passes whose scratch fits the budget; the ones that then ask for a second
    // history buffer once more, with it
    read_results(call, results);
    scratch_ran = kIndex;
    for (int round = kIndex ? 1 : 0; round < 2; round++) {
      const uint32_t want = round == 0 ? kStatusRetryLegacy : kStatusNeedHist;
      const size_t budget = partial_budget_bytes(ws);
      bool any = false;
      size_t next = 0;
      while (next < n_tasks) {   // (task order: a pass is a stretch of the call's tasks)
        std::vector<uint32_t> ids[4]; uint64_t bytes = 0; size_t taken = 0;
        for (; next < n_tasks; next++) {
          if (results[next].status != want) continue;
          const uint64_t b = scratch_bytes(pass_call, next) * (round ? 2 : 1);
          if (taken && bytes + b > budget) break;
          ids[width_group(pass_call.tasks[next].dtype)].push_back((uint32_t)next); bytes += b; taken++;
        }
        if (!taken) break;
        std::vector<uint32_t> list; size_t goff[5];
        flatten_groups(ids, list, goff);
        run_scratch(pass_call, list, goff, round == 1, nullptr, round == 0 ? kStatusNeedHist : (uint32_t)PCO_GFX_UNSUPPORTED);
        PCO_HIP_CHECK(hipStreamSynchronize(stream));   // (the next pass writes the same scratch, and may move it)
        any = true;
      }
      if (!any) break;
      scratch_ran = true;
      read_results(call, results);
    }
  }
  if constexpr (kResume) {
    if (!scratch_ran) return;
    // the position-only `to` cursors of route 2; a synchronous call then reads its results once more
    PCO_TIMED_LAUNCH("reads_finish_kernel", stream, reads_finish_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_tasks, d_ranges, d_curs,
                     (const ReadRec*)d_recs, d_results, (uint32_t)n_tasks);
    PCO_HIP_CHECK(hipGetLastError());
    if (results) read_results(call, results);
  }
  if constexpr (kIndex) {
    if (!scratch_ran) return;
    // the position-only cursors of route 2 and their tasks' results; a synchronous call then reads its results once more
    PCO_TIMED_LAUNCH("index_finish_kernel", stream, index_finish_kernel, dim3((uint32_t)std::min<size_t>(n_tasks, 65535)), dim3(256), 0, stream, d_tasks, (const DecPlan*)d_plans, d_irefs,
                     d_results, (uint32_t)n_tasks);
    PCO_HIP_CHECK(hipGetLastError());
    if (results) read_results(call, results);
  }
}

// One task's arguments, in the order every entry point checks them.  `t` is the task as the driver takes it; pieces: the directory form's pair,
// checked against n_pieces in place of the meta / page pointers it has not got.
// chunks: the pair names one standalone chunk (section 4l).
void check_partial_task(const std::string& who, const PcoGfxPageRangeTask& t, const DirPieces* pieces = nullptr, uint64_t n_pieces = 0, bool chunks = false) {
  if (t.format_major > 4) throw HostError{PCO_GFX_CORRUPTION, who + ": the file's format version definitely cannot be decompressed"};   // wrapped/file_decompressor.rs:31-36
  if (pieces && chunks) check_chunk_piece(pieces->meta_piece, pieces->page_piece, n_pieces, who);
  else if (pieces) check_piece_pair(pieces->meta_piece, pieces->page_piece, n_pieces, who);
  else if (t.meta == nullptr || t.page == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null ChunkMeta or page"};
  if (width_group(t.dtype) < 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
  if (t.page_n == 0 || t.page_n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a page holds 1 ..= 2^24 numbers"};
  if (t.first > t.page_n || t.count > t.page_n - t.first) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": rows beyond the page"};
  if (t.count > 0 && t.dst == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null dst"};
}

// checked tasks -> the call's return value; what: "page range", "directory page range", "page read", "page index"
template <int kForm>
PcoError run_partial(const char* what, size_t n_tasks, const PcoGfxPageRangeTask* tasks, const ReadRef* cursors, const IndexRef* index, const DirLaunch* dir, uint32_t flags,
                     PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, hipStream_t stream, const HistRef* hist = nullptr, const IndexHistRef* ihist = nullptr) {
  if (n_tasks == 0) return PcoSuccess;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
  { WorkspaceUse use(workspace(), stream); launch_partial<kForm>(n_tasks, tasks, cursors, index, dir, flags, results, d_results, stream, hist, ihist); }
  if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
    set_error((int)results[i].status, std::string(what) + " task " + std::to_string(i) + " failed");
    return PcoDecompressionError;
  }
  return PcoSuccess;
}

}  // namespace
}  // namespace pcogfx

using namespace pcogfx;

// Every argument is checked before anything is launched (and before a device is asked for).

extern "C" enum PcoError pco_gfx_decompress_page_ranges(size_t n_tasks, const PcoGfxPageRangeTask* tasks, PcoGfxTaskResult* results,
                                                        PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page ranges: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page ranges: results and d_results are both null"};
    for (size_t i = 0; i < n_tasks; i++) check_partial_task("page range task " + std::to_string(i), tasks[i]);
    return run_partial<kFormRange>("page range", n_tasks, tasks, nullptr, nullptr, nullptr, 0, results, d_results, (hipStream_t)stream);
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}

// include/pco_gfx.h section 4e.  (It refuses a call without results even when it has no tasks; the pointer forms do not.)
extern "C" enum PcoError pco_gfx_decompress_page_ranges_dir(size_t n_tasks, const PcoGfxDirPageRangeTask* tasks, const PcoGfxDirectory* dir,
                                                            PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page range directory: null task array"};
    DirLaunch dl{checked_directory(dir, "page range"), nullptr};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page range directory: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<DirPieces> pieces(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxDirPageRangeTask& t = tasks[i];
      rt[i] = PcoGfxPageRangeTask{nullptr, 0, nullptr, 0, t.dst, t.page_n, t.first, t.count, t.dtype, t.format_major};
      pieces[i] = DirPieces{t.meta_piece, t.page_piece};
      check_partial_task("directory page range task " + std::to_string(i), rt[i], &pieces[i], dl.args.n_pieces);
    }
    dl.pieces = pieces.data();
    return run_partial<kFormRange>("directory page range", n_tasks, rt.data(), nullptr, nullptr, &dl, 0, results, d_results, (hipStream_t)stream);
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}

// include/pco_gfx.h section 4f: a read task is a range task and its two cursors
extern "C" enum PcoError pco_gfx_decompress_page_reads_ex(size_t n_tasks, const PcoGfxPageReadTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                                          PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: unknown flags"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<ReadRef> cursors(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageReadTask& t = tasks[i];
      rt[i] = PcoGfxPageRangeTask{t.meta, t.meta_len, t.page, t.page_len, t.dst, t.page_n, t.first, t.count, t.dtype, t.format_major};
      cursors[i] = ReadRef{t.from ? t.from->w : nullptr, t.to ? t.to->w : nullptr};
      check_partial_task("page read task " + std::to_string(i), rt[i]);
    }
    return run_partial<kFormResume>("page read", n_tasks, rt.data(), cursors.data(), nullptr, nullptr, flags, results, d_results, (hipStream_t)stream);
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}

extern "C" enum PcoError pco_gfx_decompress_page_reads(size_t n_tasks, const PcoGfxPageReadTask* tasks, PcoGfxTaskResult* results,
                                                       PcoGfxTaskResult* d_results, void* stream) {
  return pco_gfx_decompress_page_reads_ex(n_tasks, tasks, 0, results, d_results, stream);
}

// include/pco_gfx.h section 4i: a read task and its history buffer
extern "C" size_t pco_gfx_lookback_history_bytes(uint32_t window_n_log, unsigned char dtype) {
  return width_group(dtype) < 0 ? 0 : (size_t)history_bytes(window_n_log, (uint32_t)(dtype_bits(dtype) / 8));
}

extern "C" enum PcoError pco_gfx_decompress_page_reads_hist(size_t n_tasks, const PcoGfxPageReadHistTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                                            PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads with histories: unknown flags"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads with histories: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page reads with histories: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<ReadRef> cursors(n_tasks); std::vector<HistRef> hist(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageReadHistTask& t = tasks[i];
      const std::string who = "page read task " + std::to_string(i);
      rt[i] = PcoGfxPageRangeTask{t.meta, t.meta_len, t.page, t.page_len, t.dst, t.page_n, t.first, t.count, t.dtype, t.format_major};
      cursors[i] = ReadRef{t.from ? t.from->w : nullptr, t.to ? t.to->w : nullptr};
      hist[i] = HistRef{t.history, t.history_len};
      check_partial_task(who, rt[i]);
      if ((t.history == nullptr) != (t.history_len == 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a history and its length go together"};
      if (((uintptr_t)t.history & 7u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": misaligned history"};
    }
    return run_partial<kFormResume>("page read", n_tasks, rt.data(), cursors.data(), nullptr, nullptr, flags, results, d_results, (hipStream_t)stream, hist.data());
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}

// include/pco_gfx.h section 4g: an index task is the range task {first 0, count k * every_rows} without a dst, and where its k cursors go
extern "C" size_t pco_gfx_page_index_len(uint64_t page_n, uint64_t every_rows) { return (size_t)index_len(page_n, every_rows); }

extern "C" enum PcoError pco_gfx_index_pages_ex(size_t n_tasks, const PcoGfxPageIndexTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                                PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page index: unknown flags"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page index: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page index: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<IndexRef> index(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageIndexTask& t = tasks[i];
      const std::string who = "page index task " + std::to_string(i);
      rt[i] = PcoGfxPageRangeTask{t.meta, t.meta_len, t.page, t.page_len, nullptr, t.page_n, 0, 0, t.dtype, t.format_major};
      check_partial_task(who, rt[i]);
      if (t.every_rows == 0 || (t.every_rows & 255u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": every_rows is a positive multiple of 256"};
      const uint64_t k = index_len(t.page_n, t.every_rows);
      if (k > 0 && (t.cursors == nullptr || ((uintptr_t)t.cursors & 7u) != 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null or misaligned cursors"};
      rt[i].count = k * t.every_rows;   // (< page_n: the walk never reaches the page's last batch)
      index[i] = IndexRef{k ? t.cursors->w : nullptr, (uint32_t)(k ? t.every_rows >> 8 : 0), (uint32_t)k};
    }
    return run_partial<kFormIndex>("page index", n_tasks, rt.data(), nullptr, index.data(), nullptr, flags, results, d_results, (hipStream_t)stream);
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}

extern "C" enum PcoError pco_gfx_index_pages(size_t n_tasks, const PcoGfxPageIndexTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results,
                                             void* stream) {
  return pco_gfx_index_pages_ex(n_tasks, tasks, 0, results, d_results, stream);
}

// include/pco_gfx.h section 4j: an index task and where its k histories go
extern "C" enum PcoError pco_gfx_index_pages_hist(size_t n_tasks, const PcoGfxPageIndexHistTask* tasks, uint32_t flags, PcoGfxTaskResult* results,
                                                  PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page index with histories: unknown flags"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page index with histories: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page index with histories: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<IndexRef> index(n_tasks); std::vector<IndexHistRef> hist(n_tasks);
    bool any = false;
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageIndexHistTask& t = tasks[i];
      const std::string who = "page index task " + std::to_string(i);
      rt[i] = PcoGfxPageRangeTask{t.meta, t.meta_len, t.page, t.page_len, nullptr, t.page_n, 0, 0, t.dtype, t.format_major};
      check_partial_task(who, rt[i]);
      if (t.every_rows == 0 || (t.every_rows & 255u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": every_rows is a positive multiple of 256"};
      const uint64_t k = index_len(t.page_n, t.every_rows);
      if (k > 0 && (t.cursors == nullptr || ((uintptr_t)t.cursors & 7u) != 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null or misaligned cursors"};
      if ((t.histories == nullptr) != (t.history_stride == 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": histories and their stride go together"};
      if ((t.history_stride & 7u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": the stride is a multiple of 8"};
      if (((uintptr_t)t.histories & 7u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": misaligned histories"};
      rt[i].count = k * t.every_rows;
      index[i] = IndexRef{k ? t.cursors->w : nullptr, (uint32_t)(k ? t.every_rows >> 8 : 0), (uint32_t)k};
      hist[i] = k ? IndexHistRef{t.histories, t.history_stride} : IndexHistRef{nullptr, 0};
      any = any || hist[i].histories != nullptr;
    }
    // (a call without a history is the _ex call: the same kernels, the same arguments)
    return run_partial<kFormIndex>("page index", n_tasks, rt.data(), nullptr, index.data(), nullptr, flags, results, d_results, (hipStream_t)stream, nullptr, any ? hist.data() : nullptr);
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}

// include/pco_gfx.h section 4k: 4i's read entry point and 4j's index entry point with each task's ChunkMeta and page named by piece index.  The host
// checks are check_partial_task's (with the piece pair in place of the pointers) and the _hist entry points', in their order; the directory's
// verdicts are the resolve kernel's (dir_resolve.hip), and everything behind it is the pointer form's call.
static_assert(sizeof(PcoGfxDirPageReadTask) == 80 && sizeof(PcoGfxDirPageIndexTask) == 56, "PcoGfxDirPageReadTask, PcoGfxDirPageIndexTask");
static_assert(sizeof(DirCursorPair) == sizeof(ReadRef) && offsetof(DirCursorPair, to) == offsetof(ReadRef, to), "dir_resolve_reads_kernel writes ReadRef's two words");

extern "C" int pco_gfx_lookback_window_n_log(uint64_t n) {   // delta/mod.rs:37-48, pco_encode_config.inc lookback_window_log
  if (n == 0 || n > kMaxEntries) return 0;
  int b = 0;
  while (((uint64_t)1 << b) < n) b++;   // ceil(log2(n))
  return b < 4 ? 4 : (b > 15 ? 15 : b);
}

// (chunks: section 4l, where each task's one piece is a standalone chunk; else section 4k.  Nothing else differs on the host)
static PcoError reads_dir(bool chunks, size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags, PcoGfxTaskResult* results,
                          PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  const std::string w = chunks ? "chunk" : "page";   // (the messages' word)
  try {
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, w + " read directory: unknown flags"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, w + " read directory: null task array"};
    DirLaunch dl{checked_directory(dir, (w + " read").c_str()), nullptr, chunks};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, w + " read directory: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<DirPieces> pieces(n_tasks); std::vector<ReadRef> cursors(n_tasks); std::vector<HistRef> hist(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxDirPageReadTask& t = tasks[i];
      const std::string who = "directory " + w + " read task " + std::to_string(i);
      rt[i] = PcoGfxPageRangeTask{nullptr, 0, nullptr, 0, t.dst, t.page_n, t.first, t.count, t.dtype, t.format_major};
      pieces[i] = DirPieces{t.meta_piece, t.page_piece};
      cursors[i] = ReadRef{t.from ? t.from->w : nullptr, t.to ? t.to->w : nullptr};
      hist[i] = HistRef{t.history, t.history_len};
      check_partial_task(who, rt[i], &pieces[i], dl.args.n_pieces, chunks);
      if ((t.history == nullptr) != (t.history_len == 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a history and its length go together"};
      if (((uintptr_t)t.history & 7u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": misaligned history"};
    }
    dl.pieces = pieces.data();
    return run_partial<kFormResume>(("directory " + w + " read").c_str(), n_tasks, rt.data(), cursors.data(), nullptr, &dl, flags, results, d_results, (hipStream_t)stream, hist.data());
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}
extern "C" enum PcoError pco_gfx_decompress_page_reads_dir(size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                           PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return reads_dir(false, n_tasks, tasks, dir, flags, results, d_results, stream);
}

static PcoError index_dir(bool chunks, size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags, PcoGfxTaskResult* results,
                          PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  const std::string w = chunks ? "chunk" : "page";   // (the messages' word)
  try {
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, w + " index directory: unknown flags"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, w + " index directory: null task array"};
    DirLaunch dl{checked_directory(dir, (w + " index").c_str()), nullptr, chunks};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, w + " index directory: results and d_results are both null"};
    std::vector<PcoGfxPageRangeTask> rt(n_tasks); std::vector<DirPieces> pieces(n_tasks); std::vector<IndexRef> index(n_tasks); std::vector<IndexHistRef> hist(n_tasks);
    bool any = false;
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxDirPageIndexTask& t = tasks[i];
      const std::string who = "directory " + w + " index task " + std::to_string(i);
      rt[i] = PcoGfxPageRangeTask{nullptr, 0, nullptr, 0, nullptr, t.page_n, 0, 0, t.dtype, t.format_major};
      pieces[i] = DirPieces{t.meta_piece, t.page_piece};
      check_partial_task(who, rt[i], &pieces[i], dl.args.n_pieces, chunks);
      if (t.every_rows == 0 || (t.every_rows & 255u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": every_rows is a positive multiple of 256"};
      const uint64_t k = index_len(t.page_n, t.every_rows);
      if (k > 0 && (t.cursors == nullptr || ((uintptr_t)t.cursors & 7u) != 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null or misaligned cursors"};
      if ((t.histories == nullptr) != (t.history_stride == 0)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": histories and their stride go together"};
      if ((t.history_stride & 7u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": the stride is a multiple of 8"};
      if (((uintptr_t)t.histories & 7u) != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": misaligned histories"};
      rt[i].count = k * t.every_rows;
      index[i] = IndexRef{k ? t.cursors->w : nullptr, (uint32_t)(k ? t.every_rows >> 8 : 0), (uint32_t)k};
      hist[i] = k ? IndexHistRef{t.histories, t.history_stride} : IndexHistRef{nullptr, 0};
      any = any || hist[i].histories != nullptr;
    }
    dl.pieces = pieces.data();
    // (a call without a history launches pco_gfx_index_pages_ex's kernels, as pco_gfx_index_pages_hist does)
    return run_partial<kFormIndex>(("directory " + w + " index").c_str(), n_tasks, rt.data(), nullptr, index.data(), &dl, flags, results, d_results, (hipStream_t)stream, nullptr,
                                   any ? hist.data() : nullptr);
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}
extern "C" enum PcoError pco_gfx_index_pages_dir(size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                 PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return index_dir(false, n_tasks, tasks, dir, flags, results, d_results, stream);
}

// include/pco_gfx.h section 4l: the same two with each task's one piece a standalone chunk behind pco_gfx_compact_chunks' offsets
extern "C" enum PcoError pco_gfx_decompress_chunk_reads_dir(size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                            PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return reads_dir(true, n_tasks, tasks, dir, flags, results, d_results, stream);
}
extern "C" enum PcoError pco_gfx_index_chunks_dir(size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                  PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return index_dir(true, n_tasks, tasks, dir, flags, results, d_results, stream);
}

// ---------------------------------------------------------------------------------------------------------
// include/pco_gfx.h section 4m: the chunk directory of standalone streams, scanned on the device (scan.hip).  ONE launch, one wave per stream; the
// global table scratch is taken up front in both forms, as an asynchronous decode takes it.
// ---------------------------------------------------------------------------------------------------------
static_assert(sizeof(PcoGfxScanTask) == 48, "PcoGfxScanTask");

namespace pcogfx {
namespace {

void launch_scan(size_t n_tasks, const PcoGfxScanTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results_user, hipStream_t stream) {
  Workspace& ws = workspace();
  PcoGfxScanTask* d_tasks = (PcoGfxScanTask*)ws.tasks.ensure(n_tasks * sizeof(PcoGfxScanTask) + 64);
  PcoGfxTaskResult* d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)ws.results.ensure(n_tasks * sizeof(PcoGfxTaskResult));
  const size_t grid = std::min<size_t>(n_tasks, kPartialGeneralGrid);
  uint8_t* tbl = (uint8_t*)ws.tbl_ws.ensure(grid * kTblWsBytes);
  PCO_HIP_CHECK(hipMemcpyAsync(d_tasks, tasks, n_tasks * sizeof(PcoGfxScanTask), hipMemcpyHostToDevice, stream));
  PCO_TIMED_LAUNCH("pco_scan_kernel", stream, pco_scan_kernel, dim3((uint32_t)grid), dim3(64), kPartialDecodeLdsBytes, stream, (const PcoGfxScanTask*)d_tasks, d_results, (uint32_t)n_tasks,
                   kPartialDecodeLdsBytes - kLdsFixed, tbl);
  PCO_HIP_CHECK(hipGetLastError());
  if (results) {
    PCO_HIP_CHECK(hipMemcpyAsync(results, d_results, n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
}

}  // namespace
}  // namespace pcogfx

extern "C" enum PcoError pco_gfx_scan_chunks(size_t n_tasks, const PcoGfxScanTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "scan: null task array"};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "scan: results and d_results are both null"};
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxScanTask& t = tasks[i];
      const std::string who = "scan task " + std::to_string(i);
      if (t.src == nullptr || t.d_offsets == nullptr || t.d_counts == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null src, d_offsets or d_counts"};
      if (t.max_chunks == 0 || t.max_chunks >= (1u << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": max_chunks must be 1 ..= 2^31 - 1"};
      if (width_group(t.dtype) < 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
      if (t.reserved != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": reserved must be 0"};
      if (t.flags & ~(PCO_GFX_TASK_HAS_FILE_HEADER | 0xff00u)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": unknown flag bits"};
      if (((uintptr_t)t.d_offsets & 7u) || ((uintptr_t)t.d_counts & 3u)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": d_offsets must be 8-byte and d_counts 4-byte aligned"};
    }
    if (n_tasks >= ((size_t)1 << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "scan: too many tasks for one call"};
    if (n_tasks == 0) return PcoSuccess;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_scan(n_tasks, tasks, results, d_results, (hipStream_t)stream); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "scan task " + std::to_string(i) + " failed behind " + std::to_string(results[i].n_out) + " chunks");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}
