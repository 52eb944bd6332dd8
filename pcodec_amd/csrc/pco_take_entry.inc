// pco_take_entry.inc -- pco_gfx_take_rows (include/pco_gfx.h section 4n): rows of indexed pages by row ids that live on the device.
// The entry point checks its arguments (before a device is asked for, in the order of the header's list, each refusal with its own words), cuts every
// take task's page at its index's cursors into segments and hands the driver of pco_partial_driver.inc ONE asynchronous read call whose tasks are
// those segments, laid out for whole segments with `dst` the segment's place in the task's row area; the driver's plan_take step lets the device
// narrow every segment's range to what the ids want.  Behind the driver the gather kernel moves the wanted rows to `dst` and the finishing kernel
// folds the segments' results into one per take task (take.hip).  Nothing of d_rows is read on the host, and nothing synchronises but the read-back of
// the synchronous form's results.

namespace pcogfx {
namespace {

struct TakeAt {
  size_t i;
  [[noreturn]] void refuse(int status, const char* why) const { throw HostError{status, "take rows task " + std::to_string(i) + ": " + why}; }
  [[noreturn]] void invalid(const char* why) const { refuse(PCO_GFX_INVALID_ARGUMENT, why); }
};

// one task's fields, in the header's order; segs: the segments of the call so far
void check_take_task(const TakeAt& at, const PcoGfxTakeTask& t, uint64_t& segs) {
  if (width_group(t.dtype) < 0) at.invalid("invalid number type");
  if (t.page_n == 0 || t.page_n > kMaxEntries) at.invalid("a page holds 1 ..= 2^24 numbers");
  if (t.meta == nullptr || t.page == nullptr) at.invalid("null ChunkMeta or page");
  if (t.row_base + t.page_n < t.row_base) at.invalid("row_base + page_n wraps");
  if ((t.every_rows & 255u) != 0) at.invalid("every_rows is a multiple of 256");
  const uint64_t k = index_len(t.page_n, t.every_rows);
  if (t.every_rows == 0 ? t.cursors != nullptr : (k > 0 && t.cursors == nullptr)) at.invalid("cursors and every_rows go together");
  if (((uintptr_t)t.cursors & 7u) != 0) at.invalid("misaligned cursors");
  const uintptr_t width = (uintptr_t)(dtype_bits(t.dtype) / 8);
  if (t.n_rows > 0 && (t.d_rows == nullptr || ((uintptr_t)t.d_rows & 7u) != 0)) at.invalid("null or misaligned d_rows");
  if (t.n_rows > 0 && (t.dst == nullptr || ((uintptr_t)t.dst & (width - 1)) != 0)) at.invalid("null or misaligned dst");
  if (t.n_rows >= (1ull << 32)) at.invalid("a task takes fewer than 2^32 row ids");
  segs += k + 1;
  if (segs > (1ull << 31)) at.invalid("more than 2^31 segments in one call; split the call");
  if (t.format_major > 4) at.refuse(PCO_GFX_CORRUPTION, "the file's format version definitely cannot be decompressed");   // wrapped/file_decompressor.rs:31-36
}

// the numbers of prefix scratch the driver gives a segment of `rows` rows on its scratch route (scratch_bytes with the walk's start known)
uint64_t take_scratch_numbers(uint64_t rows, uint64_t first, uint64_t page_n) { return std::min<uint64_t>((take_batches(rows) + 1) * kBatchN, page_n - first); }

void launch_take(size_t n_tasks, const PcoGfxTakeTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, hipStream_t stream) {
  Workspace& ws = workspace();
  const bool general = (flags & PCO_GFX_CURSOR_GENERAL) != 0;
  std::vector<TakeDev> takes(n_tasks); std::vector<uint64_t> area_at(n_tasks);
  std::vector<PcoGfxPageRangeTask> rt; std::vector<ReadRef> cursors; std::vector<uint32_t> seg_take;
  TakeLaunch tl{};
  std::vector<uint32_t> prefix[4];
  uint64_t area_bytes = 0, max_walk = 0, prefix_bytes = 0;
  for (size_t i = 0; i < n_tasks; i++) {
    const PcoGfxTakeTask& t = tasks[i];
    const uint32_t width = (uint32_t)(dtype_bits(t.dtype) / 8), n_seg = take_segments(t.page_n, t.every_rows);
    area_at[i] = area_bytes; area_bytes += (t.page_n * width + 255) & ~(uint64_t)255;
    takes[i] = TakeDev{t.d_rows, t.n_rows, t.dst, nullptr, t.row_base, t.page_n, t.every_rows, (uint32_t)rt.size(), n_seg, width, 0};
    tl.max_rows = std::max<uint64_t>(tl.max_rows, t.n_rows);
    for (uint32_t s = 0; s < n_seg; s++) {
      const uint64_t first = take_first(s, t.every_rows), rows = take_segment_rows(s, t.page_n, t.every_rows);
      if (s == 0) prefix[width_group(t.dtype)].push_back((uint32_t)rt.size());
      if (s == 0 || general) prefix_bytes += (take_scratch_numbers(rows, first, t.page_n) * width + 255) & ~(uint64_t)255;
      max_walk = std::max<uint64_t>(max_walk, take_batches(rows));
      rt.push_back(PcoGfxPageRangeTask{t.meta, t.meta_len, t.page, t.page_len, nullptr, t.page_n, first, rows, t.dtype, t.format_major});
      cursors.push_back(ReadRef{s ? t.cursors[s - 1].w : nullptr, nullptr});
      seg_take.push_back((uint32_t)i);
      tl.start_rows.push_back(first);
    }
  }
  const size_t n_segs = rt.size();
  flatten_groups(prefix, tl.prefix_ids, tl.prefix_off);
  // the scratch of the call, taken up front: the row areas, the symbols of the segments' walks, the scratch route's extents
  const uint64_t scratch = area_bytes + (uint64_t)n_segs * 3 * (max_walk * kBatchN + 256) + prefix_bytes;
  if (scratch > partial_budget_bytes(ws))
    throw HostError{PCO_GFX_INVALID_ARGUMENT, "take rows: the call takes " + std::to_string(scratch) + " bytes of scratch, more than PCO_GFX_WORKSPACE_GB allows; split the call"};

  WorkspaceUse use(ws, stream);
  uint8_t* area = (uint8_t*)ws.take_rows.ensure(area_bytes + 64);
  for (size_t i = 0; i < n_tasks; i++) {
    takes[i].area = area + area_at[i];
    for (uint32_t s = 0; s < takes[i].n_seg; s++) rt[takes[i].seg0 + s].dst = area + area_at[i] + rt[takes[i].seg0 + s].first * takes[i].width;
  }
  Layout at;
  const size_t takes_at = at.place(n_tasks * sizeof(TakeDev)), seg_take_at = at.place(n_segs * 4), zero_at = at.place(n_tasks * sizeof(TakeTally)),
               marks_at = at.place(n_segs * 4), zero_end = at.end, seg_res_at = at.place(n_segs * sizeof(PcoGfxTaskResult)), out_at = at.place(n_tasks * sizeof(PcoGfxTaskResult));
  uint8_t* small = (uint8_t*)ws.take_small.ensure(at.end + 64);
  TakeDev* d_takes = (TakeDev*)(small + takes_at);
  PcoGfxTaskResult* d_seg_results = (PcoGfxTaskResult*)(small + seg_res_at);
  PcoGfxTaskResult* d_out = d_results ? d_results : (PcoGfxTaskResult*)(small + out_at);
  PCO_HIP_CHECK(hipMemcpyAsync(d_takes, takes.data(), n_tasks * sizeof(TakeDev), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(small + seg_take_at, seg_take.data(), n_segs * 4, hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemsetAsync(small + zero_at, 0, zero_end - zero_at, stream));   // (the tallies and the marks)
  tl.d_takes = d_takes; tl.n_takes = (uint32_t)n_tasks; tl.d_seg_take = (const uint32_t*)(small + seg_take_at);
  tl.d_marks = (uint32_t*)(small + marks_at); tl.d_tally = (TakeTally*)(small + zero_at);

  PartialRequest rq{kFormResume, "take rows segment", n_segs, rt.data(), cursors.data(), nullptr, nullptr, nullptr, nullptr, flags, nullptr, d_seg_results, stream, &tl};
  launch_partial(rq);

  PCO_TIMED_LAUNCH("take_gather_kernel", stream, take_gather_kernel, tl.id_grid(kTakeBlock), dim3(kTakeBlock), 0, stream, (const TakeDev*)d_takes, tl.n_takes, (const PcoGfxTaskResult*)d_seg_results);
  PCO_TIMED_LAUNCH("take_finish_kernel", stream, take_finish_kernel, dim3(std::min<uint32_t>(tl.n_takes, 65535u)), dim3(64), 0, stream, (const TakeDev*)d_takes, tl.n_takes,
                   (const uint32_t*)tl.d_marks, (const PcoGfxTaskResult*)d_seg_results, tl.d_recs, (const TakeTally*)tl.d_tally, d_out);
  PCO_HIP_CHECK(hipGetLastError());
  if (results) {
    PCO_HIP_CHECK(hipMemcpyAsync(results, d_out, n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
}

}  // namespace
}  // namespace pcogfx

// include/pco_gfx.h section 4n
extern "C" enum PcoError pco_gfx_take_rows(size_t n_tasks, const PcoGfxTakeTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "take rows: null task array"};
    if (n_tasks && !results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "take rows: results and d_results are both null"};
    if (flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, "take rows: unknown flags"};
    uint64_t segs = 0;
    for (size_t i = 0; i < n_tasks; i++) check_take_task(TakeAt{i}, tasks[i], segs);
    if (n_tasks == 0) return PcoSuccess;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
    launch_take(n_tasks, tasks, flags, results, d_results, (hipStream_t)stream);
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "take rows task " + std::to_string(i) + " failed");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& err) { set_error(err.status, err.msg); return PcoDecompressionError; }
}
