// pco_partial_driver.inc -- the host driver of every entry point that decodes PART of a page (pco_gfx_ranges.hip includes it behind the kernels).
// An entry point (pco_partial_entry.inc) fills a PartialRequest; launch_partial derives a PartialPlan from it and runs the named steps below:
//   plan_tasks -> upload -> plan_take -> resolve_directory -> read_start_rows -> size_walk -> run_fast_route -> run_scratch_route -> finish
// Two routes decode a task.  Route 1, the two-kernel route: the walkers and the expander of decode_fast.hip in their range / resume / index forms,
// over every task of the call.  Route 2, the scratch route: the tasks the walkers hand back (Lookback, Conv1, Dict, tables beyond their LDS) decode
// their prefix into scratch with the single-kernel decoder, and their rows are copied out of it.

namespace pcogfx {
namespace {

constexpr uint32_t kPartialDecodeLdsBytes = 16 * 1024;   // the single-kernel decoder's dynamic LDS (fixed area + tANS tables), as in launch_decode
constexpr size_t kPartialGeneralGrid = 4096;             // ... and its grid bound: each block owns kTblWsBytes of table scratch

// what the scratch of one synchronous pass may take: PCO_GFX_WORKSPACE_GB, default 80 % of the free device memory (plus what the buffer holds).
// Read at every call: a test narrows it in mid-process.
size_t partial_budget_bytes(const Workspace& ws) { return scratch_budget_bytes(std::getenv("PCO_GFX_WORKSPACE_GB"), ws.dec_hist.cap); }

constexpr int kFormRange = 0, kFormResume = 1, kFormIndex = 2;   // what the tasks of a request are

// ---- the names pco_gfx_profile_* reports: "stem<uNN>", one string per kernel stem and width group, built here and kept (the profile keeps pointers) ----
struct WidthNames {
  std::string stem, name[4];
  explicit WidthNames(const std::string& s) : stem(s) {
    const char* const suffix[4] = {"<u64>", "<u32>", "<u16>", "<u8>"};
    for (int g = 0; g < 4; g++) name[g] = s + suffix[g];
  }
  const char* operator[](int g) const { return name[g].c_str(); }
};
struct FastNames {   // route 1's three kernels in one form
  WidthNames walk, walk4, expand;
  explicit FastNames(const std::string& form) : walk("dec_walk_" + form + "_kernel"), walk4("dec_walk4_" + form + "_kernel"), expand("dec_expand_" + form + "_kernel") {}
};
const FastNames kFastNames[3] = {FastNames("range"), FastNames("resume"), FastNames("index")};   // [form]
const WidthNames kPrefixName("pco_decode_prefix_kernel"), kCopyName("range_copy_kernel"), kGeneralResumeName("pco_decode_general_resume_kernel"),
    kGeneralIndexName("pco_decode_general_index_kernel"), kGeneralIndexHistName("pco_decode_general_index_hist_kernel"), kSnapshotName("index_history_snapshot_kernel");

// ---- a take call (pco_gfx_take_rows, section 4n; pco_take_entry.inc fills it) ----
// Its request is a read call whose tasks are the SEGMENTS of the take tasks' pages, laid out for whole segments; the device decides from the row
// ids what each of them reads (plan_take).  The host states where every segment starts, so no cursor is read back; without the general flag only
// the tasks of `prefix_ids` -- the segments that start at their page's first row -- have a place on the scratch route.
struct TakeLaunch {
  const TakeDev* d_takes; uint32_t n_takes; const uint32_t* d_seg_take; uint32_t* d_marks; TakeTally* d_tally; uint64_t max_rows;
  std::vector<uint64_t> start_rows;                            // per read task: s * every_rows
  std::vector<uint32_t> prefix_ids; size_t prefix_off[5];      // the read tasks with start row 0, grouped by width as PartialPlan::ids
  const RangeRef* d_ranges = nullptr; const ReadRec* d_recs = nullptr;   // (out) where the request's ranges and records lie, for the kernels behind the driver
  dim3 id_grid(uint32_t per_block) const { return dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>((max_rows + per_block - 1) / per_block, 1), 2048), std::min<uint32_t>(n_takes, 65535u)); }
};

// ---- the request ----
// What an entry point asks for.  Every task is seen as a range: a read is a range and its two cursors; an index task is the range {first 0,
// count k * every_rows} without a dst, and `index` says where its k cursors go.  A _dir form leaves the tasks' meta / page null and names them in
// dir->pieces.  The references that a form does not have are null.
struct PartialRequest {
  int form;                           // kFormRange, kFormResume (the tasks are reads), kFormIndex
  std::string what;                   // "page range", "directory chunk read", ...: the call's failure report is "<what> task i failed"
  size_t n_tasks;
  const PcoGfxPageRangeTask* tasks;
  const ReadRef* cursors;             // reads: from / to
  const IndexRef* index;              // index calls
  const HistRef* hist;                // reads with histories (section 4i and the _dir reads): one reference per task, null pointers for the tasks without
  const IndexHistRef* ihist;          // index calls in which some task has histories (section 4j): one reference per task
  const DirLaunch* dir;               // the _dir forms: the directory, the tasks' piece pairs, whether a piece is a standalone chunk (section 4l)
  uint32_t flags;                     // PCO_GFX_CURSOR_GENERAL or 0
  PcoGfxTaskResult* results; PcoGfxTaskResult* d_results;   // results null: the asynchronous form
  hipStream_t stream;
  TakeLaunch* take = nullptr;         // a take call: its tasks are segments, and plan_take writes their ranges
  bool resume() const { return form == kFormResume; }
  bool indexing() const { return form == kFormIndex; }
  bool synchronous() const { return results != nullptr; }
  std::string form_word() const { return indexing() ? "page index: " : (resume() ? "page reads: " : "page ranges: "); }
};

// ---- the call's device arrays ----
// They lie side by side in one workspace buffer.  device_arrays() below is the ONE list of them: which exist for this request, how long they are and
// what the host uploads into them.
struct PartialArrays {
  PcoGfxDecodeTask* tasks = nullptr; uint32_t* ids = nullptr; MetaRef* metas = nullptr; RangeRef* ranges = nullptr;
  ReadRef* curs = nullptr; ReadRec* recs = nullptr; uint64_t* rows = nullptr;         // a read call: cursor references | per-task records | the rows the `from` cursors stand at
  DirPieces* pieces = nullptr; uint8_t* bad_meta = nullptr;                            // a directory call: piece pairs | (chunks) the one-byte ChunkMeta of a refusal by Corruption
  IndexRef* irefs = nullptr; RangeRef* ranges1 = nullptr;                              // an index call: cursor references | route 2's ranges
  ReadRef* srefs = nullptr; uint64_t* swords = nullptr; uint64_t* grows = nullptr; RangeRef* rel = nullptr;   // shadows (read_start_rows) | their rows | the rows' places in the scratch
  HistRef* hrefs = nullptr;                                                            // a read call with histories
  IndexHistRef* ihrefs = nullptr; IndexHistRec* ihrecs = nullptr;                      // an index call with histories: references | what the walk leaves the snapshot kernel
};

// ---- the plan: the request and everything the steps derive from it ----
struct PartialPlan {
  const PartialRequest& rq;
  Workspace& ws;
  const uint32_t allow_general;   // the call's flag, as the kernels take it
  const bool general;             // route 2 runs the kernels of decode_general.hip in place of the prefix kernel
  const bool shadows;             // a read call on the general route: route 1 starts from shadows of the `from` cursors
  // plan_tasks
  std::vector<PcoGfxDecodeTask> dt; std::vector<MetaRef> metas; std::vector<RangeRef> ranges;
  std::vector<PcoGfxPageRangeTask> first_row; std::vector<RangeRef> ranges1;   // (an index call) what route 2 decodes: the range {0, 1}
  std::vector<PcoGfxPageRangeTask> prefix_row;   // (an index call with histories) ... and what sizes its scratch where a task with histories gets its whole prefix
  std::vector<uint32_t> ids; size_t id_off[5] = {0, 0, 0, 0, 0};   // task ids grouped by number width: group g at [id_off[g], id_off[g + 1])
  uint64_t max_count = 0, snap_grid = 1; bool any_from = false;
  // upload
  PartialArrays d;
  // read_start_rows
  std::vector<uint64_t> rows, grows;   // (reads) the row each `from` cursor stands at, for route 1 and for the general route: zeros where the host does not know
  // size_walk
  uint64_t max_walk = 0; PcoGfxTaskResult* d_results = nullptr; DecPlan* d_plans = nullptr;

  explicit PartialPlan(const PartialRequest& r)
      : rq(r), ws(workspace()), allow_general((r.flags & PCO_GFX_CURSOR_GENERAL) != 0 ? 1u : 0u),
        general(r.form != kFormRange && (allow_general || (r.resume() && r.hist != nullptr) || (r.indexing() && r.ihist != nullptr))), shadows(r.resume() && general) {}
  uint32_t n() const { return (uint32_t)rq.n_tasks; }
  dim3 task_grid() const { return dim3((uint32_t)((rq.n_tasks + 255) / 256)); }   // one thread per task
  const RangeRef* scratch_ranges() const { return rq.indexing() ? d.ranges1 : d.ranges; }
  const PcoGfxPageRangeTask* scratch_view() const { return rq.indexing() ? first_row.data() : rq.tasks; }
  uint32_t copy_slices() const { return rq.indexing() ? 0u : (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (max_count + 4095) / 4096)); }   // (an index call copies no rows)
};

// Step 1: the tasks as the kernels take them, grouped by number width.  An index task's device range is {0, k * every_rows}, so the kernels'
// "count == 0 takes no verdict" is the k == 0 of an index task; route 2 gets the range {0, 1} for it (two batches of scratch, the verdict and no copy).
// A task with histories may walk its whole prefix into scratch, and only the device knows which do: an asynchronous call gives every such task that
// scratch up front; a synchronous one gives two batches as ever and sizes the passes of its second round by the whole prefixes.
void plan_tasks(PartialPlan& p) {
  const PartialRequest& rq = p.rq;
  const size_t n = rq.n_tasks;
  p.dt.resize(n); p.metas.resize(n); p.ranges.resize(n);
  if (rq.indexing()) { p.first_row.resize(n); p.ranges1.resize(n); }
  if (rq.indexing() && rq.ihist) p.prefix_row.resize(n);
  std::vector<uint32_t> ids[4];
  for (size_t i = 0; i < n; i++) {
    const PcoGfxPageRangeTask& t = rq.tasks[i];
    p.dt[i] = PcoGfxDecodeTask{t.page, t.page_len, t.dst, t.page_n, t.dtype, PCO_GFX_TASK_WRAPPED_PAGE | (t.format_major << 8)};
    p.metas[i] = MetaRef{t.meta, t.meta_len}; p.ranges[i] = RangeRef{t.first, t.count};
    if (rq.resume()) p.any_from = p.any_from || (rq.cursors[i].from != nullptr && t.count != 0);
    if (rq.indexing()) { p.first_row[i] = t; p.first_row[i].count = t.count ? 1 : 0; p.ranges1[i] = RangeRef{0, p.first_row[i].count}; }
    if (rq.indexing() && rq.ihist) {
      p.prefix_row[i] = rq.ihist[i].histories && t.count ? t : p.first_row[i];
      if (!rq.synchronous()) p.first_row[i] = p.prefix_row[i];   // (the device ranges stay {0, 1}: the kernel sizes a snapshot walk by the index reference and its scratch's cap)
      if (rq.ihist[i].histories && t.count)   // (cursor, stretch) pairs of the longest history this task can have: the snapshot kernel's grid.x
        p.snap_grid = std::max<uint64_t>(p.snap_grid, (t.count / rq.index[i].every_batches / kBatchN) * ((std::min<uint64_t>(t.count + kBatchN, t.page_n) + 8 + kSnapRows - 1) / kSnapRows));
    }
    ids[width_group(t.dtype)].push_back((uint32_t)i);
    p.max_count = std::max<uint64_t>(p.max_count, t.count);
  }
  flatten_groups(ids, p.ids, p.id_off);
}

// The list of the call's device arrays: f(pointer, elements, whether this request has the array, what to upload or nullptr).
template <class F>
void device_arrays(PartialPlan& p, F& f) {
  const PartialRequest& rq = p.rq;
  const size_t n = rq.n_tasks;
  const bool dir = rq.dir != nullptr;
  f(p.d.tasks, n, true, p.dt.data());
  f(p.d.ids, n, true, p.ids.data());
  f(p.d.metas, n, true, p.metas.data());
  f(p.d.ranges, n, true, p.ranges.data());
  f(p.d.curs, n, rq.resume(), rq.cursors);
  f(p.d.recs, n, rq.resume(), nullptr);
  f(p.d.rows, n, rq.resume(), nullptr);
  f(p.d.pieces, n, dir, dir ? rq.dir->pieces : nullptr);
  f(p.d.bad_meta, 16, dir && rq.dir->chunks, nullptr);
  f(p.d.irefs, n, rq.indexing(), rq.index);
  f(p.d.ranges1, n, rq.indexing(), p.ranges1.data());
  f(p.d.srefs, n, p.shadows, nullptr);
  f(p.d.swords, n * kCursorWords, p.shadows, nullptr);
  f(p.d.grows, n, p.shadows, nullptr);
  f(p.d.rel, n, p.shadows, nullptr);
  f(p.d.hrefs, n, rq.hist != nullptr, rq.hist);
  f(p.d.ihrefs, n, rq.ihist != nullptr, rq.ihist);
  f(p.d.ihrecs, n, rq.ihist != nullptr, nullptr);
}

// One walk over that list.  base == nullptr: the arrays are placed and the buffer's size is at.end; else each array gets its pointer and its upload.
template <class T> struct SameAs { using type = T; };   // (keeps `src` out of the deduction: it may be a plain nullptr)
struct PlaceArrays {
  uint8_t* base; hipStream_t stream; Layout at;
  template <class T>
  void operator()(T*& ptr, size_t count, bool present, const typename SameAs<T>::type* src) {
    if (!present) return;
    const size_t off = at.place(count * sizeof(T));
    if (!base) return;
    ptr = (T*)(base + off);
    if (src) PCO_HIP_CHECK(hipMemcpyAsync(ptr, src, count * sizeof(T), hipMemcpyHostToDevice, stream));
  }
};

// Step 2: the device arrays, placed and uploaded.
void upload(PartialPlan& p) {
  PlaceArrays size{nullptr, p.rq.stream, Layout{}};
  device_arrays(p, size);
  PlaceArrays fill{(uint8_t*)p.ws.tasks.ensure(size.at.end + 64), p.rq.stream, Layout{}};
  device_arrays(p, fill);
  if (p.d.ihrecs) PCO_HIP_CHECK(hipMemsetAsync(p.d.ihrecs, 0, p.rq.n_tasks * sizeof(IndexHistRec), p.rq.stream));   // (the one array that starts as zeros)
}

// Step 3 (a take call; nothing for every other request): the ids mark their segments, and every segment's device range becomes what its read task
// reads -- {first, largest wanted row + 1 - first}, or {first, 0} for a segment nobody wants (take.hip).  The host arrays keep the whole segments.
void plan_take(PartialPlan& p) {
  TakeLaunch* tk = p.rq.take;
  if (!tk) return;
  const hipStream_t stream = p.rq.stream;
  PCO_TIMED_LAUNCH("take_mark_kernel", stream, take_mark_kernel, tk->id_grid(2 * kTakePairTile), dim3(kTakeBlock), 0, stream, tk->d_takes, tk->n_takes, tk->d_marks, tk->d_tally);
  PCO_TIMED_LAUNCH("take_plan_kernel", stream, take_plan_kernel, p.task_grid(), dim3(kTakeBlock), 0, stream, tk->d_takes, tk->d_seg_take, (const uint32_t*)tk->d_marks, p.n(), p.d.ranges,
                   tk->d_tally);
  PCO_HIP_CHECK(hipGetLastError());
  tk->d_ranges = p.d.ranges; tk->d_recs = p.d.recs;
}

// Step 4 (the _dir forms): the resolve kernel fills the device tasks' sources and ChunkMeta references from the directory and the piece pairs
// (dir_resolve.hip).  A refused read task loses the device copy of its cursor pair as well, so the read forms pass it; a chunk directory (section 4l)
// has kernels of its own, which point a refusal by Corruption at bad_meta.
template <class Kernel, class... Tail>
void launch_resolve(const PartialPlan& p, const char* name, Kernel* kernel, Tail... tail) {
  PCO_TIMED_LAUNCH(name, p.rq.stream, kernel, p.task_grid(), dim3(256), 0, p.rq.stream,
                   p.d.tasks, p.d.metas, (const DirPieces*)p.d.pieces, (const RangeRef*)p.d.ranges, p.n(), p.rq.dir->args, tail...);
  PCO_HIP_CHECK(hipGetLastError());
}
void resolve_directory(PartialPlan& p) {
  if (!p.rq.dir) return;
  DirCursorPair* pairs = (DirCursorPair*)p.d.curs;
  if (p.rq.dir->chunks && p.rq.resume()) launch_resolve(p, "dir_resolve_chunks_reads_kernel", dir_resolve_chunks_reads_kernel<true>, p.d.bad_meta, pairs);
  else if (p.rq.dir->chunks) launch_resolve(p, "dir_resolve_chunks_kernel", dir_resolve_chunks_kernel<true>, p.d.bad_meta);
  else if (p.rq.resume()) launch_resolve(p, "dir_resolve_reads_kernel", dir_resolve_reads_kernel<true>, pairs);
  else launch_resolve(p, "dir_resolve_kernel", dir_resolve_kernel<true>);
}

// Step 5 (reads): where the walks start.  A read walks from batch at / 256, and `at` lives in the `from` cursor on the device: a synchronous call reads
// the rows back; an asynchronous one cannot.  On the general route the two-kernel route gets shadows of the `from` cursors it cannot take itself:
// reads_shadow_kernel's of the kind-3 cursors of a flagged call; with histories reads_shadow_hist_kernel's -- of kind-3 cursors under the flag, of
// kind-4 cursors for the tasks with a history.  Both leave the rows for route 1 and for the general kernel's scratch beside the shadows.
void read_start_rows(PartialPlan& p) {
  const PartialRequest& rq = p.rq;
  if (!rq.resume()) return;
  const PartialArrays& d = p.d; const ReadRef* curs = d.curs; const RangeRef* ranges = d.ranges;
  p.rows.assign(rq.n_tasks, 0);
  if (p.shadows) p.grows.assign(rq.n_tasks, 0);
  if (rq.take) { p.rows = rq.take->start_rows; if (p.shadows) p.grows = rq.take->start_rows; }   // (stated by construction: a cursor that stands elsewhere is refused by walk_cap)
  const bool read_back = rq.synchronous() && p.any_from;
  if (p.shadows && rq.hist)
    PCO_TIMED_LAUNCH("reads_shadow_hist_kernel", rq.stream, reads_shadow_hist_kernel, p.task_grid(), dim3(256), 0, rq.stream, curs, ranges, (const HistRef*)d.hrefs, p.allow_general, p.n(),
                     d.srefs, d.swords, d.rows, d.grows);
  else if (p.shadows)
    PCO_TIMED_LAUNCH("reads_shadow_kernel", rq.stream, reads_shadow_kernel, p.task_grid(), dim3(256), 0, rq.stream, curs, ranges, p.n(), d.srefs, d.swords, d.rows, d.grows);
  else if (read_back)
    PCO_TIMED_LAUNCH("reads_rows_kernel", rq.stream, reads_rows_kernel, p.task_grid(), dim3(256), 0, rq.stream, curs, p.n(), d.rows);
  else
    return;
  PCO_HIP_CHECK(hipGetLastError());
  if (!read_back) return;
  PCO_HIP_CHECK(hipMemcpyAsync(p.rows.data(), d.rows, rq.n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, rq.stream));
  if (p.shadows) PCO_HIP_CHECK(hipMemcpyAsync(p.grows.data(), d.grows, rq.n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, rq.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(rq.stream));
}

// Step 6: symbols and section starts are sized by the most batches a task of the call WALKS, not by its longest page.  A range walks its PREFIX,
// batches [0, ceil((first + count) / 256)); a read walks from its start row where the host knows it, and is sized by the end batch as a range where
// it does not.
void size_walk(PartialPlan& p) {
  const PartialRequest& rq = p.rq;
  for (size_t i = 0; i < rq.n_tasks; i++) {
    if (!rq.tasks[i].count) continue;
    const uint64_t b_end = range_end_batch(rq.tasks[i].first, rq.tasks[i].count);
    p.max_walk = std::max<uint64_t>(p.max_walk, b_end - (rq.resume() ? std::min<uint64_t>(p.rows[i] >> 8, b_end - 1) : 0));   // (a cursor behind `first` is refused on the device)
  }
  p.d_results = rq.d_results ? rq.d_results : (PcoGfxTaskResult*)p.ws.results.ensure(rq.n_tasks * sizeof(PcoGfxTaskResult));
  if (rq.n_tasks * 3 * (p.max_walk * kBatchN + 256) > ((size_t)48 << 30))
    throw HostError{PCO_GFX_INVALID_ARGUMENT, rq.form_word() + (rq.resume() ? "the batches one call walks" : "the prefixes of one call") +
                    " may take 48 GiB of symbol scratch at most; split the call"};
  p.d_plans = (DecPlan*)p.ws.dec_plans.ensure(rq.n_tasks * sizeof(DecPlan));
}

// Route 1 over one width group: the 8-chunk walker, the 4-chunk walker over what that one handed back, the expander.  The form chooses the kernels;
// the resume ones take ResumeArgs behind the range ones' arguments -- the shadows where the call has them -- and the index ones IndexArgs.
struct FastStep {
  const PartialPlan& p; int g; uint8_t* d_bins; uint8_t* d_sym; uint64_t sym_stride; uint64_t* d_offpos; uint64_t offpos_stride;
  template <class L>
  void launch() const {
    if (p.rq.indexing()) run<L>(dec_walk_index_kernel<L, 8>, dec_walk_index_kernel<L, 4>, dec_expand_index_kernel<L>, IndexArgs{p.d.irefs});
    else if (p.rq.resume())
      run<L>(dec_walk_resume_kernel<L, 8>, dec_walk_resume_kernel<L, 4>, dec_expand_resume_kernel<L>, ResumeArgs{p.shadows ? p.d.srefs : p.d.curs, p.d.recs, (uint32_t)p.max_walk});
    else run<L>(dec_walk_range_kernel<L, 8>, dec_walk_range_kernel<L, 4>, dec_expand_range_kernel<L>);
  }
  template <class L, class Walk, class Expand, class... Tail>
  void run(Walk* walk8, Walk* walk4, Expand* expand, Tail... tail) const {
    const FastNames& names = kFastNames[p.rq.form];
    PCO_RESERVE_LDS(walk8, 4 * WalkCfg<8>::kWalkLdsBytes, names.walk.stem);   // (both before anything is launched; L is a parameter because the walkers of all
    PCO_RESERVE_LDS(walk4, 4 * WalkCfg<4>::kWalkLdsBytes, names.walk.stem);   // widths have one type, and each needs its own reservation)
    walk<8>(names.walk, walk8, 0u, tail...);
    walk<4>(names.walk4, walk4, kStatusRetryK4, tail...);
    PCO_TIMED_LAUNCH(names.expand[g], p.rq.stream, expand, dim3((uint32_t)std::min<size_t>(cnt(), kPartialGeneralGrid)), dim3(256), kExpLdsBytes, p.rq.stream, (const PcoGfxDecodeTask*)p.d.tasks,
                     p.d_results, ids(), cnt(), p.d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, (const RangeRef*)p.d.ranges, tail...);
  }
  // a walker of kWQ chunks a wave, four waves a block; accept_status: the status of the tasks it takes (0: every task; the 4-chunk walker: what the 8-chunk one handed back).
  template <uint32_t kWQ, class Walk, class... Tail>
  void walk(const WidthNames& name, Walk* kernel, uint32_t accept_status, Tail... tail) const {
    PCO_TIMED_LAUNCH(name[g], p.rq.stream, kernel, dim3(((cnt() + kWQ - 1) / kWQ + 3) / 4), dim3(256), 4 * WalkCfg<kWQ>::kWalkLdsBytes, p.rq.stream, (const PcoGfxDecodeTask*)p.d.tasks, ids(), cnt(),
                     p.d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, accept_status, p.d_results, (const MetaRef*)p.d.metas, (const RangeRef*)p.d.ranges, tail...);
  }
  uint32_t cnt() const { return (uint32_t)(p.id_off[g + 1] - p.id_off[g]); }
  const uint32_t* ids() const { return p.d.ids + p.id_off[g]; }
};

// Step 7: route 1 over every task of the call, one width group at a time.
void run_fast_route(PartialPlan& p) {
  const size_t n = p.rq.n_tasks;
  const uint64_t sym_stride = p.max_walk * kBatchN + 256, offpos_stride = sym_stride / 256 + 2;
  uint8_t* d_bins = (uint8_t*)p.ws.dec_bins.ensure(n * kBinsAreaPerTask);
  uint8_t* d_sym = (uint8_t*)p.ws.dec_sym.ensure(n * 3 * sym_stride + 64);
  uint64_t* d_offpos = (uint64_t*)p.ws.dec_offpos.ensure(n * 3 * offpos_stride * 8);
  for (int g = 0; g < 4; g++) {
    if (p.id_off[g + 1] == p.id_off[g]) continue;
    launch_width(g, FastStep{p, g, d_bins, d_sym, sym_stride, d_offpos, offpos_stride});
    PCO_HIP_CHECK(hipGetLastError());
  }
}

// One pass of route 2: the tasks `list` (task ids grouped by width, group g at [goff[g], goff[g + 1])), whose scratch is sized by `view`.
// filt: run over every task of the call and let the device pick the ones the walkers handed back (the asynchronous form).  with_hist: the pass has
// the second history buffer; need_hist: the status of a task that asks for one.
struct ScratchPass {
  const PcoGfxPageRangeTask* view; const std::vector<uint32_t>& list; const size_t (&goff)[5]; bool with_hist; const uint32_t* filt; uint32_t need_hist;
};

// (the general route of a read) the batch a task's walk starts at, as far as the host knows: the batch of its `from` cursor in a synchronous call, else 0
uint64_t start_batch(const PartialPlan& p, const PcoGfxPageRangeTask& t, size_t i) { return p.shadows ? std::min<uint64_t>(p.grows[i] >> 8, t.first >> 8) : 0; }
// the scratch a task takes on route 2: the batches it walks and one more, or what the page has from there
uint64_t scratch_bytes(const PartialPlan& p, const PcoGfxPageRangeTask& t, size_t i) {
  const uint64_t b0 = start_batch(p, t, i);
  const uint64_t numbers = std::min<uint64_t>((range_end_batch(t.first, t.count) - b0 + 1) * kBatchN, t.page_n - b0 * kBatchN);   // (b0 == 0: range_scratch_numbers)
  return (numbers * (uint64_t)(dtype_bits(t.dtype) / 8) + 255) & ~(uint64_t)255;
}

// Route 2 over one width group: the tasks' prefixes into scratch, their rows out of it.  launch() picks the decoder once -- the prefix kernel, or on the
// general route the kernel of decode_general.hip for the call's form -- with its profile name and what it takes behind the arguments all of them share;
// an index call, which wants the verdict and no rows, has copy_slices() == 0 and copies nothing.
struct ScratchStep {
  const PartialPlan& p; const ScratchPass& pass; int g; uint8_t* tbl; uint8_t* d_scratch; uint8_t* d_hist; const uint64_t* d_off; const uint32_t* d_list; const uint32_t* d_wcap;
  uint32_t cnt() const { return (uint32_t)(pass.goff[g + 1] - pass.goff[g]); }

  template <class L>
  void launch() const {
    const PartialArrays& d = p.d;
    const IndexArgs ix{d.irefs}; const IndexHistArgs ha{d.ihrefs, d.ihrecs, d_wcap, p.allow_general};   // what the general index decoders take behind the common arguments
    const GeneralResumeArgs ga{d.curs, d.recs, d_wcap, d.rel};   // ... and the general read decoders, which say in `rel` which rows of the scratch are the task's
    if (p.rq.ihist) decode(kGeneralIndexHistName, pco_decode_general_index_hist_kernel<L>, ix, p.d_plans, ha);   // (the index kernel compiled with kHist)
    else if (p.general && p.rq.indexing()) decode(kGeneralIndexName, pco_decode_general_index_kernel<L>, ix, p.d_plans);
    else if (p.shadows && p.rq.hist) decode(kGeneralResumeName, pco_decode_general_resume_kernel<L, true>, ga, HistArgs{d.hrefs, p.allow_general});   // (... the resume kernel with kHist)
    else if (p.shadows) decode(kGeneralResumeName, pco_decode_general_resume_kernel<L>, ga, NoGeneralIO{});   // (its defaulted last argument, which a call through a pointer has to name)
    else decode(kPrefixName, pco_decode_prefix_kernel<L>);
    if (p.rq.ihist)   // the rings out of the scratch the index kernel left
      PCO_TIMED_LAUNCH(kSnapshotName[g], p.rq.stream, index_history_snapshot_kernel<L>, dim3((uint32_t)std::min<uint64_t>(p.snap_grid, 8192), std::min<uint32_t>(cnt(), 1024u)), dim3(256), 0,
                       p.rq.stream, (const PcoGfxDecodeTask*)d.tasks, (const PcoGfxTaskResult*)p.d_results, d_list, cnt(), (const uint8_t*)d_scratch, d_off, (const IndexRef*)d.irefs, ha);
    if (p.copy_slices() == 0) return;
    PCO_TIMED_LAUNCH(kCopyName[g], p.rq.stream, range_copy_kernel<L>, dim3(std::min<uint32_t>(cnt(), 16384u), p.copy_slices()), dim3(256), 0, p.rq.stream, (const PcoGfxDecodeTask*)d.tasks,
                     (const PcoGfxTaskResult*)p.d_results, d_list, cnt(), pass.filt, (uint32_t)(sizeof(DecPlan) / 4), kStatusRetryLegacy, (const uint8_t*)d_scratch, d_off,
                     p.shadows ? (const RangeRef*)d.rel : p.scratch_ranges());
  }
  // the one launch of a single-kernel decoder: `tail` is what this one takes behind the arguments of pco_decode_prefix_kernel
  template <class Kernel, class... Tail>
  void decode(const WidthNames& names, Kernel* kernel, Tail... tail) const {
    PCO_TIMED_LAUNCH(names[g], p.rq.stream, kernel, dim3((uint32_t)std::min<size_t>(cnt(), kPartialGeneralGrid)), dim3(64), kPartialDecodeLdsBytes, p.rq.stream,
                     (const PcoGfxDecodeTask*)p.d.tasks, p.d_results, d_list, cnt(), kPartialDecodeLdsBytes - kLdsFixed, tbl, pass.filt, (uint32_t)(sizeof(DecPlan) / 4), kStatusRetryLegacy,
                     d_scratch, d_off, d_hist, pass.need_hist, (const MetaRef*)p.d.metas, p.scratch_ranges(), tail...);
  }
};

// One pass of route 2: its scratch (the tasks' extents, behind them the second history buffer of a pass that has one, then the extents' offsets, the
// task list and -- on the general route -- the batches of scratch each task has from its start batch), then the width groups.
void run_scratch(PartialPlan& p, const ScratchPass& pass) {
  const std::vector<uint32_t>& list = pass.list;
  std::vector<uint64_t> offs(list.size()); uint64_t bytes = 0;
  std::vector<uint32_t> wcap(p.general ? list.size() : 0);
  for (size_t k = 0; k < list.size(); k++) {
    offs[k] = bytes;
    const PcoGfxPageRangeTask& t = pass.view[list[k]];
    if (t.count) bytes += scratch_bytes(p, t, list[k]);
    if (p.general) wcap[k] = t.count ? (uint32_t)(range_end_batch(t.first, t.count) - start_batch(p, t, list[k])) : 0u;
  }
  const uint64_t hist_at = (bytes + 255) & ~(uint64_t)255, tail_at = hist_at + (pass.with_hist ? hist_at : 0);
  uint8_t* d_scratch = (uint8_t*)p.ws.dec_hist.ensure(tail_at + list.size() * 16 + 256);
  uint64_t* d_off = (uint64_t*)(d_scratch + tail_at);
  uint32_t* d_list = (uint32_t*)(d_off + list.size());
  uint32_t* d_wcap = d_list + list.size();
  PCO_HIP_CHECK(hipMemcpyAsync(d_off, offs.data(), list.size() * 8, hipMemcpyHostToDevice, p.rq.stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, p.rq.stream));
  if (p.general && !list.empty()) PCO_HIP_CHECK(hipMemcpyAsync(d_wcap, wcap.data(), list.size() * 4, hipMemcpyHostToDevice, p.rq.stream));
  size_t max_grid = 0;
  for (int g = 0; g < 4; g++) max_grid = std::max(max_grid, std::min<size_t>(pass.goff[g + 1] - pass.goff[g], kPartialGeneralGrid));
  uint8_t* tbl = (uint8_t*)p.ws.tbl_ws.ensure(max_grid * kTblWsBytes);
  for (int g = 0; g < 4; g++) {
    if (pass.goff[g + 1] == pass.goff[g]) continue;
    launch_width(g, ScratchStep{p, pass, g, tbl, d_scratch, pass.with_hist ? d_scratch + hist_at : nullptr, d_off + pass.goff[g], d_list + pass.goff[g], d_wcap + pass.goff[g]});
    PCO_HIP_CHECK(hipGetLastError());
  }
}

void read_results(const PartialPlan& p) {
  PCO_HIP_CHECK(hipMemcpyAsync(p.rq.results, p.d_results, p.rq.n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, p.rq.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(p.rq.stream));
}

// (a synchronous call) one round of passes over the tasks whose status is `want`, each pass a stretch of the call's tasks whose scratch fits the
// budget; returns whether any ran.  The second round has the second history buffer, and twice the scratch a task.
bool run_scratch_round(PartialPlan& p, int round) {
  const PartialRequest& rq = p.rq;
  const uint32_t want = round == 0 ? kStatusRetryLegacy : kStatusNeedHist;
  const PcoGfxPageRangeTask* view = rq.indexing() && rq.ihist ? p.prefix_row.data() : p.scratch_view();
  const size_t budget = partial_budget_bytes(p.ws);
  bool any = false;
  for (size_t next = 0; next < rq.n_tasks;) {
    std::vector<uint32_t> ids[4]; uint64_t bytes = 0; size_t taken = 0;
    for (; next < rq.n_tasks; next++) {
      if (rq.results[next].status != want) continue;
      const uint64_t b = scratch_bytes(p, view[next], next) * (round ? 2 : 1);
      if (taken && bytes + b > budget) break;
      ids[width_group(view[next].dtype)].push_back((uint32_t)next); bytes += b; taken++;
    }
    if (!taken) break;
    std::vector<uint32_t> list; size_t goff[5];
    flatten_groups(ids, list, goff);
    run_scratch(p, ScratchPass{view, list, goff, round == 1, nullptr, round == 0 ? kStatusNeedHist : (uint32_t)PCO_GFX_UNSUPPORTED});
    PCO_HIP_CHECK(hipStreamSynchronize(rq.stream));   // (the next pass writes the same scratch, and may move it)
    any = true;
  }
  return any;
}

// Step 8: route 2; returns whether it ran at all.
// Asynchronous: the call cannot come back, so every task takes its prefix scratch up front and the device picks the tasks of route 2 (the history of
// a delta'd secondary variable under lookback stays the one thing such a call does not have: PCO_GFX_UNSUPPORTED, as in pco_gfx_decompress_pages).
// An index call does so in both forms: two batches a task need no passes, and its synchronous form comes back for that history alone (and for the
// tasks with histories that need more than two batches, which come back with the same status).
// Synchronous: the tasks the walkers handed back go through route 2 in passes whose scratch fits the budget; the ones that then ask for a second
// history buffer once more, with it.
bool run_scratch_route(PartialPlan& p) {
  const PartialRequest& rq = p.rq;
  if (rq.take && !p.general)   // (a take call is asynchronous; its segments behind a cursor have no prefix scratch)
    run_scratch(p, ScratchPass{p.scratch_view(), rq.take->prefix_ids, rq.take->prefix_off, false, (const uint32_t*)p.d_plans, (uint32_t)PCO_GFX_UNSUPPORTED});
  else if (!rq.synchronous() || rq.indexing())
    run_scratch(p, ScratchPass{p.scratch_view(), p.ids, p.id_off, false, (const uint32_t*)p.d_plans, rq.synchronous() ? kStatusNeedHist : (uint32_t)PCO_GFX_UNSUPPORTED});
  if (!rq.synchronous()) return true;
  read_results(p);
  bool ran = rq.indexing();
  for (int round = rq.indexing() ? 1 : 0; round < 2; round++) {
    if (!run_scratch_round(p, round)) break;
    ran = true;
    read_results(p);
  }
  return ran;
}

// Step 9 (reads and index calls whose route 2 ran): the finishing kernel writes the position-only cursors of route 2 -- a read's `to`, an index
// task's k cursors and its result; a synchronous call then reads its results once more.
void finish(PartialPlan& p) {
  const PartialRequest& rq = p.rq; const PartialArrays& d = p.d;
  if (rq.form == kFormRange) return;
  if (rq.resume())
    PCO_TIMED_LAUNCH("reads_finish_kernel", rq.stream, reads_finish_kernel, p.task_grid(), dim3(256), 0, rq.stream, (const PcoGfxDecodeTask*)d.tasks, (const RangeRef*)d.ranges,
                     (const ReadRef*)d.curs, (const ReadRec*)d.recs, p.d_results, p.n());
  else
    PCO_TIMED_LAUNCH("index_finish_kernel", rq.stream, index_finish_kernel, dim3((uint32_t)std::min<size_t>(rq.n_tasks, 65535)), dim3(256), 0, rq.stream, (const PcoGfxDecodeTask*)d.tasks,
                     (const DecPlan*)p.d_plans, (const IndexRef*)d.irefs, p.d_results, p.n());
  PCO_HIP_CHECK(hipGetLastError());
  if (rq.synchronous()) read_results(p);
}

// The driver of every partial-decode entry point.
void launch_partial(const PartialRequest& rq) {
  if (rq.n_tasks == 0) return;
  if (rq.n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, rq.form_word() + "too many tasks"};
  PartialPlan p(rq);
  plan_tasks(p);
  upload(p);
  plan_take(p);
  resolve_directory(p);
  read_start_rows(p);
  size_walk(p);
  run_fast_route(p);
  if (run_scratch_route(p)) finish(p);
}

// checked tasks -> the call's return value
PcoError run_partial(const PartialRequest& rq) {
  if (rq.n_tasks == 0) return PcoSuccess;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
  { WorkspaceUse use(workspace(), rq.stream); launch_partial(rq); }
  if (rq.results) for (size_t i = 0; i < rq.n_tasks; i++) if (rq.results[i].status != PCO_GFX_OK) {
    set_error((int)rq.results[i].status, rq.what + " task " + std::to_string(i) + " failed");
    return PcoDecompressionError;
  }
  return PcoSuccess;
}

}  // namespace
}  // namespace pcogfx
