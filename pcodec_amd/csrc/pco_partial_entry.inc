// pco_partial_entry.inc -- the extern "C" entry points of the partial decode (include/pco_gfx.h sections 4d to 4l): each names its words and hands
// its arguments to partial_entry, which checks them, fills a PartialRequest and runs the driver of pco_partial_driver.inc.
// Every argument is checked before anything is launched (and before a device is asked for), in the order of the header's lists: the flags, the task
// array, the directory, the results, then task by task the fields every task has, the index fields, the history fields.  That order is part of the
// tested ABI, and so are the words of the refusals.

namespace pcogfx {
namespace {
// What an extern "C" function hands partial_entry.  `call` heads the refusals of the call's own arguments ("page reads with histories: unknown
// flags"); `stem` names a task ("page read task 3: ...", in a _dir form "directory page read task 3: ...") and the call in its failure report.
// kind: a _dir form takes a directory, and refuses a missing one -- and missing results -- even without tasks; the pointer forms do not.  In a chunk
// directory each task's one piece is a standalone chunk (section 4l).
enum EntryKind { kPointerForm, kPageDirForm, kChunkDirForm };
struct Entry {
  std::string call, stem; EntryKind kind;
  size_t n_tasks; const PcoGfxDirectory* dir; uint32_t flags; PcoGfxTaskResult* results; PcoGfxTaskResult* d_results; void* stream;
  DirLaunch dl{};   // (a _dir form) the checked directory, then the tasks' piece pairs
  bool dir_form() const { return kind != kPointerForm; }
  std::string what() const { return dir_form() ? "directory " + stem : stem; }
  std::string who(size_t i) const { return what() + " task " + std::to_string(i); }
};

// the call's own arguments
void check_call(Entry& e, const void* tasks) {
  if (e.flags & ~(uint32_t)PCO_GFX_CURSOR_GENERAL) throw HostError{PCO_GFX_INVALID_ARGUMENT, e.call + ": unknown flags"};   // (the range forms take none: 0)
  if (e.n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, e.call + ": null task array"};
  if (e.dir_form()) e.dl = DirLaunch{checked_directory(e.dir, e.stem.c_str()), nullptr, e.kind == kChunkDirForm};
  if ((e.dir_form() || e.n_tasks) && !e.results && !e.d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, e.call + ": results and d_results are both null"};
}

// the task structs, by what they have
template <class T, class... Us> constexpr bool kIsOneOf = (std::is_same<T, Us>::value || ...);
template <class T> constexpr bool kDirTask = kIsOneOf<T, PcoGfxDirPageRangeTask, PcoGfxDirPageReadTask, PcoGfxDirPageIndexTask>;        // pieces in place of pointers
template <class T> constexpr bool kIndexTask = kIsOneOf<T, PcoGfxPageIndexTask, PcoGfxPageIndexHistTask, PcoGfxDirPageIndexTask>;      // cursors and every_rows in place of dst and rows
template <class T> constexpr bool kReadTask = kIsOneOf<T, PcoGfxPageReadTask, PcoGfxPageReadHistTask, PcoGfxDirPageReadTask>;          // from / to
template <class T> constexpr bool kHistoryTask = kIsOneOf<T, PcoGfxPageReadHistTask, PcoGfxDirPageReadTask>;                           // history, history_len
template <class T> constexpr bool kHistoriesTask = kIsOneOf<T, PcoGfxPageIndexHistTask, PcoGfxDirPageIndexTask>;                       // histories, history_stride

// Any task as the driver takes it.  A directory task has no pointers; an index task has no dst, and its rows -- {0, k * every_rows} -- once its
// index fields are checked.
template <class T> PcoGfxPageRangeTask range_view(const T& t) {
  PcoGfxPageRangeTask r{nullptr, 0, nullptr, 0, nullptr, t.page_n, 0, 0, t.dtype, t.format_major};
  if constexpr (!kDirTask<T>) { r.meta = t.meta; r.meta_len = t.meta_len; r.page = t.page; r.page_len = t.page_len; }
  if constexpr (!kIndexTask<T>) { r.dst = t.dst; r.first = t.first; r.count = t.count; }
  return r;
}

// Task i of a call, for the checks below.  A refusal's words -- "<who>: <why>" -- are built only when a check fires: a call of several thousand good
// tasks builds no string.
struct TaskAt {
  const Entry& e; size_t i;
  [[noreturn]] void refuse(int status, const char* why) const { throw HostError{status, e.who(i) + ": " + why}; }
  [[noreturn]] void invalid(const char* why) const { refuse(PCO_GFX_INVALID_ARGUMENT, why); }
};

// One task's fields, each checked at one place.  The fields every task has, on its range view; a _dir form checks its piece pair against n_pieces in
// place of the meta / page pointers it has not got.
void check_partial_task(const TaskAt& at, const PcoGfxPageRangeTask& t) {
  const Entry& e = at.e;
  if (t.format_major > 4) at.refuse(PCO_GFX_CORRUPTION, "the file's format version definitely cannot be decompressed");   // wrapped/file_decompressor.rs:31-36
  if (e.kind == kChunkDirForm) check_chunk_piece(e.dl.pieces[at.i].meta_piece, e.dl.pieces[at.i].page_piece, e.dl.args.n_pieces, e.who(at.i));
  else if (e.dir_form()) check_piece_pair(e.dl.pieces[at.i].meta_piece, e.dl.pieces[at.i].page_piece, e.dl.args.n_pieces, e.who(at.i));
  else if (t.meta == nullptr || t.page == nullptr) at.invalid("null ChunkMeta or page");
  if (width_group(t.dtype) < 0) at.invalid("invalid number type");
  if (t.page_n == 0 || t.page_n > kMaxEntries) at.invalid("a page holds 1 ..= 2^24 numbers");
  if (t.first > t.page_n || t.count > t.page_n - t.first) at.invalid("rows beyond the page");
  if (t.count > 0 && t.dst == nullptr) at.invalid("null dst");
}

// an index task's every_rows and cursors: where its k cursors go, and its rows into the range view (< page_n: the walk never reaches the page's last batch)
template <class T> IndexRef checked_index_fields(const TaskAt& at, const T& t, PcoGfxPageRangeTask& r) {
  if (t.every_rows == 0 || (t.every_rows & 255u) != 0) at.invalid("every_rows is a positive multiple of 256");
  const uint64_t k = index_len(t.page_n, t.every_rows);
  if (k > 0 && (t.cursors == nullptr || ((uintptr_t)t.cursors & 7u) != 0)) at.invalid("null or misaligned cursors");
  r.count = k * t.every_rows;
  return IndexRef{k ? t.cursors->w : nullptr, (uint32_t)(k ? t.every_rows >> 8 : 0), (uint32_t)k};
}

// a read task's history and its length
template <class T> HistRef checked_history_pair(const TaskAt& at, const T& t) {
  if ((t.history == nullptr) != (t.history_len == 0)) at.invalid("a history and its length go together");
  if (((uintptr_t)t.history & 7u) != 0) at.invalid("misaligned history");
  return HistRef{t.history, t.history_len};
}

// an index task's histories and their stride; a task without cursors (k == 0) has no histories either
template <class T> IndexHistRef checked_index_histories(const TaskAt& at, const T& t, uint32_t k) {
  if ((t.histories == nullptr) != (t.history_stride == 0)) at.invalid("histories and their stride go together");
  if ((t.history_stride & 7u) != 0) at.invalid("the stride is a multiple of 8");
  if (((uintptr_t)t.histories & 7u) != 0) at.invalid("misaligned histories");
  return k ? IndexHistRef{t.histories, t.history_stride} : IndexHistRef{nullptr, 0};
}

// Every entry point: the call's checks, then each task's in the order above, then the driver.  A range task IS the driver's view and is passed through;
// every other task struct is turned into one.  What a task struct does not have is not checked and not passed on: pco_gfx_decompress_page_reads_ex
// passes no history array, so its calls keep the kernels without kHist; an index call in which no task has histories passes none either, and is the
// _ex call -- the same kernels, the same arguments.
template <class T>
PcoError partial_entry(Entry e, const T* tasks) {
  constexpr bool kIsView = std::is_same<T, PcoGfxPageRangeTask>::value;
  clear_error();
  try {
    check_call(e, tasks);
    const size_t n = e.n_tasks;
    std::vector<PcoGfxPageRangeTask> rt(kIsView ? 0 : n); std::vector<DirPieces> pieces(kDirTask<T> ? n : 0);
    std::vector<ReadRef> cursors(kReadTask<T> ? n : 0); std::vector<HistRef> hist(kHistoryTask<T> ? n : 0);
    std::vector<IndexRef> index(kIndexTask<T> ? n : 0); std::vector<IndexHistRef> ihist(kHistoriesTask<T> ? n : 0);
    e.dl.pieces = pieces.data();
    const PcoGfxPageRangeTask* view = rt.data();
    if constexpr (kIsView) view = tasks;
    bool any_histories = false;
    for (size_t i = 0; i < n; i++) {
      const T& t = tasks[i]; const TaskAt at{e, i};
      if constexpr (!kIsView) rt[i] = range_view(t);
      if constexpr (kDirTask<T>) pieces[i] = DirPieces{t.meta_piece, t.page_piece};
      if constexpr (kReadTask<T>) cursors[i] = ReadRef{t.from ? t.from->w : nullptr, t.to ? t.to->w : nullptr};
      check_partial_task(at, view[i]);
      if constexpr (kIndexTask<T>) index[i] = checked_index_fields(at, t, rt[i]);
      if constexpr (kHistoryTask<T>) hist[i] = checked_history_pair(at, t);
      if constexpr (kHistoriesTask<T>) { ihist[i] = checked_index_histories(at, t, index[i].k); any_histories = any_histories || ihist[i].histories != nullptr; }
    }
    return run_partial(PartialRequest{kIndexTask<T> ? kFormIndex : (kReadTask<T> ? kFormResume : kFormRange), e.what(), n, view, kReadTask<T> ? cursors.data() : nullptr,
                                      kIndexTask<T> ? index.data() : nullptr, kHistoryTask<T> ? hist.data() : nullptr, any_histories ? ihist.data() : nullptr,
                                      e.dir_form() ? &e.dl : nullptr, e.flags, e.results, e.d_results, (hipStream_t)e.stream});
  } catch (const HostError& err) { set_error(err.status, err.msg); return PcoDecompressionError; }
}
}  // namespace
}  // namespace pcogfx

using namespace pcogfx;
// include/pco_gfx.h section 4d
extern "C" enum PcoError pco_gfx_decompress_page_ranges(size_t n_tasks, const PcoGfxPageRangeTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page ranges", "page range", kPointerForm, n_tasks, nullptr, 0, results, d_results, stream}, tasks);
}

// section 4e
extern "C" enum PcoError pco_gfx_decompress_page_ranges_dir(size_t n_tasks, const PcoGfxDirPageRangeTask* tasks, const PcoGfxDirectory* dir, PcoGfxTaskResult* results,
                                                            PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page range directory", "page range", kPageDirForm, n_tasks, dir, 0, results, d_results, stream}, tasks);
}

// section 4f: a read task is a range task and its two cursors
extern "C" enum PcoError pco_gfx_decompress_page_reads_ex(size_t n_tasks, const PcoGfxPageReadTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page reads", "page read", kPointerForm, n_tasks, nullptr, flags, results, d_results, stream}, tasks);
}
extern "C" enum PcoError pco_gfx_decompress_page_reads(size_t n_tasks, const PcoGfxPageReadTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return pco_gfx_decompress_page_reads_ex(n_tasks, tasks, 0, results, d_results, stream);
}

// section 4i: a read task and its history buffer
extern "C" size_t pco_gfx_lookback_history_bytes(uint32_t window_n_log, unsigned char dtype) {
  return width_group(dtype) < 0 ? 0 : (size_t)history_bytes(window_n_log, (uint32_t)(dtype_bits(dtype) / 8));
}
extern "C" enum PcoError pco_gfx_decompress_page_reads_hist(size_t n_tasks, const PcoGfxPageReadHistTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page reads with histories", "page read", kPointerForm, n_tasks, nullptr, flags, results, d_results, stream}, tasks);
}

// section 4g: an index task is the range task {first 0, count k * every_rows} without a dst, and where its k cursors go
extern "C" size_t pco_gfx_page_index_len(uint64_t page_n, uint64_t every_rows) { return (size_t)index_len(page_n, every_rows); }
extern "C" enum PcoError pco_gfx_index_pages_ex(size_t n_tasks, const PcoGfxPageIndexTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page index", "page index", kPointerForm, n_tasks, nullptr, flags, results, d_results, stream}, tasks);
}
extern "C" enum PcoError pco_gfx_index_pages(size_t n_tasks, const PcoGfxPageIndexTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return pco_gfx_index_pages_ex(n_tasks, tasks, 0, results, d_results, stream);
}

// section 4j: an index task and where its k histories go
extern "C" enum PcoError pco_gfx_index_pages_hist(size_t n_tasks, const PcoGfxPageIndexHistTask* tasks, uint32_t flags, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page index with histories", "page index", kPointerForm, n_tasks, nullptr, flags, results, d_results, stream}, tasks);
}

// section 4k: 4i's read entry point and 4j's index entry point with each task's ChunkMeta and page named by piece index.  The directory's verdicts are
// the resolve kernel's (dir_resolve.hip), and everything behind it is the pointer form's call.
extern "C" int pco_gfx_lookback_window_n_log(uint64_t n) {   // delta/mod.rs:37-48, pco_encode_config.inc lookback_window_log
  if (n == 0 || n > kMaxEntries) return 0;
  int b = 0;
  while (((uint64_t)1 << b) < n) b++;   // ceil(log2(n))
  return b < 4 ? 4 : (b > 15 ? 15 : b);
}
extern "C" enum PcoError pco_gfx_decompress_page_reads_dir(size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                           PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page read directory", "page read", kPageDirForm, n_tasks, dir, flags, results, d_results, stream}, tasks);
}
extern "C" enum PcoError pco_gfx_index_pages_dir(size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                 PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"page index directory", "page index", kPageDirForm, n_tasks, dir, flags, results, d_results, stream}, tasks);
}

// section 4l: the same two with each task's one piece a standalone chunk behind pco_gfx_compact_chunks' offsets.  Nothing else differs on the host
extern "C" enum PcoError pco_gfx_decompress_chunk_reads_dir(size_t n_tasks, const PcoGfxDirPageReadTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                            PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"chunk read directory", "chunk read", kChunkDirForm, n_tasks, dir, flags, results, d_results, stream}, tasks);
}
extern "C" enum PcoError pco_gfx_index_chunks_dir(size_t n_tasks, const PcoGfxDirPageIndexTask* tasks, const PcoGfxDirectory* dir, uint32_t flags,
                                                  PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  return partial_entry(Entry{"chunk index directory", "chunk index", kChunkDirForm, n_tasks, dir, flags, results, d_results, stream}, tasks);
}
