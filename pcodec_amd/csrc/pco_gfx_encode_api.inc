// pco_gfx_encode_api.inc -- run_encode, the host driver of every encode entry point (included by pco_gfx.hip): one EncodeCall context and one
// function per phase of the pipeline, in launch order.
namespace pcogfx {

// PCO_GFX_TRACE=1: wall-clock of the host phases of an encode call on stderr (each phase is followed by a stream synchronise, so
// the numbers are not what an untraced call pays for overlap-able work)
static const bool g_trace = std::getenv("PCO_GFX_TRACE") != nullptr;
struct TracePhase {
  const char* name; hipStream_t stream; std::chrono::steady_clock::time_point t0;
  TracePhase(const char* n, hipStream_t s) : name(n), stream(s) { if (g_trace) { (void)hipStreamSynchronize(s); t0 = std::chrono::steady_clock::now(); } }
  ~TracePhase() { if (g_trace) { (void)hipStreamSynchronize(stream); fprintf(stderr, "[pco_gfx trace] %-28s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); } }
};

// device counter of the (chunk, variable) histograms whose literal replay reached the reference's heapsort branch (strict mode)
static uint32_t* strict_fell_back_counter(hipStream_t stream) {
  Workspace& w = workspace();
  if (!w.enc_strict.p) { w.enc_strict.ensure(256); PCO_HIP_CHECK(hipMemsetAsync(w.enc_strict.p, 0, 256, stream)); }
  return (uint32_t*)w.enc_strict.p;
}

// One pass of the encode pipeline: what it was called with, the call-wide facts (computed once, here), and what the phases hand on to one another.
struct EncodeCall {
  const size_t n_tasks; const PcoGfxEncodeTask* const tasks; const std::vector<EncModePlan>& plans; const std::vector<EncPage>& pages; const ResolvedConfig& cfg;
  PcoGfxTaskResult* const results; const hipStream_t stream; const int stop_after;   // stop_after: 1 = split, 2 = train
  Workspace& wsp;
  // the call-wide facts
  uint64_t n_max = 0, page_max = 0;
  bool any_sec = false, any_lookback = false, any_conv1 = false;
  bool any_big = false;     // a chunk histograms into more than 256 bins (levels 9..12 on chunks of >= 2^13 numbers)
  uint32_t widths = 0;      // the number widths of the call's chunks: 8 | 16 | 32 | 64
  const bool lat_exact;     // a synchronous call: the full-width latent slots are counted on the device and read back
  const uint32_t nt, np;
  // filled by the phases
  EncWorkspace ws{};        // what the kernels take (by value, as it stands at each launch)
  PcoGfxEncodeTask* d_tasks = nullptr; EncModePlan* d_plans = nullptr; PcoGfxTaskResult* d_results = nullptr;
  size_t lat_slot_bytes = 0, sort_bytes = 0; bool sort_upfront = false;
  uint32_t c16_enable = 0, tiles_per_page = 0;
  bool any_full0 = false, any_spec = false;   // chunks that do not / do speculate on 16-bit latents
  uint32_t n_full = 0;                        // chunks that never speculate (synchronous calls: exact)

  EncodeCall(size_t n, const PcoGfxEncodeTask* t, const std::vector<EncModePlan>& pl, const std::vector<EncPage>& pg, const ResolvedConfig& c, PcoGfxTaskResult* res, hipStream_t s, int stop)
      : n_tasks(n), tasks(t), plans(pl), pages(pg), cfg(c), results(res), stream(s), stop_after(stop), wsp(workspace()), lat_exact(res != nullptr), nt((uint32_t)n), np((uint32_t)pg.size()) {
    for (size_t i = 0; i < n_tasks; i++) {
      n_max = std::max<uint64_t>(n_max, tasks[i].n);
      any_sec |= plans[i].mode_kind != kClassic; any_lookback |= plans[i].delta_kind == kDeltaLookback; any_conv1 |= plans[i].delta_kind == kDeltaConv1;
      any_big |= (plans[i].ubl_override != 0xffffffffu ? plans[i].ubl_override : choose_unoptimized_bins_log(cfg.level, tasks[i].n)) > kMaxUnoptBinsLog;
      widths |= (uint32_t)dtype_bits(tasks[i].dtype);
    }
    for (auto& p : pages) page_max = std::max<uint64_t>(page_max, p.n);
  }
};

// Phase 1: the workspace carved into the kernels' arrays, the tasks, plans and pages uploaded.
static void encode_carve_and_upload(EncodeCall& c, PcoGfxTaskResult* d_results_user) {
  Workspace& wsp = c.wsp; EncWorkspace& ws = c.ws; const size_t n_tasks = c.n_tasks, n_pages = c.pages.size(); const hipStream_t stream = c.stream;
  wsp.lb_n = 0;   // (pco_gfx_debug_lookback_routes speaks of THIS pass: set again by the lookback phase if it has lookback pages)
  ws.dict = c.cfg.d_dict;
  ws.n_stride = ((c.n_max + 255) & ~(uint64_t)255) + 256;
  ws.n_slots = 0;
  ws.slot_of_var[0] = c.any_lookback ? ws.n_slots++ : 0xffffffffu;
  ws.slot_of_var[1] = ws.n_slots++;
  ws.slot_of_var[2] = c.any_sec ? ws.n_slots++ : 0xffffffffu;
  const size_t state_bytes = n_tasks * sizeof(EncChunk) + 256;
  // bin capacity of the plan regions: 4096 as soon as one chunk histograms into more than 256 bins (levels 9..12 on chunks of >= 2^13 numbers)
  ws.plan_cap = c.any_big ? kBigBins : kMaxBins;
  const size_t plan_bytes = n_tasks * 3 * plan_bytes_for(ws.plan_cap);
  const size_t off_plans = (n_tasks * sizeof(PcoGfxEncodeTask) + 63) & ~(size_t)63;
  const size_t off_pages = (off_plans + n_tasks * sizeof(EncModePlan) + 63) & ~(size_t)63;
  const size_t off_flags = (off_pages + n_pages * sizeof(EncPage) + 63) & ~(size_t)63;
  const size_t off_slots = off_flags + 64;
  uint8_t* d_small = (uint8_t*)wsp.enc_small.ensure(off_slots + n_tasks * sizeof(uint32_t) + 256);
  ws.need_sort = (uint32_t*)(d_small + off_flags);
  ws.need_full0 = ws.need_sort + 1;
  ws.lat_used = ws.need_sort + 2;
  ws.lat_slot = (uint32_t*)(d_small + off_slots);
  PCO_HIP_CHECK(hipMemsetAsync(ws.need_sort, 0, 12, stream));
  PCO_HIP_CHECK(hipMemsetAsync(ws.lat_slot, 0xff, n_tasks * sizeof(uint32_t), stream));
  c.d_tasks = (PcoGfxEncodeTask*)d_small;
  c.d_plans = (EncModePlan*)(d_small + off_plans);
  ws.pages = (EncPage*)(d_small + off_pages);
  wsp.pack_np = n_pages; wsp.pack_pages_off = off_pages;   // (pco_gfx_debug_pack_routes speaks of THIS pass)
  uint8_t* d_state = (uint8_t*)wsp.enc_state.ensure(state_bytes + plan_bytes);
  ws.chunks = (EncChunk*)d_state;
  ws.plans = d_state + ((n_tasks * sizeof(EncChunk) + 255) & ~(size_t)255);
  wsp.hist_nt = n_tasks; wsp.hist_plans_off = (size_t)(ws.plans - d_state); wsp.hist_plan_cap = ws.plan_cap;   // (pco_gfx_debug_histogram speaks of THIS pass)
  // Full-width latents (8 B per number and variable) are scratch of the chunks that do not get by with 16-bit latents.  Which chunks those are
  // is decided on the device (enc_init_kernel, enc_presample_kernel, the 16-bit split itself), so the slots are handed out there
  // (enc_lat_slots_kernel).  A synchronous call reads the count back twice -- behind the sample and behind the 16-bit split, where it waits for
  // the device anyway or for 4 bytes more -- and allocates exactly that: nothing to speak of on data whose deltas are narrow (the headline),
  // everything for lookback.  An asynchronous call cannot wait and takes a slot per chunk up front.
  ws.lat_esz = (c.widths & 64u) ? 8 : 4;
  c.lat_slot_bytes = (size_t)ws.n_slots * ws.n_stride * ws.lat_esz;
  ws.lat = nullptr; ws.lat2 = nullptr; ws.lat_cap1 = 0;
  if (!c.lat_exact) { ws.lat_cap1 = (uint32_t)n_tasks; ws.lat = (uint8_t*)wsp.enc_lat.ensure(n_tasks * c.lat_slot_bytes); ws.lat2 = ws.lat; }
  // The two 8-byte-per-number sort buffers are only touched by lookback staging and by the radix-sort histogram; whether the
  // latter is needed is known on the device after the split.  Synchronous calls ask (one 4-byte read-back) and allocate on
  // demand; asynchronous calls (no host results) cannot wait and allocate up front.
  c.sort_bytes = n_tasks * 2 * ws.n_stride * ws.lat_esz;
  c.sort_upfront = c.any_lookback || c.any_conv1 || c.results == nullptr || c.stop_after != 0 || c.cfg.strict_hist;   // (the strict histogram permutes a copy of every variable in the sort buffers)
  ws.sort = c.sort_upfront ? (uint8_t*)wsp.enc_sort.ensure(c.sort_bytes) : (uint8_t*)wsp.enc_sort.p;
  ws.dissect = (uint32_t*)wsp.enc_ans.ensure(n_tasks * ws.n_slots * ws.n_stride * 4);
  c.d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)wsp.results.ensure(n_pages * sizeof(PcoGfxTaskResult));
  PCO_HIP_CHECK(hipMemcpyAsync(c.d_tasks, c.tasks, n_tasks * sizeof(PcoGfxEncodeTask), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(c.d_plans, c.plans.data(), n_tasks * sizeof(EncModePlan), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(ws.pages, c.pages.data(), n_pages * sizeof(EncPage), hipMemcpyHostToDevice, stream));
}

// Phase 2: the chunk records, the 64-position sample that takes hopeless chunks out of the 16-bit speculation, and the first hand-out of
// full-width latent slots -- which a synchronous call reads back and allocates exactly.
static void encode_init_and_latent_slots(EncodeCall& c) {
  EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const uint32_t nt = c.nt;
  c.c16_enable = c.stop_after != 1 ? 1u : 0u;   // speculative 16-bit latents (the Auto-delta sampling reads the full-width latents back)
  PCO_TIMED_LAUNCH("enc_init_kernel", stream, enc_init_kernel, dim3((nt + 63) / 64), dim3(64), 0, stream, ws, c.d_tasks, c.d_plans, nt, c.cfg.level, c.c16_enable);
  c.tiles_per_page = (uint32_t)std::max<uint64_t>((c.page_max + kSplitTile - 1) / kSplitTile, 1);
  if ((uint64_t)c.np * c.tiles_per_page >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many pages in one call"};
  c.any_spec = c.c16_enable != 0;
  c.any_full0 = !c.c16_enable || c.any_lookback || c.any_big;   // (chunks with more than 256 bins never speculate on 16-bit latents)
  if (c.c16_enable) PCO_TIMED_LAUNCH("enc_presample_kernel", stream, enc_presample_kernel, dim3(nt), dim3(64), 0, stream, ws, c.d_tasks, nt);   // a 64-position sample takes hopeless chunks out of the speculation up front
  PCO_TIMED_LAUNCH("enc_lat_slots_kernel", stream, enc_lat_slots_kernel, dim3((nt + 63) / 64), dim3(64), 0, stream, ws, nt, 0u);
  if (c.lat_exact) {   // synchronous call: ask how many slots are gone, i.e. how many chunks write full-width latents from the start (12 bytes); asynchronous calls launch every kernel regardless
    uint32_t flags[3] = {0, 0, 0};
    PCO_HIP_CHECK(hipMemcpyAsync(flags, ws.need_sort, 12, hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
    c.n_full = flags[2];
    c.any_full0 = c.n_full != 0; c.any_spec = c.c16_enable && c.n_full < c.n_tasks;
    ws.lat_cap1 = std::max<uint32_t>(c.n_full, 1u);
    ws.lat = (uint8_t*)c.wsp.enc_lat.ensure((size_t)ws.lat_cap1 * c.lat_slot_bytes);
    ws.lat2 = ws.lat;
  } else if (c.c16_enable) c.any_full0 = true;
}

// Phase 3: the split into latent variables -- speculating on 16-bit latents, at full width, and once more at full width for the chunks whose
// speculation failed.
static void encode_split(EncodeCall& c) {
  EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const uint32_t nt = c.nt, np = c.np, tiles_per_page = c.tiles_per_page;
  if (c.any_spec) PCO_TIMED_LAUNCH("enc_split_kernel<c16>", stream, (enc_split_kernel<true, false>), dim3(np * tiles_per_page), dim3(256), kSplitLdsBytes, stream, ws, c.d_tasks, tiles_per_page, 1u, 1u);
  if (c.any_full0) PCO_TIMED_LAUNCH("enc_split_kernel", stream, (enc_split_kernel<false, false>), dim3(np * tiles_per_page), dim3(256), kSplitLdsBytes, stream, ws, c.d_tasks, tiles_per_page, 1u, 0u);
  if (!c.any_spec) return;
  // the chunks whose speculation failed
  PCO_TIMED_LAUNCH("enc_lat_slots_kernel", stream, enc_lat_slots_kernel, dim3((nt + 63) / 64), dim3(64), 0, stream, ws, nt, 2u);
  bool any_redo = true;
  if (c.lat_exact) {
    uint32_t used = 0;
    PCO_HIP_CHECK(hipMemcpyAsync(&used, ws.lat_used, 4, hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
    const uint32_t n_redo = used > ws.lat_cap1 ? used - ws.lat_cap1 : 0u;   // (lat_cap1 is max(slots of the first hand-out, 1): with none handed out yet, slot 0 is the first redo chunk's and lies in lat)
    any_redo = used > c.n_full;
    if (n_redo) ws.lat2 = (uint8_t*)c.wsp.enc_lat2.ensure((size_t)n_redo * c.lat_slot_bytes);
  }
  if (any_redo) {
    const uint32_t tpb = 32, bpp = (tiles_per_page + tpb - 1) / tpb;
    PCO_TIMED_LAUNCH("enc_split_kernel(redo)", stream, (enc_split_kernel<false, true>), dim3(np * bpp), dim3(256), kSplitLdsBytes, stream, ws, c.d_tasks, tiles_per_page, tpb, 2u);
  }
}

// Phase 4: Conv1 delta (encode_conv1.hip): the fit over each whole chunk, then the residuals page by page.
static void encode_conv1(EncodeCall& c) {
  if (!c.any_conv1) return;
  EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const uint32_t nt = c.nt;
  const size_t conv_bytes = (c.n_tasks * sizeof(EncConv) + 255) & ~(size_t)255;
  uint8_t* d_conv = (uint8_t*)c.wsp.enc_conv.ensure(conv_bytes + c.pages.size() * kConv1MaxOrder * sizeof(uint32_t) + 256);
  ws.conv = (EncConv*)d_conv; ws.conv_state = (uint32_t*)(d_conv + conv_bytes);
  PCO_TIMED_LAUNCH("enc_conv1_stats_kernel", stream, enc_conv1_stats_kernel, dim3(nt), dim3(kConv1Threads), 0, stream, ws, nt);
  PCO_TIMED_LAUNCH("enc_conv1_solve_kernel", stream, enc_conv1_solve_kernel, dim3(nt), dim3(64), 0, stream, ws, nt);
  PCO_TIMED_LAUNCH("enc_conv1_resid_kernel", stream, enc_conv1_resid_kernel, dim3(c.np * c.tiles_per_page), dim3(kConv1Threads), 0, stream, ws, c.tiles_per_page);
}

// Phase 5: the lookback search over the pages of the chunks with a lookback delta (encode_lookback.hip).
static void encode_lookback(EncodeCall& c) {
  if (!c.any_lookback) return;
  Workspace& wsp = c.wsp; const EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const uint64_t page_max = c.page_max;
  // per page: last-index hash tables (2 x 2^(w+1) u32) + lookback counts (2^w u32); w <= 15
  uint32_t wmax = 4; for (size_t i = 0; i < c.n_tasks; i++) if (c.plans[i].delta_kind == kDeltaLookback) wmax = std::max(wmax, c.plans[i].window_n_log);
  const uint64_t stride_u32 = (4ull << wmax) + (1ull << wmax) + 64;
  std::vector<uint32_t> lb_pages;
  uint64_t page_min_lb = ~0ull;
  for (size_t pi = 0; pi < c.pages.size(); pi++) if (c.plans[c.pages[pi].chunk].delta_kind == kDeltaLookback && !(c.pages[pi].flags & kPageFlagMetaOnly)) { lb_pages.push_back((uint32_t)pi); page_min_lb = std::min<uint64_t>(page_min_lb, c.pages[pi].n); }
  const uint32_t n_lb = (uint32_t)lb_pages.size();
  if (!n_lb) return;
  uint32_t* d_lb = (uint32_t*)wsp.enc_lb.ensure((size_t)n_lb * stride_u32 * 4 + (size_t)n_lb * 12 + 256);   // tables and counts per page, then the page ids, the redo list and the pre-pass's skip list
  uint32_t* d_ids = d_lb + (size_t)n_lb * stride_u32;
  PCO_HIP_CHECK(hipMemcpyAsync(d_ids, lb_pages.data(), (size_t)n_lb * 4, hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns, like the task arrays)
  // The hash proposals as a pre-pass with the page's tables in LDS (enc_lookback_hash_kernel), then the four-wave pipeline per page fed
  // from their streams (encode_lookback.hip).  The pipeline hands pages on which its speculation keeps failing back to the one-wave-per-page
  // kernel, which therefore always runs behind it.
  uint32_t* redo = d_ids + n_lb;
  uint32_t* d_skip = redo + n_lb;
  wsp.lb_n = n_lb; wsp.lb_redo_off = (size_t)(redo - d_lb); wsp.lb_skip_off = (size_t)(d_skip - d_lb);
  const bool small = page_max <= kLbPipeSmallMaxPage && wmax <= 13;
  const uint64_t prop_stride = ((page_max + 63) & ~(uint64_t)63) + 64;
  uint16_t* d_props = (uint16_t*)wsp.enc_lbprops.ensure((size_t)n_lb * 6 * prop_stride * 2 + 256);
  PCO_RESERVE_LDS(enc_lookback_hash_kernel, lh_lds_bytes(15), "enc_lookback_hash_kernel");
  PCO_TIMED_LAUNCH("enc_lookback_hash_kernel", stream, enc_lookback_hash_kernel, dim3(2 * n_lb), dim3(kLhThreads), lh_lds_bytes(std::min(wmax, 15u)), stream, ws, (const uint32_t*)d_ids, n_lb, d_props, prop_stride, lh_queue_off(std::min(wmax, 15u)), d_skip);
  // page slots: four per CU, the pages dealt out in equal rounds.  Throughput stops growing there: a CU gets through one tile's stage work
  // per ~5 k cycles however many pages share it (scripts/lb_scaling.py).
  int n_cu = 256; { int dev = 0; hipDeviceProp_t pr; if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) n_cu = pr.multiProcessorCount; }
  const uint32_t per_round = 4u * (uint32_t)n_cu, rounds = (n_lb + per_round - 1) / per_round;
  const uint32_t slots = std::min((n_lb + rounds - 1) / rounds, n_lb);
  typedef LbPipe<false, true, true> PipeF; typedef LbPipe<true, true, true> PipeSF;
  if (small) PCO_TIMED_LAUNCH("enc_lookback_pipe_kernel<small,props,fastd>", stream, (enc_lookback_pipe_kernel<PipeSF>), dim3(slots), dim3(PipeSF::kThreads), PipeSF::kLdsBytes, stream, ws, (const uint32_t*)d_ids, n_lb, d_lb, stride_u32, redo, (const uint16_t*)d_props, prop_stride, (const uint32_t*)d_skip);
  else PCO_TIMED_LAUNCH("enc_lookback_pipe_kernel<props,fastd>", stream, (enc_lookback_pipe_kernel<PipeF>), dim3(slots), dim3(PipeF::kThreads), PipeF::kLdsBytes, stream, ws, (const uint32_t*)d_ids, n_lb, d_lb, stride_u32, redo, (const uint16_t*)d_props, prop_stride, (const uint32_t*)d_skip);
  // the pages the pre-pass's screen took out (duplicate-heavy trial samples), element by element with everything in LDS
  if (page_min_lb <= kLbSeqMaxPage) {
    const uint32_t n_round = lbseq_round((uint32_t)std::min<uint64_t>(page_max, kLbSeqMaxPage));
    PCO_TIMED_LAUNCH("enc_lookback_seq_kernel", stream, enc_lookback_seq_kernel, dim3(n_lb), dim3(64), lbseq_lds_bytes(n_round), stream, ws, (const uint32_t*)d_ids, n_lb, (const uint16_t*)d_props, prop_stride, (const uint32_t*)d_skip, redo, n_round);
  }
  if (page_max <= kLbSmallMaxPage) PCO_TIMED_LAUNCH("enc_lookback_kernel<small>", stream, (enc_lookback_kernel<LbSmall>), dim3(n_lb), dim3(64), LbSmall::kLbLdsBytes, stream, ws, (const uint32_t*)d_ids, n_lb, d_lb, stride_u32, redo);
  else PCO_TIMED_LAUNCH("enc_lookback_kernel", stream, (enc_lookback_kernel<LbFull>), dim3(n_lb), dim3(64), LbFull::kLbLdsBytes, stream, ws, (const uint32_t*)d_ids, n_lb, d_lb, stride_u32, redo);
}

// wide value ranges: the quantile-segmented bucket select over the chunks of one number width
struct HistSelectStep {
  const EncodeCall& c;
  template <class L>
  void launch() const {
    PCO_RESERVE_LDS(enc_hist_select_kernel<L>, kSelLdsBytes, "enc_hist_select_kernel");
    PCO_TIMED_LAUNCH("enc_hist_select_kernel", c.stream, enc_hist_select_kernel<L>, dim3(c.nt), dim3(kSelThr), kSelLdsBytes, c.stream, c.ws, c.nt);
  }
};

// Phase 6: the histograms, tier by tier of value range: the first counting tier for everybody, then the tiers that have anything to do.
static void encode_histograms(EncodeCall& c) {
  Workspace& wsp = c.wsp; EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const uint32_t nt = c.nt;
  PCO_TIMED_LAUNCH("enc_hist_kernel", stream, enc_hist_kernel, dim3(nt), dim3(256), kHistLdsBytes, stream, ws, nt);
  PCO_RESERVE_LDS(enc_hist_wide_kernel<kWideHistRange>, hist_lds_bytes(kWideHistRange), "enc_hist_wide_kernel");
  PCO_RESERVE_LDS(enc_hist_wide_kernel<kMidHistRange>, hist_lds_bytes(kMidHistRange), "enc_hist_wide_kernel");
  PCO_RESERVE_LDS(enc_hist_sort_kernel, kHistSortLdsBytes, "enc_hist_sort_kernel");
  // Which of the wider-range kernels have anything to do is known on the device once enc_hist_kernel has seen every variable's range:
  // synchronous calls ask (one 4-byte read-back) and launch only those; asynchronous calls launch them all (idle blocks leave at once,
  // but 8192 blocks of 1024 threads still cost 0.15 ms per kernel).
  // What the host knows without asking: a variable is never longer than its chunk, so a call of short chunks only (the Auto-delta
  // trial samples) has nothing for the select kernel; the whole-variable-in-LDS kernel's LDS is sized for the longest short chunk.
  uint32_t small_lds = 0;
  for (size_t i = 0; i < c.n_tasks; i++) {
    const uint32_t kb = dtype_bits(c.tasks[i].dtype) == 64 ? 8u : 4u;
    small_lds = std::max(small_lds, small_lds_bytes((uint32_t)std::min<uint64_t>(c.tasks[i].n, kSmallHistCap), kb));
  }
  const bool any_long = c.n_max > kSmallHistCap;   // (short variables never reach the 16 k / 32 k-counter kernels or the select kernel)
  bool run_mid = any_long, run_wide = any_long, run_sort = any_long || c.any_big, run_small = true;
  if (c.results != nullptr && c.stop_after == 0) {
    uint32_t flag = 0;
    PCO_HIP_CHECK(hipMemcpyAsync(&flag, ws.need_sort, 4, hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
    run_sort = (flag & 1u) != 0; run_mid = (flag & 2u) != 0; run_wide = (flag & 4u) != 0; run_small = (flag & 8u) != 0;
  }
  if (run_sort && !c.sort_upfront) ws.sort = (uint8_t*)wsp.enc_sort.ensure(c.sort_bytes);
  // the kernels with one or two big blocks per CU leave their bin walks (one thread's work, half their time) to enc_hist_walk_kernel
  if (run_mid || run_wide || run_small || run_sort) ws.walk = (uint8_t*)wsp.enc_walk.ensure((size_t)nt * 3 * kWalkRecBytes);
  if (run_mid) PCO_TIMED_LAUNCH("enc_hist_wide_kernel<16384>", stream, enc_hist_wide_kernel<kMidHistRange>, dim3(nt), dim3(1024), hist_lds_bytes(kMidHistRange), stream, ws, nt);
  if (run_wide) PCO_TIMED_LAUNCH("enc_hist_wide_kernel<32768>", stream, enc_hist_wide_kernel<kWideHistRange>, dim3(nt), dim3(1024), hist_lds_bytes(kWideHistRange), stream, ws, nt);
  if (run_small) {   // value ranges beyond the first counting tier, at most 8192 latents: ordered whole in LDS
    PCO_RESERVE_LDS(enc_hist_small_kernel, small_lds_bytes(kSmallHistCap, 8), "enc_hist_small_kernel");
    PCO_TIMED_LAUNCH("enc_hist_small_kernel", stream, enc_hist_small_kernel, dim3(nt), dim3(kSelT), small_lds, stream, ws, nt);
  }
  if (run_sort) {   // wide value ranges: quantile-segmented bucket select, one launch per number width of the call; the radix-sort kernel only sees what that one gave up on
    for (int g = 0; g < 4; g++) if (c.widths & (64u >> g)) launch_width(g, HistSelectStep{c});
    PCO_TIMED_LAUNCH("enc_hist_sort_kernel", stream, enc_hist_sort_kernel, dim3(nt), dim3(256), kHistSortLdsBytes, stream, ws, nt);
  }
  if (ws.walk != nullptr) PCO_TIMED_LAUNCH("enc_hist_walk_kernel", stream, enc_hist_walk_kernel, dim3(nt), dim3(64), kWalkLdsBytes, stream, ws, nt);
  // strict mode: the literal replay of histograms.rs overwrites the bins (encode_hist_literal.hip); everything else the kernels above left
  // behind (16-bit copies, ranges, paths) stands
  if (c.cfg.strict_hist) PCO_TIMED_LAUNCH("enc_hist_literal_kernel", stream, enc_hist_literal_kernel, dim3(nt), dim3(64), kLitLdsBytes, stream, ws, nt, strict_fell_back_counter(stream));
}

// Phase 7: bins, weights and tANS tables from the histograms.
static void encode_train(EncodeCall& c) {
  const hipStream_t stream = c.stream; const uint32_t nt = c.nt;
  PCO_TIMED_LAUNCH("enc_train_kernel", stream, enc_train_kernel, dim3(nt), dim3(64), kTrainLdsBytes, stream, c.ws, nt);
  if (c.any_big) {   // levels 9..12: chunks with more than 256 histogram bins
    PCO_RESERVE_LDS(enc_train_big_kernel, kTrainBigLdsBytes, "enc_train_big_kernel");
    PCO_TIMED_LAUNCH("enc_train_big_kernel", stream, enc_train_big_kernel, dim3(nt), dim3(1024), kTrainBigLdsBytes, stream, c.ws, nt);
  }
}

// LDS of the single-kernel page encoder: the variables' tables.  With more than 256 bins in play (levels 9..12) the worst case is two
// variables of 4096 bins (the secondary never has more than 64: wrapped/chunk_compressor.rs:238-248) next to a small one.
static uint32_t encode_page_lds(const EncodeCall& c) {
  const EncWorkspace& ws = c.ws;
  if (!c.any_big) return kPageLdsVar + ws.n_slots * page_var_bytes(c.cfg.level <= 8 ? 10 : kMaxEncTableLog);
  PCO_RESERVE_LDS(enc_page_kernel, 160 * 1024, "enc_page_kernel");
  return kPageLdsVar + std::min<uint32_t>(ws.n_slots, 2) * page_var_bytes(kMaxEncTableLog, kBigBins) + (ws.n_slots > 2 ? page_var_bytes(kMaxEncTableLog) : 0);
}

static void encode_pack(const EncodeCall& c, const EncFast& fx, uint64_t n_blocks, bool forked);   // (defined behind phase 8: the kernels are instantiated in the order of their first use)

// Phase 8, the common case: dissect / walk / scan / pack (encode_fast.hip); enc_page_kernel then only sees the rest.  Returns whether it ran.
static bool encode_fast_pages(EncodeCall& c) {
  Workspace& wsp = c.wsp; const EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const size_t n_tasks = c.n_tasks, n_pages = c.pages.size();
  const uint32_t nt = c.nt, np = c.np; const uint64_t page_max = c.page_max;
  EncFast fx{};
  const uint64_t max_batches = (page_max + kBatchN - 1) / kBatchN;
  fx.bat_stride = (uint32_t)max_batches + 1;
  fx.runs_per_page = (uint32_t)((max_batches + kRunBatches - 1) / kRunBatches); if (fx.runs_per_page == 0) fx.runs_per_page = 1;
  fx.run_stride = fx.runs_per_page + 1;
  uint32_t max_page_idx = 0; for (auto& pgi : c.pages) max_page_idx = std::max(max_page_idx, pgi.page_idx);
  fx.stride = ws.n_stride + 16ull * (max_page_idx + 1) + 64;
  fx.sym = (uint8_t*)wsp.enc_sym.ensure(n_tasks * ws.n_slots * fx.stride + 64);
  fx.answ = (uint16_t*)wsp.enc_answ.ensure(n_tasks * ws.n_slots * fx.stride * 2 + 64);
  fx.bat = (uint32_t*)wsp.enc_bat.ensure(n_pages * 3 * (size_t)fx.bat_stride * 8);
  fx.run_start = (uint64_t*)wsp.enc_run.ensure(n_pages * (size_t)fx.run_stride * 8);
  // (behind the final states, in the same buffer: the page body records and the block flags of enc_walkp_kernel)
  const size_t fstate_bytes = (n_pages * 12 * 4 + 63) & ~(size_t)63, body_bytes = (n_pages * 16 + 63) & ~(size_t)63, wpb_bytes = ((n_pages * (size_t)ws.n_slots + 15) / 16) * 4 + 64;
  fx.fstate = (uint32_t*)wsp.enc_fstate.ensure(fstate_bytes + body_bytes + wpb_bytes);
  const uint64_t n_blocks = (uint64_t)np * fx.runs_per_page;
  if (n_blocks >= (1ull << 31)) return false;
  const uint32_t n_items = np * ws.n_slots;
  // variables with 16-bit latents get their symbols from the second wave of the walker's block (enc_walkd_kernel) instead of enc_dissect_kernel:
  // all of them while 8192 items cover the launch, else those whose tables need the big slots
  // the value -> bin tables are 8 KB per (chunk, variable) whatever the chunk's length: a call of very many short chunks keeps enc_dissect_kernel instead
  const size_t vlut_bytes = n_tasks * (size_t)ws.n_slots * kDirectHistRange * 2;
  uint64_t input_bytes = 0; for (size_t i = 0; i < n_tasks; i++) input_bytes += c.tasks[i].n * (uint64_t)(dtype_bits(c.tasks[i].dtype) / 8);
  const bool lookups = vlut_bytes <= std::max<uint64_t>(64ull << 20, input_bytes / 2);
  // walk + pack in one block for the pages that qualify (encode_walkpack.hip); enc_walkd_kernel and the pack kernels take the rest.  PCO_GFX_WALKP=0: off
  static const bool walkp_on = env_not_zero("PCO_GFX_WALKP");
  // A launch of more than 8192 items used to be split by table size (round 5: the 16-per-wave walker for the tables that fit its slots, enc_walkd_kernel
  // for the rest -- two rounds of enc_walkd_kernel's blocks cost more).  enc_walkp_kernel's cost is per item (4.2 ms per 8192, 6.6 per 12 288), and a
  // block of it qualifies only when all sixteen of its items are its own: one-variable calls keep every item with the fused kernels at any size
  // (configs[1] at 12 288 chunks: walkp 7.3 + walkd 3.8 + walk16 4.1 ms became one walkp launch)
  const bool keep_fused = walkp_on && lookups && ws.n_slots == 1;
  fx.fused = n_items > 8192 && !keep_fused ? 2u : 1u;
  if (lookups) fx.fused |= kFusedLookups;
  // long page variables are walked sixteen segments side by side (enc_walkseg_kernel) while the call is small: the unsegmented walkers keep
  // 512 chains in flight whatever the call's size (3.4 ms per 2^18 latents, for 256 chunks as for 8192), the segmented one a block per item
  // -- 0.4 ms for 64 chunks, 0.75 for 1024, 2.2 for 3072, 3.0 for 4096 (where the two meet), but 6.4 for 8192: on a full chip the gathering
  // waves alone take 3.1 ms (profiles/r05_walkseg_scaling.txt)
  const bool any_seg = page_max >= (uint64_t)kWsMinBatches * kBatchN && n_items <= kWsMaxItems;
  if (any_seg) fx.fused |= kFusedSegments;
  PCO_TIMED_LAUNCH("enc_dissect_kernel", stream, enc_dissect_kernel, dim3(np * ((fx.runs_per_page + kDisRuns - 1) / kDisRuns)), dim3(256), kDisLdsBytes, stream, ws, fx, np);
  if (fx.fused & kFusedLookups) {
    fx.vlut = (uint16_t*)wsp.enc_vlut.ensure(vlut_bytes + 64);
    PCO_TIMED_LAUNCH("enc_vlut_kernel", stream, enc_vlut_kernel, dim3(nt * 3), dim3(256), 0, stream, ws, fx, nt);
  }
  PCO_RESERVE_LDS(enc_walkd_kernel, kWdLdsBytes, "enc_walkd_kernel");
  if (any_seg) PCO_TIMED_LAUNCH("enc_walkseg_kernel", stream, enc_walkseg_kernel, dim3(n_items), dim3(128), kWsLdsBytes, stream, ws, fx, np);
  if (walkp_on && !any_seg && (fx.fused & kFusedLookups) != 0) {
    PCO_RESERVE_LDS(enc_walkp_kernel, kWpLdsBytes, "enc_walkp_kernel");
    fx.body = (uint64_t*)((uint8_t*)fx.fstate + fstate_bytes); fx.wp_block = (uint32_t*)((uint8_t*)fx.fstate + fstate_bytes + body_bytes);
    PCO_TIMED_LAUNCH("enc_walkp_kernel", stream, enc_walkp_kernel, dim3((n_items + kWpQ - 1) / kWpQ), dim3(64 * (1 + kWpHelpers)), kWpLdsBytes, stream, ws, fx, np);
  }
  PCO_TIMED_LAUNCH("enc_walkd_kernel", stream, enc_walkd_kernel, dim3((n_items + kWdQ - 1) / kWdQ), dim3(64 * (1 + kWdHelpers)), kWdLdsBytes, stream, ws, fx, np);
  // more items than 8 per wave keep resident: 16 per wave first, then whatever needs the bigger slots (enc_walkd_kernel above)
  if ((fx.fused & 0xffu) == 2u) PCO_TIMED_LAUNCH("enc_walk16_kernel", stream, enc_walk_kernel<16>, dim3((n_items + 15) / 16), dim3(64), EwCfg<16>::kLdsBytes, stream, ws, fx, np, 1u);
  PCO_TIMED_LAUNCH("enc_scan_kernel", stream, enc_scan_kernel, dim3(np), dim3(64), 0, stream, ws, fx, c.d_results, np);
  // The bodies of enc_walkp_kernel's pages are moved into place on the workspace's second stream WHILE the pack kernels below write those
  // pages' heads (0.28 ms of one-wave blocks with a serial chain each) and pack the other pages: disjoint dwords but for the boundary
  // ones, which both sides OR into what enc_scan_kernel zeroed.
  const bool forked = fx.body != nullptr;
  std::unique_ptr<TimedSpan> span;
  if (forked) {
    ensure_side_stream(wsp);
    span.reset(new TimedSpan("enc_place+pack", stream));
    PCO_HIP_CHECK(hipEventRecord(wsp.fork_event, stream));
    PCO_HIP_CHECK(hipStreamWaitEvent(wsp.side_stream, wsp.fork_event, 0));
    PCO_TIMED_LAUNCH("~enc_place_kernel", wsp.side_stream, enc_place_kernel, dim3(np * place_pieces(page_max)), dim3(256), 0, wsp.side_stream, ws, fx, np, place_pieces(page_max));
    PCO_HIP_CHECK(hipEventRecord(wsp.join_event, wsp.side_stream));
  }
  encode_pack(c, fx, n_blocks, forked);
  if (forked) { PCO_HIP_CHECK(hipStreamWaitEvent(stream, wsp.join_event, 0)); span.reset(); }
  return true;
}

// The pack kernels of phase 8 (`forked`: under the enc_place+pack span, their names with a `~`): the lean ones per shape, then the general one over the rest.
static void encode_pack(const EncodeCall& c, const EncFast& fx, uint64_t n_blocks, bool forked) {
  const EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const size_t n_tasks = c.n_tasks; const uint32_t np = c.np;
  // the lean pack kernels, one launch per shape this call can have (which variables write anything is the plan's, known here; whether a variable's latents are 16-bit only on the device: both forms are launched)
  bool any1 = false;   // a chunk with the primary variable alone
  for (size_t i = 0; i < n_tasks; i++) any1 |= c.plans[i].mode_kind == kClassic && c.plans[i].delta_kind != kDeltaLookback;   // (a three-variable plan packs lean when one of its variables turns out trivial: either two-variable shape may come of it)
  const bool any_sec = c.any_sec, any_lb = c.any_lookback, any32 = (c.widths & 32u) != 0, any64 = (c.widths & 64u) != 0;
  const dim3 g((uint32_t)n_blocks), b64(64);
#define PCO_PACK1(L, mask, wide, name) PCO_TIMED_LAUNCH(forked ? "~" name : name, stream, (enc_pack1_kernel<L, mask, wide>), g, b64, pack1_lds_bytes(mask, wide), stream, ws, fx, np)
  // (a variable that turns out trivial -- one bin, no offsets -- drops out of the mask on the device: a two-variable plan may pack as one variable)
  if (any1 || any_sec || any_lb) { PCO_PACK1(uint32_t, 2u, false, "enc_pack1_kernel"); if (any32) PCO_PACK1(uint32_t, 2u, true, "enc_pack1_kernel<wide>"); if (any64) PCO_PACK1(uint64_t, 2u, true, "enc_pack1_kernel<wide>"); }
  if (any_sec) { PCO_PACK1(uint32_t, 6u, false, "enc_pack1_kernel<sec>"); if (any32) PCO_PACK1(uint32_t, 6u, true, "enc_pack1_kernel<sec,wide>"); if (any64) PCO_PACK1(uint64_t, 6u, true, "enc_pack1_kernel<sec,wide>"); }
  if (any_lb) { PCO_PACK1(uint32_t, 3u, false, "enc_pack1_kernel<lb>"); if (any32) PCO_PACK1(uint32_t, 3u, true, "enc_pack1_kernel<lb,wide>"); if (any64) PCO_PACK1(uint64_t, 3u, true, "enc_pack1_kernel<lb,wide>"); }
#undef PCO_PACK1
  PCO_TIMED_LAUNCH(forked ? "~enc_pack_kernel" : "enc_pack_kernel", stream, enc_pack_kernel, dim3((uint32_t)n_blocks), dim3(64), pack_lds_bytes(ws.n_slots), stream, ws, fx, np);
}

// Phase 9: the single-kernel page encoder over what the fast path left, the dictionaries of a Dict call into place, the wrapped surface's piece directory.
static void encode_pages_dict_infos(EncodeCall& c, uint32_t page_lds, bool skip_fast, PcoGfxPageInfo* d_infos) {
  const EncWorkspace& ws = c.ws; const hipStream_t stream = c.stream; const uint32_t np = c.np;
  PCO_TIMED_LAUNCH("enc_page_kernel", stream, enc_page_kernel, dim3(np), dim3(64), page_lds, stream, ws, c.d_tasks, c.d_results, np, skip_fast ? 1u : 0u);
  if (ws.dict) {   // Dict: the dictionaries into the holes the meta writers left (a block per 256 KB of the longest)
    const uint32_t bpp = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (c.n_max * 8) >> 18));
    if ((uint64_t)np * bpp >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many pages in one call"};
    PCO_TIMED_LAUNCH("enc_dict_place_kernel", stream, enc_dict_place_kernel, dim3(np * bpp), dim3(256), 0, stream, ws, np, bpp);
  }
  if (d_infos) PCO_TIMED_LAUNCH("wrapped_infos_kernel", stream, wrapped_infos_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, (const EncPage*)ws.pages, (const PcoGfxEncodeTask*)c.d_tasks, (const PcoGfxTaskResult*)c.d_results, d_infos, np);
  PCO_HIP_CHECK(hipGetLastError());
}

// Run the encode pipeline over `tasks` (one per chunk) and `pages` (>= 1 per chunk; results are per page).
// stop_after: 1 = behind the split, 2 = behind train (the Auto-delta trials); ws_out: the device arrays as the pass left them;
// d_infos: the wrapped surface's piece directory, on the device.
static void run_encode(size_t n_tasks, const PcoGfxEncodeTask* tasks, std::vector<EncModePlan>& plans, std::vector<EncPage>& pages,
                       const ResolvedConfig& cfg, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results_user, hipStream_t stream,
                       EncWorkspace* ws_out = nullptr, int stop_after = 0, PcoGfxPageInfo* d_infos = nullptr) {
  EncodeCall c(n_tasks, tasks, plans, pages, cfg, results, stream, stop_after);
  encode_carve_and_upload(c, d_results_user);
  encode_init_and_latent_slots(c);
  encode_split(c);
  if (stop_after == 1) { PCO_HIP_CHECK(hipGetLastError()); if (ws_out) *ws_out = c.ws; return; }
  encode_conv1(c);
  encode_lookback(c);
  encode_histograms(c);
  encode_train(c);
  if (stop_after == 2) { PCO_HIP_CHECK(hipGetLastError()); if (ws_out) *ws_out = c.ws; return; }
  const uint32_t page_lds = encode_page_lds(c);
  const bool skip_fast = encode_fast_pages(c);
  encode_pages_dict_infos(c, page_lds, skip_fast, d_infos);
  if (results) {
    PCO_HIP_CHECK(hipMemcpyAsync(results, c.d_results, pages.size() * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  if (ws_out) *ws_out = c.ws;
}

}  // namespace pcogfx
