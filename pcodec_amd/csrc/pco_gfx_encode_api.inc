// pco_gfx_encode_api.inc -- encode entry points of the C ABI (included by pco_gfx.hip).
namespace pcogfx {

struct ResolvedConfig {
  uint32_t level;
  uint32_t mode_kind; double mode_f64; uint64_t mode_u64;
  uint32_t delta_kind, delta_order;
  uint64_t max_page_n; bool enable_8_bit;
  bool strict_hist;   // PCO_GFX_CFG_STRICT_HISTOGRAM: enc_hist_literal_kernel replays the reference's quickselect behind the fast histograms
  bool conv1 = false;           // PCO_GFX_CFG_CONV1: DeltaSpec::TryConv1 is encoded (encode_conv1.hip) instead of refused
  bool dict = false;            // PCO_GFX_CFG_DICT: ModeSpec::TryDict is encoded (encode_dict.hip) instead of refused
  DictTask* d_dict = nullptr;   // the final encode of a Dict call: the dictionaries build_dicts made (the chunks are u32 index chunks by then)
  uint32_t unknown_flags = 0;   // bits of PcoChunkConfigEx::flags this library does not know (rejected by validate_config)
};

// PCO_GFX_STRICT_HISTOGRAM=1 in the environment turns the strict histogram on for every call (the reference's own three-function C ABI has no
// field for it)
// (a plain function, and not a const variable: a namespace-scope `static const bool x = [] { ... }();` in this translation unit was compiled
//  with ANOTHER lambda's body -- g_decode_trail's, which made every call strict; hipcc numbers host and device lambdas differently there)
static bool g_strict_hist_env = env_is_one("PCO_GFX_STRICT_HISTOGRAM");
static ResolvedConfig resolve_config(const PcoChunkConfigEx* c) {
  ResolvedConfig r{8, PCO_MODE_AUTO, 0.0, 0, PCO_DELTA_AUTO, 0, 1u << 18, true, g_strict_hist_env};
  if (c) {
    r.level = c->compression_level; r.mode_kind = c->mode_kind; r.mode_f64 = c->mode_f64; r.mode_u64 = c->mode_u64;
    r.delta_kind = c->delta_kind; r.delta_order = c->delta_order; r.max_page_n = c->max_page_n ? c->max_page_n : (1u << 18);
    r.enable_8_bit = c->enable_8_bit != 0;
    r.strict_hist = g_strict_hist_env || (c->flags & PCO_GFX_CFG_STRICT_HISTOGRAM) != 0;
    r.conv1 = (c->flags & PCO_GFX_CFG_CONV1) != 0;
    r.dict = (c->flags & PCO_GFX_CFG_DICT) != 0;
    r.unknown_flags = c->flags & ~(uint32_t)(PCO_GFX_CFG_STRICT_HISTOGRAM | PCO_GFX_CFG_CONV1 | PCO_GFX_CFG_DICT);
  }
  return r;
}

// ChunkConfig::validate (chunk_config.rs:269-314) + validate_chunk_size (wrapped/chunk_compressor.rs:113-127)
static void validate_config(const ResolvedConfig& c, int latent_bits) {
  if (c.unknown_flags) throw HostError{PCO_GFX_INVALID_ARGUMENT, "PcoChunkConfigEx::flags holds bits this library does not know (zero-initialise the struct)"};
  if (c.level > 12) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compression level may not exceed 12"};
  if (c.delta_kind == PCO_DELTA_TRY_CONSECUTIVE && c.delta_order > 7) throw HostError{PCO_GFX_INVALID_ARGUMENT, "consecutive delta order may not exceed 7"};
  if (c.delta_kind == PCO_DELTA_TRY_CONV1 && !c.conv1) throw HostError{PCO_GFX_UNSUPPORTED, "Conv1 delta encoding is outside the hot-path scope"};
  if (c.delta_kind == PCO_DELTA_TRY_CONV1) {   // chunk_config.rs:288-303
    if (c.delta_order > kConv1MaxOrder) throw HostError{PCO_GFX_INVALID_ARGUMENT, "conv1 delta order may not exceed 32 (was " + std::to_string(c.delta_order) + ")"};
    if (latent_bits > 32) throw HostError{PCO_GFX_INVALID_ARGUMENT, "Conv1 delta encoding is only supported for types with 32 or fewer bits"};
  }
  if (c.delta_kind > PCO_DELTA_TRY_CONV1 || c.mode_kind > PCO_MODE_TRY_DICT) throw HostError{PCO_GFX_INVALID_ARGUMENT, "unknown mode / delta spec"};
  if (c.mode_kind == PCO_MODE_TRY_DICT && !c.dict) throw HostError{PCO_GFX_UNSUPPORTED, "Dict mode is outside the hot-path scope"};
  // (Conv1 on Dict indices would fit in the u32 index type's arithmetic, not the number type's: not implemented)
  if (c.mode_kind == PCO_MODE_TRY_DICT && c.delta_kind == PCO_DELTA_TRY_CONV1) throw HostError{PCO_GFX_UNSUPPORTED, "Conv1 delta on Dict mode is outside the hot-path scope"};
  if (latent_bits == 8 && !c.enable_8_bit) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compressing 8-bit types with Pco is often a mistake; enable them on the ChunkConfig"};
}

// Resolve the mode / delta for one chunk from explicit specs
// (data_types/unsigned.rs:28-47, float.rs:82-132, wrapped/chunk_compressor.rs:373-394, delta/mod.rs:37-48).
static void plan_mode_explicit(EncModePlan& p, const ResolvedConfig& c, uint32_t dtype) {
  const uint32_t kind = dtype_kind(dtype); const int bits = dtype_bits(dtype);
  p.ubl_override = 0xffffffffu;
  switch (c.mode_kind) {
    case PCO_MODE_CLASSIC: p.mode_kind = kClassic; break;
    case PCO_MODE_TRY_INT_MULT: {
      if (kind == kFloat) throw HostError{PCO_GFX_INVALID_ARGUMENT, "unable to use int mult mode on floats"};
      p.mode_kind = kIntMult; p.mode_base = bits == 64 ? c.mode_u64 : (bits == 32 ? (uint64_t)(uint32_t)c.mode_u64 : (bits == 16 ? (uint64_t)(uint16_t)c.mode_u64 : (uint64_t)(uint8_t)c.mode_u64));
      if (p.mode_base == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
      break;
    }
    case PCO_MODE_TRY_FLOAT_MULT: {
      if (kind != kFloat) throw HostError{PCO_GFX_INVALID_ARGUMENT, "unable to use float mode for ints"};
      p.mode_kind = kFloatMult;
      if (bits == 64) {
        const double base = c.mode_f64, inv = 1.0 / base;
        if (!std::isfinite(base) || base == 0.0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
        uint64_t b; std::memcpy(&b, &base, 8); p.mode_aux2 = b; uint64_t iv; std::memcpy(&iv, &inv, 8); p.mode_aux = iv;
        p.mode_base = (b & (1ull << 63)) ? ~b : (b ^ (1ull << 63));
      } else if (bits == 32) {
        const float base = (float)c.mode_f64, inv = 1.0f / base;
        if (!std::isfinite(base) || base == 0.0f) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
        uint32_t b; std::memcpy(&b, &base, 4); p.mode_aux2 = b; uint32_t iv; std::memcpy(&iv, &inv, 4); p.mode_aux = iv;
        p.mode_base = (b & 0x80000000u) ? (uint32_t)~b : (b ^ 0x80000000u);
      } else {   // f16: the base is rounded once from the double, its inverse is ONE / base through f32 (float.rs:264-281; pco_half.h)
        const F16 base = F16::from_f64(c.mode_f64), inv = F16(1.0) / base;
        if ((base.bits & 0x7c00u) == 0x7c00u || (base.bits & 0x7fffu) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
        p.mode_aux2 = base.bits; p.mode_aux = inv.bits;
        p.mode_base = (base.bits & 0x8000u) ? (uint16_t)~base.bits : (uint16_t)(base.bits ^ 0x8000u);
      }
      break;
    }
    case PCO_MODE_TRY_FLOAT_QUANT: {
      if (kind != kFloat) throw HostError{PCO_GFX_INVALID_ARGUMENT, "unable to use float mode for ints"};
      const uint32_t prec = bits == 64 ? 52 : (bits == 32 ? 23 : 10);
      if (c.mode_u64 == 0 || c.mode_u64 > prec) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
      p.mode_kind = kFloatQuant; p.mode_k = (uint32_t)c.mode_u64; break;
    }
    default: throw HostError{PCO_GFX_INVALID_ARGUMENT, "ModeSpec::Auto must be resolved before planning"};
  }
}
static uint32_t lookback_window_log(uint64_t n) {  // delta/mod.rs:37-48
  const uint32_t m = (uint32_t)n - 1; const uint32_t b = m == 0 ? 0 : 32 - (uint32_t)__builtin_clz(m);
  return b < 4 ? 4 : (b > 15 ? 15 : b);
}
static void plan_delta_explicit(EncModePlan& p, const ResolvedConfig& c, uint64_t n) {
  p.delta_kind = kDeltaNone; p.delta_order = 0; p.window_n_log = 0; p.state_n_log = 0;
  switch (c.delta_kind) {
    case PCO_DELTA_NOOP: p.delta_kind = kDeltaNone; break;
    case PCO_DELTA_TRY_CONSECUTIVE: if (c.delta_order == 0) p.delta_kind = kDeltaNone; else { p.delta_kind = kDeltaConsecutive; p.delta_order = c.delta_order; } break;
    case PCO_DELTA_TRY_LOOKBACK: p.delta_kind = kDeltaLookback; p.window_n_log = lookback_window_log(n); p.state_n_log = 0; break;
    case PCO_DELTA_TRY_CONV1:   // TryConv1(0) is NoOp (wrapped/chunk_compressor.rs:381); the fit may still turn a chunk into NoOp (enc_conv1_solve_kernel)
      if (c.delta_order == 0) p.delta_kind = kDeltaNone; else { p.delta_kind = kDeltaConv1; p.delta_order = c.delta_order; }
      break;
    default: throw HostError{PCO_GFX_INVALID_ARGUMENT, "DeltaSpec::Auto must be resolved before planning"};
  }
}

// Run the encode pipeline over `tasks` (one per chunk) and `pages` (>= 1 per chunk; results are per page).
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
static void run_encode(size_t n_tasks, const PcoGfxEncodeTask* tasks, std::vector<EncModePlan>& plans, std::vector<EncPage>& pages,
                       const ResolvedConfig& cfg, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results_user, hipStream_t stream,
                       EncWorkspace* ws_out = nullptr, int stop_after = 0 /* 1 = split, 2 = train */, PcoGfxPageInfo* d_infos = nullptr /* wrapped surface: the piece directory, on the device */) {
  Workspace& wsp = workspace();
  wsp.lb_n = 0;   // (pco_gfx_debug_lookback_routes speaks of THIS pass: set again below if it has lookback pages)
  uint64_t n_max = 0, page_max = 0; bool any_sec = false, any_lookback = false, any_conv1 = false;
  for (size_t i = 0; i < n_tasks; i++) {
    n_max = std::max<uint64_t>(n_max, tasks[i].n);
    any_sec |= plans[i].mode_kind != kClassic; any_lookback |= plans[i].delta_kind == kDeltaLookback; any_conv1 |= plans[i].delta_kind == kDeltaConv1;
  }
  for (auto& p : pages) page_max = std::max<uint64_t>(page_max, p.n);
  const size_t n_pages = pages.size();
  EncWorkspace ws{};
  ws.dict = cfg.d_dict;
  ws.n_stride = ((n_max + 255) & ~(uint64_t)255) + 256;
  ws.n_slots = 0;
  ws.slot_of_var[0] = any_lookback ? ws.n_slots++ : 0xffffffffu;
  ws.slot_of_var[1] = ws.n_slots++;
  ws.slot_of_var[2] = any_sec ? ws.n_slots++ : 0xffffffffu;
  const size_t state_bytes = n_tasks * sizeof(EncChunk) + 256;
  // bin capacity of the plan regions: 4096 as soon as one chunk histograms into more than 256 bins (levels 9..12 on chunks of >= 2^13 numbers)
  bool any_big = false;
  for (size_t i = 0; i < n_tasks; i++) any_big |= (plans[i].ubl_override != 0xffffffffu ? plans[i].ubl_override : choose_unoptimized_bins_log(cfg.level, tasks[i].n)) > kMaxUnoptBinsLog;
  ws.plan_cap = any_big ? kBigBins : kMaxBins;
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
  PcoGfxEncodeTask* d_tasks = (PcoGfxEncodeTask*)d_small;
  EncModePlan* d_plans = (EncModePlan*)(d_small + off_plans);
  ws.pages = (EncPage*)(d_small + off_pages);
  uint8_t* d_state = (uint8_t*)wsp.enc_state.ensure(state_bytes + plan_bytes);
  ws.chunks = (EncChunk*)d_state;
  ws.plans = d_state + ((n_tasks * sizeof(EncChunk) + 255) & ~(size_t)255);
  // Full-width latents (8 B per number and variable) are scratch of the chunks that do not get by with 16-bit latents.  Which chunks those are
  // is decided on the device (enc_init_kernel, enc_presample_kernel, the 16-bit split itself), so the slots are handed out there
  // (enc_lat_slots_kernel).  A synchronous call reads the count back twice -- behind the sample and behind the 16-bit split, where it waits for
  // the device anyway or for 4 bytes more -- and allocates exactly that: nothing to speak of on data whose deltas are narrow (the headline),
  // everything for lookback.  An asynchronous call cannot wait and takes a slot per chunk up front.
  ws.lat_esz = 4; for (size_t i = 0; i < n_tasks; i++) if (dtype_bits(tasks[i].dtype) == 64) ws.lat_esz = 8;
  const size_t lat_slot_bytes = (size_t)ws.n_slots * ws.n_stride * ws.lat_esz;
  const bool lat_exact = results != nullptr;
  ws.lat = nullptr; ws.lat2 = nullptr; ws.lat_cap1 = 0;
  if (!lat_exact) { ws.lat_cap1 = (uint32_t)n_tasks; ws.lat = (uint8_t*)wsp.enc_lat.ensure(n_tasks * lat_slot_bytes); ws.lat2 = ws.lat; }
  // The two 8-byte-per-number sort buffers are only touched by lookback staging and by the radix-sort histogram; whether the
  // latter is needed is known on the device after the split.  Synchronous calls ask (one 4-byte read-back) and allocate on
  // demand; asynchronous calls (no host results) cannot wait and allocate up front.
  const size_t sort_bytes = n_tasks * 2 * ws.n_stride * ws.lat_esz;
  const bool sort_upfront = any_lookback || any_conv1 || results == nullptr || stop_after != 0 || cfg.strict_hist;   // (the strict histogram permutes a copy of every variable in the sort buffers)
  ws.sort = sort_upfront ? (uint8_t*)wsp.enc_sort.ensure(sort_bytes) : (uint8_t*)wsp.enc_sort.p;
  ws.dissect = (uint32_t*)wsp.enc_ans.ensure(n_tasks * ws.n_slots * ws.n_stride * 4);
  PcoGfxTaskResult* d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)wsp.results.ensure(n_pages * sizeof(PcoGfxTaskResult));
  PCO_HIP_CHECK(hipMemcpyAsync(d_tasks, tasks, n_tasks * sizeof(PcoGfxEncodeTask), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_plans, plans.data(), n_tasks * sizeof(EncModePlan), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(ws.pages, pages.data(), n_pages * sizeof(EncPage), hipMemcpyHostToDevice, stream));
  const uint32_t nt = (uint32_t)n_tasks, np = (uint32_t)n_pages;
  uint32_t skip_fast = 0;
  const uint32_t c16_enable = stop_after != 1 ? 1u : 0u;   // speculative 16-bit latents (the Auto-delta sampling reads the full-width latents back)
  PCO_TIMED_LAUNCH("enc_init_kernel", stream, enc_init_kernel, dim3((nt + 63) / 64), dim3(64), 0, stream, ws, d_tasks, d_plans, nt, cfg.level, c16_enable);
  const uint32_t tiles_per_page = (uint32_t)std::max<uint64_t>((page_max + kSplitTile - 1) / kSplitTile, 1);
  if ((uint64_t)np * tiles_per_page >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many pages in one call"};
  bool any_full0 = !c16_enable, any_spec = c16_enable != 0;   // chunks that do not / do speculate on 16-bit latents
  size_t n_lookback = 0;
  for (size_t i = 0; i < n_tasks; i++) n_lookback += plans[i].delta_kind == kDeltaLookback;
  any_full0 = any_full0 || n_lookback != 0 || any_big;   // (chunks with more than 256 bins never speculate on 16-bit latents)
  if (c16_enable) PCO_TIMED_LAUNCH("enc_presample_kernel", stream, enc_presample_kernel, dim3(nt), dim3(64), 0, stream, ws, d_tasks, nt);   // a 64-position sample takes hopeless chunks out of the speculation up front
  PCO_TIMED_LAUNCH("enc_lat_slots_kernel", stream, enc_lat_slots_kernel, dim3((nt + 63) / 64), dim3(64), 0, stream, ws, nt, 0u);
  uint32_t n_full = 0;   // chunks that never speculate (synchronous calls: exact)
  if (lat_exact) {   // synchronous call: ask how many slots are gone, i.e. how many chunks write full-width latents from the start (12 bytes); asynchronous calls launch every kernel regardless
    uint32_t flags[3] = {0, 0, 0};
    PCO_HIP_CHECK(hipMemcpyAsync(flags, ws.need_sort, 12, hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
    n_full = flags[2];
    any_full0 = n_full != 0; any_spec = c16_enable && n_full < n_tasks;
    ws.lat_cap1 = std::max<uint32_t>(n_full, 1u);
    ws.lat = (uint8_t*)wsp.enc_lat.ensure((size_t)ws.lat_cap1 * lat_slot_bytes);
    ws.lat2 = ws.lat;
  } else if (c16_enable) any_full0 = true;
  if (any_spec) PCO_TIMED_LAUNCH("enc_split_kernel<c16>", stream, (enc_split_kernel<true, false>), dim3(np * tiles_per_page), dim3(256), kSplitLdsBytes, stream, ws, d_tasks, tiles_per_page, 1u, 1u);
  if (any_full0) PCO_TIMED_LAUNCH("enc_split_kernel", stream, (enc_split_kernel<false, false>), dim3(np * tiles_per_page), dim3(256), kSplitLdsBytes, stream, ws, d_tasks, tiles_per_page, 1u, 0u);
  if (any_spec) {  // the chunks whose speculation failed
    PCO_TIMED_LAUNCH("enc_lat_slots_kernel", stream, enc_lat_slots_kernel, dim3((nt + 63) / 64), dim3(64), 0, stream, ws, nt, 2u);
    bool any_redo = true;
    if (lat_exact) {
      uint32_t used = 0;
      PCO_HIP_CHECK(hipMemcpyAsync(&used, ws.lat_used, 4, hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipStreamSynchronize(stream));
      const uint32_t n_redo = used > ws.lat_cap1 ? used - ws.lat_cap1 : 0u;   // (lat_cap1 is max(slots of the first hand-out, 1): with none handed out yet, slot 0 is the first redo chunk's and lies in lat)
      any_redo = used > n_full;
      if (n_redo) ws.lat2 = (uint8_t*)wsp.enc_lat2.ensure((size_t)n_redo * lat_slot_bytes);
    }
    if (any_redo) {
      const uint32_t tpb = 32, bpp = (tiles_per_page + tpb - 1) / tpb;
      PCO_TIMED_LAUNCH("enc_split_kernel(redo)", stream, (enc_split_kernel<false, true>), dim3(np * bpp), dim3(256), kSplitLdsBytes, stream, ws, d_tasks, tiles_per_page, tpb, 2u);
    }
  }
  if (stop_after == 1) { PCO_HIP_CHECK(hipGetLastError()); if (ws_out) *ws_out = ws; return; }
  if (any_conv1) {   // Conv1 delta (encode_conv1.hip): the fit over each whole chunk, then the residuals page by page
    const size_t conv_bytes = (n_tasks * sizeof(EncConv) + 255) & ~(size_t)255;
    uint8_t* d_conv = (uint8_t*)wsp.enc_conv.ensure(conv_bytes + n_pages * kConv1MaxOrder * sizeof(uint32_t) + 256);
    ws.conv = (EncConv*)d_conv; ws.conv_state = (uint32_t*)(d_conv + conv_bytes);
    PCO_TIMED_LAUNCH("enc_conv1_stats_kernel", stream, enc_conv1_stats_kernel, dim3(nt), dim3(kConv1Threads), 0, stream, ws, nt);
    PCO_TIMED_LAUNCH("enc_conv1_solve_kernel", stream, enc_conv1_solve_kernel, dim3(nt), dim3(64), 0, stream, ws, nt);
    PCO_TIMED_LAUNCH("enc_conv1_resid_kernel", stream, enc_conv1_resid_kernel, dim3(np * tiles_per_page), dim3(kConv1Threads), 0, stream, ws, tiles_per_page);
  }
  if (any_lookback) {
    // per page: last-index hash tables (2 x 2^(w+1) u32) + lookback counts (2^w u32); w <= 15
    uint32_t wmax = 4; for (size_t i = 0; i < n_tasks; i++) if (plans[i].delta_kind == kDeltaLookback) wmax = std::max(wmax, plans[i].window_n_log);
    const uint64_t stride_u32 = (4ull << wmax) + (1ull << wmax) + 64;
    std::vector<uint32_t> lb_pages;
    uint64_t page_min_lb = ~0ull;
    for (size_t pi = 0; pi < n_pages; pi++) if (plans[pages[pi].chunk].delta_kind == kDeltaLookback && !(pages[pi].flags & kPageFlagMetaOnly)) { lb_pages.push_back((uint32_t)pi); page_min_lb = std::min<uint64_t>(page_min_lb, pages[pi].n); }
    const uint32_t n_lb = (uint32_t)lb_pages.size();
    if (n_lb) {
      uint32_t* d_lb = (uint32_t*)wsp.enc_lb.ensure((size_t)n_lb * stride_u32 * 4 + (size_t)n_lb * 12 + 256);   // tables and counts per page, then the page ids, the redo list and the pre-pass's skip list
      uint32_t* d_ids = d_lb + (size_t)n_lb * stride_u32;
      PCO_HIP_CHECK(hipMemcpyAsync(d_ids, lb_pages.data(), (size_t)n_lb * 4, hipMemcpyHostToDevice, stream));   // (pageable source: staged before the call returns, like the task arrays above)
      // The hash proposals as a pre-pass with the page's tables in LDS (enc_lookback_hash_kernel), then the four-wave pipeline per page fed
      // from their streams (encode_lookback.hip).  The pipeline hands pages on which its speculation keeps failing back to the one-wave-per-page
      // kernel, which therefore always runs behind it.
      uint32_t* redo = d_ids + n_lb;
      uint32_t* d_skip = redo + n_lb;
      wsp.lb_n = n_lb; wsp.lb_redo_off = (size_t)(redo - d_lb); wsp.lb_skip_off = (size_t)(d_skip - d_lb);
      const bool small = page_max <= kLbPipeSmallMaxPage && wmax <= 13;
      const uint64_t prop_stride = ((page_max + 63) & ~(uint64_t)63) + 64;
      uint16_t* d_props = (uint16_t*)wsp.enc_lbprops.ensure((size_t)n_lb * 6 * prop_stride * 2 + 256);
      static const bool hash_ok = hipFuncSetAttribute((const void*)enc_lookback_hash_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lh_lds_bytes(15)) == hipSuccess;
      if (!hash_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_lookback_hash_kernel"};
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
  }
  PCO_TIMED_LAUNCH("enc_hist_kernel", stream, enc_hist_kernel, dim3(nt), dim3(256), kHistLdsBytes, stream, ws, nt);
  {
    static const bool wide_ok = hipFuncSetAttribute((const void*)enc_hist_wide_kernel<kWideHistRange>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds_bytes(kWideHistRange)) == hipSuccess &&
                                hipFuncSetAttribute((const void*)enc_hist_wide_kernel<kMidHistRange>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hist_lds_bytes(kMidHistRange)) == hipSuccess;
    if (!wide_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_hist_wide_kernel"};
    static const bool sort_ok = hipFuncSetAttribute((const void*)enc_hist_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHistSortLdsBytes) == hipSuccess;
    if (!sort_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_hist_sort_kernel"};
    // Which of the wider-range kernels have anything to do is known on the device once enc_hist_kernel has seen every variable's range:
    // synchronous calls ask (one 4-byte read-back) and launch only those; asynchronous calls launch them all (idle blocks leave at once,
    // but 8192 blocks of 1024 threads still cost 0.15 ms per kernel).
    // What the host knows without asking: a variable is never longer than its chunk, so a call of short chunks only (the Auto-delta
    // trial samples) has nothing for the select kernel; the whole-variable-in-LDS kernel's LDS is sized for the longest short chunk.
    uint64_t max_n = 0; uint32_t small_lds = 0;
    for (size_t i = 0; i < n_tasks; i++) {
      max_n = std::max<uint64_t>(max_n, tasks[i].n);
      const uint32_t kb = dtype_bits(tasks[i].dtype) == 64 ? 8u : 4u;
      small_lds = std::max(small_lds, small_lds_bytes((uint32_t)std::min<uint64_t>(tasks[i].n, kSmallHistCap), kb));
    }
    const bool any_long = max_n > kSmallHistCap;   // (short variables never reach the 16 k / 32 k-counter kernels or the select kernel)
    bool run_mid = any_long, run_wide = any_long, run_sort = any_long || any_big, run_small = true;
    if (results != nullptr && stop_after == 0) {
      uint32_t flag = 0;
      PCO_HIP_CHECK(hipMemcpyAsync(&flag, ws.need_sort, 4, hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipStreamSynchronize(stream));
      run_sort = (flag & 1u) != 0; run_mid = (flag & 2u) != 0; run_wide = (flag & 4u) != 0; run_small = (flag & 8u) != 0;
    }
    if (run_sort && !sort_upfront) ws.sort = (uint8_t*)wsp.enc_sort.ensure(sort_bytes);
    // the kernels with one or two big blocks per CU leave their bin walks (one thread's work, half their time) to enc_hist_walk_kernel
    if (run_mid || run_wide || run_small || run_sort) ws.walk = (uint8_t*)wsp.enc_walk.ensure((size_t)nt * 3 * kWalkRecBytes);
    if (run_mid) PCO_TIMED_LAUNCH("enc_hist_wide_kernel<16384>", stream, enc_hist_wide_kernel<kMidHistRange>, dim3(nt), dim3(1024), hist_lds_bytes(kMidHistRange), stream, ws, nt);
    if (run_wide) PCO_TIMED_LAUNCH("enc_hist_wide_kernel<32768>", stream, enc_hist_wide_kernel<kWideHistRange>, dim3(nt), dim3(1024), hist_lds_bytes(kWideHistRange), stream, ws, nt);
    if (run_small) {   // value ranges beyond the first counting tier, at most 8192 latents: ordered whole in LDS
      static const bool small_ok = hipFuncSetAttribute((const void*)enc_hist_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)small_lds_bytes(kSmallHistCap, 8)) == hipSuccess;
      if (!small_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_hist_small_kernel"};
      PCO_TIMED_LAUNCH("enc_hist_small_kernel", stream, enc_hist_small_kernel, dim3(nt), dim3(kSelT), small_lds, stream, ws, nt);
    }
    if (run_sort) {   // wide value ranges: quantile-segmented bucket select; the radix-sort kernel only sees what that one gave up on
      auto launch_sel = [&](auto kernel, const char* name) {
        if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSelLdsBytes) != hipSuccess) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_hist_select_kernel"};
        PCO_TIMED_LAUNCH(name, stream, kernel, dim3(nt), dim3(kSelThr), kSelLdsBytes, stream, ws, nt);
      };
      uint32_t widths = 0;
      for (size_t i = 0; i < n_tasks; i++) widths |= (uint32_t)dtype_bits(tasks[i].dtype);   // 8 | 16 | 32 | 64
      if (widths & 64u) launch_sel(enc_hist_select_kernel<uint64_t>, "enc_hist_select_kernel");
      if (widths & 32u) launch_sel(enc_hist_select_kernel<uint32_t>, "enc_hist_select_kernel");
      if (widths & 16u) launch_sel(enc_hist_select_kernel<uint16_t>, "enc_hist_select_kernel");
      if (widths & 8u) launch_sel(enc_hist_select_kernel<uint8_t>, "enc_hist_select_kernel");
      PCO_TIMED_LAUNCH("enc_hist_sort_kernel", stream, enc_hist_sort_kernel, dim3(nt), dim3(256), kHistSortLdsBytes, stream, ws, nt);
    }
    if (ws.walk != nullptr) PCO_TIMED_LAUNCH("enc_hist_walk_kernel", stream, enc_hist_walk_kernel, dim3(nt), dim3(64), kWalkLdsBytes, stream, ws, nt);
    // strict mode: the literal replay of histograms.rs overwrites the bins (encode_hist_literal.hip); everything else the kernels above left
    // behind (16-bit copies, ranges, paths) stands
    if (cfg.strict_hist) PCO_TIMED_LAUNCH("enc_hist_literal_kernel", stream, enc_hist_literal_kernel, dim3(nt), dim3(64), kLitLdsBytes, stream, ws, nt, strict_fell_back_counter(stream));
  }
  PCO_TIMED_LAUNCH("enc_train_kernel", stream, enc_train_kernel, dim3(nt), dim3(64), kTrainLdsBytes, stream, ws, nt);
  if (any_big) {   // levels 9..12: chunks with more than 256 histogram bins
    static const bool big_ok = hipFuncSetAttribute((const void*)enc_train_big_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrainBigLdsBytes) == hipSuccess;
    if (!big_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_train_big_kernel"};
    PCO_TIMED_LAUNCH("enc_train_big_kernel", stream, enc_train_big_kernel, dim3(nt), dim3(1024), kTrainBigLdsBytes, stream, ws, nt);
  }
  if (stop_after == 2) { PCO_HIP_CHECK(hipGetLastError()); if (ws_out) *ws_out = ws; return; }
  // LDS of the single-kernel page encoder: the variables' tables.  With more than 256 bins in play (levels 9..12) the worst case is two
  // variables of 4096 bins (the secondary never has more than 64: wrapped/chunk_compressor.rs:238-248) next to a small one.
  uint32_t page_lds = kPageLdsVar + ws.n_slots * page_var_bytes(cfg.level <= 8 ? 10 : kMaxEncTableLog);
  if (any_big) {
    page_lds = kPageLdsVar + std::min<uint32_t>(ws.n_slots, 2) * page_var_bytes(kMaxEncTableLog, kBigBins) + (ws.n_slots > 2 ? page_var_bytes(kMaxEncTableLog) : 0);
    static const bool page_ok = hipFuncSetAttribute((const void*)enc_page_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    if (!page_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_page_kernel"};
  }
  {  // common case: dissect / walk / scan / pack (encode_fast.hip); enc_page_kernel then only sees the rest
    EncFast fx{};
    const uint64_t max_batches = (page_max + kBatchN - 1) / kBatchN;
    fx.bat_stride = (uint32_t)max_batches + 1;
    fx.runs_per_page = (uint32_t)((max_batches + kRunBatches - 1) / kRunBatches); if (fx.runs_per_page == 0) fx.runs_per_page = 1;
    fx.run_stride = fx.runs_per_page + 1;
    uint32_t max_page_idx = 0; for (auto& pgi : pages) max_page_idx = std::max(max_page_idx, pgi.page_idx);
    fx.stride = ws.n_stride + 16ull * (max_page_idx + 1) + 64;
    fx.sym = (uint8_t*)wsp.enc_sym.ensure(n_tasks * ws.n_slots * fx.stride + 64);
    fx.answ = (uint16_t*)wsp.enc_answ.ensure(n_tasks * ws.n_slots * fx.stride * 2 + 64);
    fx.bat = (uint32_t*)wsp.enc_bat.ensure(n_pages * 3 * (size_t)fx.bat_stride * 8);
    fx.run_start = (uint64_t*)wsp.enc_run.ensure(n_pages * (size_t)fx.run_stride * 8);
    // (behind the final states, in the same buffer: the page body records and the block flags of enc_walkp_kernel)
    const size_t fstate_bytes = (n_pages * 12 * 4 + 63) & ~(size_t)63, body_bytes = (n_pages * 16 + 63) & ~(size_t)63, wpb_bytes = ((n_pages * (size_t)ws.n_slots + 15) / 16) * 4 + 64;
    fx.fstate = (uint32_t*)wsp.enc_fstate.ensure(fstate_bytes + body_bytes + wpb_bytes);
    const uint64_t n_blocks = (uint64_t)np * fx.runs_per_page;
    if (n_blocks < (1ull << 31)) {
      const uint32_t n_items = np * ws.n_slots;
      // variables with 16-bit latents get their symbols from the second wave of the walker's block (enc_walkd_kernel) instead of enc_dissect_kernel:
      // all of them while 8192 items cover the launch, else those whose tables need the big slots
      // the value -> bin tables are 8 KB per (chunk, variable) whatever the chunk's length: a call of very many short chunks keeps enc_dissect_kernel instead
      const size_t vlut_bytes = n_tasks * (size_t)ws.n_slots * kDirectHistRange * 2;
      uint64_t input_bytes = 0; for (size_t i = 0; i < n_tasks; i++) input_bytes += tasks[i].n * (uint64_t)(dtype_bits(tasks[i].dtype) / 8);
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
      static const bool walkd_ok = hipFuncSetAttribute((const void*)enc_walkd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWdLdsBytes) == hipSuccess;
      if (!walkd_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_walkd_kernel"};
      if (any_seg) PCO_TIMED_LAUNCH("enc_walkseg_kernel", stream, enc_walkseg_kernel, dim3(n_items), dim3(128), kWsLdsBytes, stream, ws, fx, np);
      if (walkp_on && !any_seg && (fx.fused & kFusedLookups) != 0) {
        static const bool walkp_ok = hipFuncSetAttribute((const void*)enc_walkp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWpLdsBytes) == hipSuccess;
        if (!walkp_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_walkp_kernel"};
        fx.body = (uint64_t*)((uint8_t*)fx.fstate + fstate_bytes); fx.wp_block = (uint32_t*)((uint8_t*)fx.fstate + fstate_bytes + body_bytes);
        PCO_TIMED_LAUNCH("enc_walkp_kernel", stream, enc_walkp_kernel, dim3((n_items + kWpQ - 1) / kWpQ), dim3(64 * (1 + kWpHelpers)), kWpLdsBytes, stream, ws, fx, np);
      }
      PCO_TIMED_LAUNCH("enc_walkd_kernel", stream, enc_walkd_kernel, dim3((n_items + kWdQ - 1) / kWdQ), dim3(64 * (1 + kWdHelpers)), kWdLdsBytes, stream, ws, fx, np);
      // more items than 8 per wave keep resident: 16 per wave first, then whatever needs the bigger slots (enc_walkd_kernel above)
      if ((fx.fused & 0xffu) == 2u) PCO_TIMED_LAUNCH("enc_walk16_kernel", stream, enc_walk_kernel<16>, dim3((n_items + 15) / 16), dim3(64), EwCfg<16>::kLdsBytes, stream, ws, fx, np, 1u);
      PCO_TIMED_LAUNCH("enc_scan_kernel", stream, enc_scan_kernel, dim3(np), dim3(64), 0, stream, ws, fx, d_results, np);
      // The bodies of enc_walkp_kernel's pages are moved into place on the workspace's second stream WHILE the pack kernels below write those
      // pages' heads (0.28 ms of one-wave blocks with a serial chain each) and pack the other pages: disjoint dwords but for the boundary
      // ones, which both sides OR into what enc_scan_kernel zeroed.
      const bool forked = fx.body != nullptr;
      std::unique_ptr<ScopedKernelTimer> span;
      if (forked) {
        ensure_side_stream(wsp);
        span.reset(new ScopedKernelTimer("enc_place+pack", stream));
        PCO_HIP_CHECK(hipEventRecord(wsp.fork_event, stream));
        PCO_HIP_CHECK(hipStreamWaitEvent(wsp.side_stream, wsp.fork_event, 0));
        PCO_TIMED_LAUNCH("~enc_place_kernel", wsp.side_stream, enc_place_kernel, dim3(np * place_pieces(page_max)), dim3(256), 0, wsp.side_stream, ws, fx, np, place_pieces(page_max));
        PCO_HIP_CHECK(hipEventRecord(wsp.join_event, wsp.side_stream));
      }
      // the lean pack kernels, one launch per shape this call can have (which variables write anything is the plan's, known here; whether a variable's latents are 16-bit only on the device: both forms are launched)
      bool any1 = false, any_sec = false, any_lb = false, any32 = false, any64 = false;
      for (size_t i = 0; i < n_tasks; i++) {
        const bool sec = plans[i].mode_kind != kClassic, lb = plans[i].delta_kind == kDeltaLookback;
        any_sec |= sec; any_lb |= lb; any1 |= !sec && !lb;   // (a three-variable plan packs lean when one of its variables turns out trivial: either two-variable shape may come of it)
        const int b = dtype_bits(tasks[i].dtype); any32 |= b == 32; any64 |= b == 64;
      }
      const dim3 g((uint32_t)n_blocks), b64(64);
#define PCO_PACK1(L, mask, wide, name) PCO_TIMED_LAUNCH(forked ? "~" name : name, stream, (enc_pack1_kernel<L, mask, wide>), g, b64, pack1_lds_bytes(mask, wide), stream, ws, fx, np)
      // (a variable that turns out trivial -- one bin, no offsets -- drops out of the mask on the device: a two-variable plan may pack as one variable)
      if (any1 || any_sec || any_lb) { PCO_PACK1(uint32_t, 2u, false, "enc_pack1_kernel"); if (any32) PCO_PACK1(uint32_t, 2u, true, "enc_pack1_kernel<wide>"); if (any64) PCO_PACK1(uint64_t, 2u, true, "enc_pack1_kernel<wide>"); }
      if (any_sec) { PCO_PACK1(uint32_t, 6u, false, "enc_pack1_kernel<sec>"); if (any32) PCO_PACK1(uint32_t, 6u, true, "enc_pack1_kernel<sec,wide>"); if (any64) PCO_PACK1(uint64_t, 6u, true, "enc_pack1_kernel<sec,wide>"); }
      if (any_lb) { PCO_PACK1(uint32_t, 3u, false, "enc_pack1_kernel<lb>"); if (any32) PCO_PACK1(uint32_t, 3u, true, "enc_pack1_kernel<lb,wide>"); if (any64) PCO_PACK1(uint64_t, 3u, true, "enc_pack1_kernel<lb,wide>"); }
#undef PCO_PACK1
      PCO_TIMED_LAUNCH(forked ? "~enc_pack_kernel" : "enc_pack_kernel", stream, enc_pack_kernel, dim3((uint32_t)n_blocks), dim3(64), pack_lds_bytes(ws.n_slots), stream, ws, fx, np);
      if (forked) { PCO_HIP_CHECK(hipStreamWaitEvent(stream, wsp.join_event, 0)); span.reset(); }
      skip_fast = 1;
    }
  }
  PCO_TIMED_LAUNCH("enc_page_kernel", stream, enc_page_kernel, dim3(np), dim3(64), page_lds, stream, ws, d_tasks, d_results, np, skip_fast);
  if (ws.dict) {   // Dict: the dictionaries into the holes the meta writers left (a block per 256 KB of the longest)
    const uint32_t bpp = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(1, (n_max * 8) >> 18));
    if ((uint64_t)np * bpp >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many pages in one call"};
    PCO_TIMED_LAUNCH("enc_dict_place_kernel", stream, enc_dict_place_kernel, dim3(np * bpp), dim3(256), 0, stream, ws, np, bpp);
  }
  if (d_infos) PCO_TIMED_LAUNCH("wrapped_infos_kernel", stream, wrapped_infos_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, (const EncPage*)ws.pages, (const PcoGfxEncodeTask*)d_tasks, (const PcoGfxTaskResult*)d_results, d_infos, np);
  PCO_HIP_CHECK(hipGetLastError());
  if (results) {
    PCO_HIP_CHECK(hipMemcpyAsync(results, d_results, n_pages * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  if (ws_out) *ws_out = ws;
}

static void validate_task(const PcoGfxEncodeTask& t, const ResolvedConfig& cfg, bool device_dst) {
  const int bits = dtype_bits(t.dtype);
  if (!bits) throw HostError{PCO_GFX_INVALID_ARGUMENT, "invalid dtype"};
  validate_config(cfg, bits);
  if (t.n == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot compress empty chunk"};
  if (t.n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, "count may not exceed 2^24 per chunk"};
  if ((device_dst && ((uintptr_t)t.dst & 7)) || ((uintptr_t)t.src & (bits / 8 - 1))) throw HostError{PCO_GFX_INVALID_ARGUMENT, "dst must be 8-byte aligned and src naturally aligned"};
}

// ---------------------------------------------------------------------------------------------------------
// Auto specs.  ModeSpec::Auto: Floyd sample gathered on the device, decision on the host (pco_auto_host.inc).
// DeltaSpec::Auto (wrapped/chunk_compressor.rs:289-360): the primary latents are produced once without delta,
// a 33x200 strided sample of them is trial-compressed on the device under every candidate encoding at once
// (NoOp, Lookback, Consecutive 1..7), and the reference's sequential decision is replayed on the host from the
// resulting size estimates (f64 log2 via libm, like the reference).
// ---------------------------------------------------------------------------------------------------------
static void run_gather(std::vector<GatherTask>& g, uint32_t max_idx, hipStream_t stream, DevBuf& buf) {
  GatherTask* d = (GatherTask*)buf.ensure(g.size() * sizeof(GatherTask));
  PCO_HIP_CHECK(hipMemcpyAsync(d, g.data(), g.size() * sizeof(GatherTask), hipMemcpyHostToDevice, stream));
  const uint32_t bpt = (max_idx + 255) / 256;
  if (bpt == 0 || g.empty()) return;
  if ((uint64_t)bpt * g.size() >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many chunks in one call"};
  hipLaunchKernelGGL(gather_kernel, dim3(bpt * (uint32_t)g.size()), dim3(256), 0, stream, d, bpt);
  PCO_HIP_CHECK(hipGetLastError());
}

template <class L>
static void detect_mode_for(const std::vector<L>& raw, uint32_t dtype, EncModePlan& p) {
  using namespace autodetect;
  const uint32_t kind = dtype_kind(dtype);
  constexpr L mid = (L)1 << (sizeof(L) * 8 - 1);
  p.mode_kind = kClassic; p.mode_k = 0; p.mode_base = p.mode_aux = p.mode_aux2 = 0;
  if (kind != kFloat) {  // data_types/unsigned.rs:28-37: int mult is bid INSTEAD of classic when a base is found
    std::vector<L> lat(raw.size());
    for (size_t i = 0; i < raw.size(); i++) lat[i] = kind == kSigned ? (L)(raw[i] ^ mid) : raw[i];
    L base;
    if (choose_int_base<L>(lat, base)) { p.mode_kind = kIntMult; p.mode_base = (uint64_t)base; }
    return;
  }
  if constexpr (sizeof(L) >= 2) {  // data_types/float.rs:70-98: classic (0.0), float mult, float quant; last maximum wins
    typedef typename FloatTraits<L>::F F;
    std::vector<F> s;
    const F lim = max_for_sampling<L>();
    for (L b : raw) { const F x = fbits<L>(b); if (is_normal<L>(x)) { const F a = fabsx<L>(x); if (a <= lim) s.push_back(a); } }
    if (s.size() < kMinSample) return;
    double best = 0.0; int win = 0; MultConfig<L> mc{}; uint32_t qk = 0;
    { MultConfig<L> c; double v; if (FloatDetect<L>::mult_bid(s, c, v) && !(v < best)) { best = v; win = 1; mc = c; } }
    { uint32_t k; double v; if (FloatDetect<L>::quant_bid(s, k, v) && !(v < best)) { best = v; win = 2; qk = k; } }
    if (win == 1) {
      p.mode_kind = kFloatMult; p.mode_aux2 = (uint64_t)tobits<L>(mc.base); p.mode_aux = (uint64_t)tobits<L>(mc.inv_base);
      p.mode_base = (uint64_t)ordered<L>(mc.base);
      if (!is_finite<L>(mc.base) || mc.base == (F)0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
    } else if (win == 2) { p.mode_kind = kFloatQuant; p.mode_k = qk; }
  }
}

static std::vector<double> make_log2_table() { std::vector<double> v(kBigBins + 1, 0.0); for (uint32_t w = 1; w <= kBigBins; w++) v[w] = std::log2((double)w); return v; }   // (a named function: see env_is_one in pco_host.h)
static double trial_size(const TrialSummary& s, int latent_bits, uint32_t nlps_primary) {  // chunk_compressor.rs:289-307,603-621
  size_t meta_bits = kBitsModeVariant + (4 + 5 + 5 + 64 + 32 * 32), page_meta_bits = 0, body_bits = 0;
  for (int v = 0; v < 2; v++) {
    const bool present = v == 1 || (nlps_primary & 0x80000000u);  // bit31 of nlps_primary flags a lookback trial (delta var present)
    if (!present) continue;
    const uint32_t lb = v == 0 ? 32u : (uint32_t)latent_bits, asl = s.asl[v], nb = s.n_bins[v];
    meta_bits += kBitsAnsSizeLog + kBitsNBins + (size_t)nb * (asl + lb + offset_bits_bits(lb));
    page_meta_bits += (size_t)asl * 4 + (v == 1 ? (size_t)lb * (nlps_primary & 0x7fffffffu) : 0);
    const double avg = s.avg[v];   // (summed on the device in the reference's order: enc_trial_summary_kernel)
    body_bits += (size_t)std::ceil((double)s.n_lat[v] * avg * 1.0);
  }
  return (double)((meta_bits + 7) / 8 + (page_meta_bits + 7) / 8 + (body_bits + 7) / 8);
}

// Host-side per-chunk decisions (Auto mode detection on a 6.5k-number sample, scoring of the device's GCD lists) are independent per
// chunk and run on a pool of worker threads that lives as long as the process: spawning threads per call cost 4 ms a time on a
// 128-CPU host (measured: more than the work itself).  Pool size = the CPUs this process may actually use (affinity mask, cgroup quota),
// divided by LOCAL_WORLD_SIZE when a launcher says several ranks share the node, at most 64; PCO_GFX_HOST_THREADS overrides.
static size_t host_thread_count() {
  if (const char* e = std::getenv("PCO_GFX_HOST_THREADS")) { const long v = atol(e); if (v >= 1) return (size_t)std::min<long>(v, 256); }
  size_t hw = std::max<size_t>(1, std::thread::hardware_concurrency());
  cpu_set_t set; CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) hw = std::min<size_t>(hw, (size_t)CPU_COUNT(&set));
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0}; long long per = 0;
    if (fscanf(f, "%31s %lld", q, &per) == 2 && strcmp(q, "max") != 0) { const long long quota = atoll(q); if (quota > 0 && per > 0) hw = std::min<size_t>(hw, (size_t)std::max<long long>(1, (quota + per - 1) / per)); }
    fclose(f);
  }
  // one process per GPU (torchrun and friends export LOCAL_WORLD_SIZE): the ranks of a node share its CPUs, so each takes its share --
  // eight ranks on a 16-CPU container are eight pools of two threads, not eight pools of sixteen
  if (const char* e = std::getenv("LOCAL_WORLD_SIZE")) { const long lw = atol(e); if (lw > 1) hw = std::max<size_t>(1, hw / (size_t)lw); }
  if (g_trace) fprintf(stderr, "[pco_gfx trace] host pool: %zu threads (hardware_concurrency %u)\n", std::min<size_t>(hw, 64), std::thread::hardware_concurrency());
  return std::min<size_t>(hw, 64);
}
class HostPool {
 public:
  // The pool is leaked on purpose (workers must not be joined from a static destructor).  fork(): the child inherits the object but
  // none of its threads, so a job would wait for workers that do not exist -- a pthread_atfork child handler drops the inherited pool
  // (and the mutex guarding its creation, which a thread that no longer exists may have held); the next call builds a fresh one.
  static HostPool& get() {
    HostPool* p = slot().load(std::memory_order_acquire);
    if (p) return *p;
    std::lock_guard<std::mutex> lk(*create_mutex());
    p = slot().load(std::memory_order_acquire);
    if (!p) {
      static bool atfork_registered = false;
      if (!atfork_registered) { pthread_atfork(nullptr, nullptr, &HostPool::drop_in_child); atfork_registered = true; }
      p = new HostPool(host_thread_count());
      slot().store(p, std::memory_order_release);
    }
    return *p;
  }
  static void drop_in_child() { slot().store(nullptr, std::memory_order_release); create_mutex() = new std::mutex(); }   // (a named function, not a lambda: pco_host.h, env_is_one)
  size_t size() const { return n_workers_ + 1; }
  // fn(i) for i in [0, n), in blocks of `grain`; the caller works too.  HostError from any block is rethrown here.
  void run(size_t n, size_t grain, const std::function<void(size_t)>& fn) {
    if (n == 0) return;
    if (n_workers_ == 0 || n <= grain) { for (size_t i = 0; i < n; i++) fn(i); return; }
    std::unique_lock<std::mutex> call_lock(call_m_);   // one job at a time
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn; n_ = n; grain_ = grain; next_.store(0); pending_ = n_workers_; err_ = HostError{PCO_GFX_OK, ""}; gen_++;
    }
    cv_work_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return pending_ == 0; });
    fn_ = nullptr;
    if (err_.status != PCO_GFX_OK) throw err_;
  }
 private:
  static std::atomic<HostPool*>& slot() { static std::atomic<HostPool*> s{nullptr}; return s; }
  static std::mutex*& create_mutex() { static std::mutex* m = new std::mutex(); return m; }
  explicit HostPool(size_t threads) : n_workers_(threads > 1 ? threads - 1 : 0) {
    for (size_t k = 0; k < n_workers_; k++) std::thread([this] { loop(); }).detach();
  }
  void record(const HostError& e) { std::lock_guard<std::mutex> lk(m_); if (err_.status == PCO_GFX_OK) err_ = e; next_.store(n_); }
  void work() {   // (nothing may escape a worker thread: an exception there would terminate the process)
    try { for (;;) { const size_t b = next_.fetch_add(grain_); if (b >= n_) break; for (size_t i = b; i < std::min(n_, b + grain_); i++) (*fn_)(i); } }
    catch (const HostError& e) { record(e); }
    catch (const std::bad_alloc&) { record(HostError{PCO_GFX_DEVICE_ERROR, "host allocation failed in a worker thread"}); }
    catch (const std::exception& e) { record(HostError{PCO_GFX_DEVICE_ERROR, std::string("worker thread: ") + e.what()}); }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      { std::unique_lock<std::mutex> lk(m_); cv_work_.wait(lk, [&] { return gen_ != seen; }); seen = gen_; }
      work();
      { std::lock_guard<std::mutex> lk(m_); if (--pending_ == 0) cv_done_.notify_all(); }
    }
  }
  const size_t n_workers_;
  std::mutex m_, call_m_; std::condition_variable cv_work_, cv_done_;
  const std::function<void(size_t)>* fn_ = nullptr; size_t n_ = 0, grain_ = 1; std::atomic<size_t> next_{0}; size_t pending_ = 0; uint64_t gen_ = 0;
  HostError err_{PCO_GFX_OK, ""};
};
template <class F>
static void parallel_for_chunks(size_t n, F&& fn, size_t grain = 16) {
  const std::function<void(size_t)> f = std::ref(fn);
  HostPool::get().run(n, grain, f);
}

namespace autodetect {
// most_prominent_gcd (mode/int_mult.rs:187-203) over the device's (value, count, first triple) list: the scores of candidate_base, in
// its order (first appearance), last maximum kept.  Values seen once are not in the list: they never score (see gcd_table_emit).
inline bool candidate_from_counts(const IntGcdEntry* e, uint32_t n, size_t triples, uint64_t& base, double& score) {
  std::vector<IntGcdEntry> v(e, e + n);
  std::sort(v.begin(), v.end(), [](const IntGcdEntry& x, const IntGcdEntry& y) { return x.first < y.first; });
  bool found = false; double best = 0.0;
  for (const IntGcdEntry& gc : v) {
    double s;
    if (!score_gcd((double)gc.gcd, gc.count, triples, s)) continue;
    if (!found || s >= best) { found = true; best = s; base = gc.gcd; }
  }
  score = best;
  return found;
}
// The float candidates that stage 1's statistics allow (mode/float_mult.rs:145-194, 197-275; mode/float_quant.rs:73-118):
// slot[q] = 0 marks candidate q (0: trailing zeros, 1: Euclid) as present, qslot = 0 a float-quant candidate (bk, best).
template <class L> void float_candidates(const FloatStatsResult& r, uint64_t (&base)[2], uint64_t (&inv)[2], int (&slot)[2], uint32_t& bk, double& best, int& qslot) {
  typedef FloatTraits<L> T; typedef typename T::F F;
  const size_t sz = r.s_size;
  const size_t required = std::max((size_t)std::ceil((double)sz * 0.5), kMinSample);
  if (r.tz5 >= required && r.n_ints >= required) {
    uint64_t ib = 1; double sc;
    L int_base = 1;
    if (candidate_from_counts(r.e, r.n_entries, r.n_ints / 3, ib, sc)) int_base = (L)ib;
    const MultConfig<L> c = FloatDetect<L>::from_base((F)int_base * pow2<L>(r.k));
    base[0] = (uint64_t)tobits<L>(c.base); inv[0] = (uint64_t)tobits<L>(c.inv_base); slot[0] = 0;
  }
  if (r.has_euclid) {
    const MultConfig<L> c = FloatDetect<L>::snap(fbits<L>((L)r.base_c));
    base[1] = (uint64_t)tobits<L>(c.base); inv[1] = (uint64_t)tobits<L>(c.inv_base); slot[1] = 0;
  }
  uint64_t cum[64] = {0}; uint64_t rev = 0;
  for (int b = T::kPrec; b >= 0; b--) { rev += r.hist[b]; cum[b] = rev; }
  bk = 0; best = 0.0;
  for (int b = 1; b <= T::kPrec; b++) {
    if (cum[b] == 0) continue;
    const double freq = (double)cum[b] / (double)sz;
    const double sv = (double)b - worst_case_entropy(freq, (double)(((uint64_t)1 << b) - 1));
    if (sv > best) { bk = (uint32_t)b; best = sv; } else break;
  }
  // the estimate is at most the per-number saving `best` (a mean of sums of it), and 1.5 bits are asked for
  if (best > 1.499) qslot = 0;
}
}  // namespace autodetect

static void resolve_plans(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, std::vector<EncModePlan>& plans, hipStream_t stream) {
  Workspace& wsp = workspace();
  for (size_t i = 0; i < n_tasks; i++) { plans[i] = EncModePlan{}; plans[i].ubl_override = 0xffffffffu; }
  std::vector<PcoGfxAutoModeRecord>& dbg = wsp.auto_dbg;   // (pco_gfx_debug_auto_mode: the first chunks of THIS call, all-zero = route "none")
  dbg.assign(cfg.mode_kind == PCO_MODE_AUTO ? std::min<size_t>(n_tasks, PCO_GFX_AUTO_DEBUG_MAX) : 0, PcoGfxAutoModeRecord{});
  // ---------------- mode ----------------
  if (cfg.mode_kind != PCO_MODE_AUTO) { for (size_t i = 0; i < n_tasks; i++) plan_mode_explicit(plans[i], cfg, tasks[i].dtype); }
  else {
    TracePhase tp_mode("auto mode (sample + detect)", stream);
    std::unordered_map<uint64_t, std::pair<std::vector<uint32_t>, size_t>> by_n;  // n -> (indices, offset in the device index pool)
    size_t pool = 0;
    for (size_t i = 0; i < n_tasks; i++) if (!by_n.count(tasks[i].n)) { auto idx = autodetect::mode_sample_indices(tasks[i].n); by_n[tasks[i].n] = {idx, pool}; pool += idx.size(); }
    uint8_t* d_pool = (uint8_t*)wsp.auto_idx.ensure(pool * 4 + 64);
    for (auto& kv : by_n) if (!kv.second.first.empty()) PCO_HIP_CHECK(hipMemcpyAsync(d_pool + kv.second.second * 4, kv.second.first.data(), kv.second.first.size() * 4, hipMemcpyHostToDevice, stream));
    std::vector<size_t> cnts(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) cnts[i] = by_n[tasks[i].n].first.size();
    // Stage 1 on the device (auto_mode_kernels.hip): triple-GCD counts for integer chunks, the float statistics and the sample itself for
    // float chunks.  The host turns them into candidate configurations (its libm: score_gcd, snap, the float-quant entropy), stage 2
    // measures what every candidate saves, the host picks the bid.  Samples beyond kAutoCap numbers (chunks above 2^18), f16 and GCD lists
    // that do not fit their slots take the host path on the sample itself.
    std::vector<size_t> on_host;
    {
      std::vector<size_t> ints, floats;
      for (size_t i = 0; i < n_tasks; i++) {
        plans[i].mode_kind = kClassic; plans[i].mode_k = 0; plans[i].mode_base = plans[i].mode_aux = plans[i].mode_aux2 = 0;
        if (cnts[i] < autodetect::kMinSample) continue;
        const bool is_float = dtype_kind(tasks[i].dtype) == kFloat;
        if (cnts[i] > kAutoCap || (is_float && dtype_bits(tasks[i].dtype) < 32)) on_host.push_back(i);
        else if (is_float) floats.push_back(i); else ints.push_back(i);
      }
      static const bool host_only = std::getenv("PCO_GFX_AUTO_MODE_ON_HOST") != nullptr;   // A/B switch
      if (host_only) { on_host.insert(on_host.end(), ints.begin(), ints.end()); on_host.insert(on_host.end(), floats.begin(), floats.end()); ints.clear(); floats.clear(); }
      for (size_t i : on_host) if (i < dbg.size()) dbg[i].route = 3;
      const size_t ni = ints.size(), nf = floats.size(), ns_max = ni + 3 * nf;
      if (ni + nf > 0) {
        static const bool lds_ok = hipFuncSetAttribute((const void*)auto_float_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAutoStage1LdsBytes) == hipSuccess &&
                                   hipFuncSetAttribute((const void*)auto_saved_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAutoSavedLdsBytes) == hipSuccess;
        if (!lds_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for the Auto mode kernels"};
        auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
        const size_t o_it = 0, o_ft = o_it + up16(ni * sizeof(IntGcdTask)), o_ir = o_ft + up16(nf * sizeof(FloatStatsTask)), o_fr = o_ir + up16(ni * sizeof(IntGcdResult)),
                     o_st = o_fr + up16(nf * sizeof(FloatStatsResult)), o_sr = o_st + up16(ns_max * sizeof(SavedTask)), dev_bytes = o_sr + up16(ns_max * sizeof(SavedResult));
        uint8_t* d_all = (uint8_t*)wsp.auto_tasks.ensure(dev_bytes);
        uint8_t* d_sbuf = (uint8_t*)wsp.auto_samp.ensure(std::max<size_t>(nf, 1) * kAutoCap * 8);
        const size_t res_bytes = o_st - o_ir;
        uint8_t* h_all = (uint8_t*)wsp.h_samp.ensure(std::max(o_ir, res_bytes) + 64);   // stage-1 task lists going up, then results coming down
        IntGcdTask* h_it = (IntGcdTask*)(h_all + o_it); FloatStatsTask* h_ft = (FloatStatsTask*)(h_all + o_ft);
        for (size_t k = 0; k < ni; k++) { const size_t i = ints[k]; auto& e = by_n[tasks[i].n]; h_it[k] = IntGcdTask{tasks[i].src, (const uint32_t*)(d_pool + e.second * 4), (uint32_t)e.first.size(), tasks[i].dtype}; }
        for (size_t k = 0; k < nf; k++) { const size_t i = floats[k]; auto& e = by_n[tasks[i].n]; h_ft[k] = FloatStatsTask{tasks[i].src, (const uint32_t*)(d_pool + e.second * 4), d_sbuf + k * (size_t)kAutoCap * 8, (uint32_t)e.first.size(), tasks[i].dtype}; }
        {
          TracePhase tp_1("  mode: stage 1 (device statistics)", stream);
          PCO_HIP_CHECK(hipMemcpyAsync(d_all, h_all, o_ir, hipMemcpyHostToDevice, stream));
          PCO_HIP_CHECK(hipStreamSynchronize(stream));   // (h_all is reused for the results)
          if (ni) hipLaunchKernelGGL(auto_int_gcd_kernel, dim3((uint32_t)ni), dim3(256), 0, stream, (const IntGcdTask*)(d_all + o_it), (IntGcdResult*)(d_all + o_ir));
          if (nf) hipLaunchKernelGGL(auto_float_stats_kernel, dim3((uint32_t)nf), dim3(kAutoT), kAutoStage1LdsBytes, stream, (const FloatStatsTask*)(d_all + o_ft), (FloatStatsResult*)(d_all + o_fr));
          PCO_HIP_CHECK(hipGetLastError());
          PCO_HIP_CHECK(hipMemcpyAsync(h_all, d_all + o_ir, res_bytes, hipMemcpyDeviceToHost, stream));
          PCO_HIP_CHECK(hipStreamSynchronize(stream));
        }
        IntGcdResult* h_ir = (IntGcdResult*)h_all; FloatStatsResult* h_fr = (FloatStatsResult*)(h_all + (o_fr - o_ir));
        // ---- host step: candidates ----
        struct IntCand { uint64_t base; double per_adj; int slot; };            // slot: index of the chunk's stage-2 task, -1 = none
        struct FloatCand { uint64_t base[2], inv[2]; int slot[2]; uint32_t bk; double best; int qslot; uint8_t host; };
        std::vector<IntCand> icand(ni, IntCand{0, 0.0, -1}); std::vector<FloatCand> fcand(nf);
        std::vector<uint8_t> ihost(ni, 0);
        {
          TracePhase tp_h("  mode: host candidates", stream);
          parallel_for_chunks(ni, [&](size_t k) {
            IntGcdResult& r = h_ir[k];
            if (r.overflow) { ihost[k] = 1; return; }
            uint64_t base; double score;
            if (autodetect::candidate_from_counts(r.e, r.n_entries, cnts[ints[k]] / 3, base, score)) { icand[k].base = base; icand[k].per_adj = score; icand[k].slot = 0; }
          });
          parallel_for_chunks(nf, [&](size_t k) {
            FloatCand& c = fcand[k]; c = FloatCand{}; c.slot[0] = c.slot[1] = c.qslot = -1;
            FloatStatsResult& r = h_fr[k];
            if (r.s_size < autodetect::kMinSample) return;
            if (r.overflow) { c.host = 1; return; }
            if (dtype_bits(tasks[floats[k]].dtype) == 64) autodetect::float_candidates<uint64_t>(r, c.base, c.inv, c.slot, c.bk, c.best, c.qslot);
            else autodetect::float_candidates<uint32_t>(r, c.base, c.inv, c.slot, c.bk, c.best, c.qslot);
          });
        }
        // ---- stage 2: what every candidate saves ----
        std::vector<SavedTask> st; st.reserve(ns_max);
        for (size_t k = 0; k < ni; k++) if (icand[k].slot == 0) {
          const size_t i = ints[k]; auto& e = by_n[tasks[i].n];
          icand[k].slot = (int)st.size();
          st.push_back(SavedTask{tasks[i].src, (const uint32_t*)(d_pool + e.second * 4), 2u, tasks[i].dtype, (uint32_t)e.first.size(), 0u, 0, 0, icand[k].base, icand[k].per_adj});
        }
        for (size_t k = 0; k < nf; k++) {
          const size_t i = floats[k]; FloatCand& c = fcand[k]; const void* sb = d_sbuf + k * (size_t)kAutoCap * 8;
          for (int q = 0; q < 2; q++) if (c.slot[q] == 0) { c.slot[q] = (int)st.size(); st.push_back(SavedTask{sb, nullptr, 0u, tasks[i].dtype, h_fr[k].s_size, 0u, c.base[q], c.inv[q], 0, 0.0}); }
          if (c.qslot == 0) { c.qslot = (int)st.size(); st.push_back(SavedTask{sb, nullptr, 1u, tasks[i].dtype, h_fr[k].s_size, c.bk, 0, 0, 0, c.best}); }
        }
        const SavedResult* h_sr = nullptr;
        if (!st.empty()) {
          TracePhase tp_2("  mode: stage 2 (bits saved per candidate)", stream);
          PCO_HIP_CHECK(hipMemcpyAsync(d_all + o_st, st.data(), st.size() * sizeof(SavedTask), hipMemcpyHostToDevice, stream));
          hipLaunchKernelGGL(auto_saved_kernel, dim3((uint32_t)st.size()), dim3(256), kAutoSavedLdsBytes, stream, (const SavedTask*)(d_all + o_st), (SavedResult*)(d_all + o_sr));
          PCO_HIP_CHECK(hipGetLastError());
          SavedResult* h = (SavedResult*)wsp.h_sum.ensure(st.size() * sizeof(SavedResult) + 64);
          PCO_HIP_CHECK(hipMemcpyAsync(h, d_all + o_sr, st.size() * sizeof(SavedResult), hipMemcpyDeviceToHost, stream));
          PCO_HIP_CHECK(hipStreamSynchronize(stream));
          h_sr = h;
        }
        // ---- the bids (data_types/unsigned.rs:28-37, float.rs:82-98; last maximum wins) ----
        for (size_t k = 0; k < ni; k++) {
          const size_t i = ints[k];
          if (ihost[k]) { on_host.push_back(i); continue; }
          if (icand[k].slot < 0) continue;
          const double est = h_sr[icand[k].slot].s_dbl / (double)cnts[i];
          if (est > 0.5) { plans[i].mode_kind = kIntMult; plans[i].mode_base = icand[k].base; }
        }
        for (size_t k = 0; k < nf; k++) {
          const size_t i = floats[k]; const FloatCand& c = fcand[k];
          if (c.host) { on_host.push_back(i); continue; }
          const double total = (double)h_fr[k].s_size;
          double best = 0.0; int win = 0; int which = -1;
          bool found = false; double saved = 0.0;
          for (int q = 0; q < 2; q++) if (c.slot[q] >= 0) {
            const double v = (double)h_sr[c.slot[q]].s_int / total;
            if (v >= 0.5 && (!found || !(v < saved))) { found = true; saved = v; which = q; }
          }
          if (found && !(saved < best)) { best = saved; win = 1; }
          if (c.qslot >= 0) { const double v = h_sr[c.qslot].s_dbl / total; if (v > 1.5 && !(v < best)) { best = v; win = 2; } }
          if (win == 1) {
            const int bits = dtype_bits(tasks[i].dtype);
            const uint64_t bb = c.base[which], m = 1ull << (bits - 1);
            const bool finite = bits == 64 ? ((bb >> 52) & 0x7ff) != 0x7ff : ((bb >> 23) & 0xff) != 0xff;
            if (!finite || (bb & (m - 1)) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
            plans[i].mode_kind = kFloatMult; plans[i].mode_aux2 = bb; plans[i].mode_aux = c.inv[which];
            plans[i].mode_base = (bb & m) ? (~bb & (bits == 64 ? ~0ull : 0xffffffffull)) : (bb ^ m);
          } else if (win == 2) { plans[i].mode_kind = kFloatQuant; plans[i].mode_k = c.bk; }
        }
        // ---- the test hook's records: copies of what this step holds anyway ----
        for (size_t k = 0; k < ni; k++) {
          const size_t i = ints[k]; if (i >= dbg.size()) continue;
          PcoGfxAutoModeRecord& d = dbg[i];
          d.route = ihost[k] ? 4u : 1u; d.n_entries = h_ir[k].n_entries; d.overflow = h_ir[k].overflow;
          if (!ihost[k] && icand[k].slot >= 0) { const SavedResult& sr = h_sr[icand[k].slot]; d.cand_mask = 8u; d.base[3] = icand[k].base; d.s_int[3] = sr.s_int; std::memcpy(&d.s_dbl[3], &sr.s_dbl, 8); }
        }
        for (size_t k = 0; k < nf; k++) {
          const size_t i = floats[k]; if (i >= dbg.size()) continue;
          PcoGfxAutoModeRecord& d = dbg[i]; const FloatStatsResult& r = h_fr[k]; const FloatCand& c = fcand[k];
          d.route = c.host ? 4u : (r.s_size < autodetect::kMinSample ? 0u : 2u); d.n_entries = r.n_entries; d.overflow = r.overflow; d.s_size = r.s_size;
          if (d.route != 2u) continue;
          d.tz5 = r.tz5; d.n_ints = r.n_ints; d.n_gcd = r.n_gcd; d.has_euclid = r.has_euclid; d.k = r.k; d.base_c = r.base_c;
          for (int q = 0; q < 3; q++) d.sim[q] = r.sim[q];
          for (int q = 0; q < 3; q++) {
            const int slot = q < 2 ? c.slot[q] : c.qslot; if (slot < 0) continue;
            const SavedResult& sr = h_sr[slot];
            d.cand_mask |= 1u << q; d.s_int[q] = sr.s_int; std::memcpy(&d.s_dbl[q], &sr.s_dbl, 8);
            if (q < 2) { d.base[q] = c.base[q]; d.inv[q] = c.inv[q]; } else d.bk = c.bk;
          }
        }
        std::sort(on_host.begin(), on_host.end());
      }
    }
    if (!on_host.empty()) {
      size_t total_bytes = 0;
      std::vector<size_t> off(on_host.size());
      for (size_t k = 0; k < on_host.size(); k++) { const size_t i = on_host[k]; off[k] = total_bytes; total_bytes += ((cnts[i] * (size_t)(dtype_bits(tasks[i].dtype) / 8)) + 15) & ~(size_t)15; }
      uint8_t* d_samp = (uint8_t*)wsp.auto_samp.ensure(total_bytes + 64);
      std::vector<GatherTask> g; uint32_t max_idx = 0;
      for (size_t k = 0; k < on_host.size(); k++) {
        const size_t i = on_host[k]; auto& e = by_n[tasks[i].n];
        g.push_back(GatherTask{tasks[i].src, d_samp + off[k], (const uint32_t*)(d_pool + e.second * 4), (uint32_t)e.first.size(), (uint32_t)(dtype_bits(tasks[i].dtype) / 8)});
        max_idx = std::max<uint32_t>(max_idx, (uint32_t)e.first.size());
      }
      uint8_t* h_samp = (uint8_t*)wsp.h_samp.ensure(total_bytes + 64);
      {
        TracePhase tp_g("  mode: gather + D2H", stream);
        run_gather(g, max_idx, stream, wsp.auto_tasks);
        PCO_HIP_CHECK(hipMemcpyAsync(h_samp, d_samp, total_bytes, hipMemcpyDeviceToHost, stream));
        PCO_HIP_CHECK(hipStreamSynchronize(stream));
        if (g_trace) fprintf(stderr, "[pco_gfx trace]   mode sample bytes %zu (%zu of %zu chunks)\n", total_bytes, on_host.size(), n_tasks);
      }
      TracePhase tp_d("  mode: host detect", stream);
      parallel_for_chunks(on_host.size(), [&](size_t k) {
        const size_t i = on_host[k];
        const size_t cnt = cnts[i];
        const int bits = dtype_bits(tasks[i].dtype);
        if (bits == 64) { std::vector<uint64_t> v((uint64_t*)(h_samp + off[k]), (uint64_t*)(h_samp + off[k]) + cnt); detect_mode_for<uint64_t>(v, tasks[i].dtype, plans[i]); }
        else if (bits == 32) { std::vector<uint32_t> v((uint32_t*)(h_samp + off[k]), (uint32_t*)(h_samp + off[k]) + cnt); detect_mode_for<uint32_t>(v, tasks[i].dtype, plans[i]); }
        else if (bits == 16) { std::vector<uint16_t> v((uint16_t*)(h_samp + off[k]), (uint16_t*)(h_samp + off[k]) + cnt); detect_mode_for<uint16_t>(v, tasks[i].dtype, plans[i]); }
        else { std::vector<uint8_t> v(h_samp + off[k], h_samp + off[k] + cnt); detect_mode_for<uint8_t>(v, tasks[i].dtype, plans[i]); }
      }, 1);   // (a detection is some 0.5 ms of libm and hashing: one chunk per grab)
    }
  }
  // ---------------- delta ----------------
  if (cfg.delta_kind != PCO_DELTA_AUTO) { for (size_t i = 0; i < n_tasks; i++) plan_delta_explicit(plans[i], cfg, tasks[i].n); return; }
  // 1 + 2. the delta samples (sampling.rs:27-60): primary latents at the sampled positions, split on the fly from the source numbers
  std::unique_ptr<TracePhase> tp_lists(g_trace ? new TracePhase("auto delta: sample lists", stream) : nullptr);
  std::unordered_map<uint64_t, std::pair<std::vector<uint32_t>, size_t>> by_n; size_t pool = 0, total_bytes = 0;
  for (size_t i = 0; i < n_tasks; i++) if (!by_n.count(tasks[i].n)) { auto idx = autodetect::delta_sample_indices(tasks[i].n); by_n[tasks[i].n] = {idx, pool}; pool += idx.size(); }
  std::vector<size_t> off(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) { off[i] = total_bytes; total_bytes += ((by_n[tasks[i].n].first.size() * (size_t)(dtype_bits(tasks[i].dtype) / 8)) + 15) & ~(size_t)15; }
  uint8_t* d_pool = (uint8_t*)wsp.auto_idx.ensure(pool * 4 + 64);
  uint8_t* d_samp = (uint8_t*)wsp.auto_samp.ensure(total_bytes + 64);
  for (auto& kv : by_n) if (!kv.second.first.empty()) PCO_HIP_CHECK(hipMemcpyAsync(d_pool + kv.second.second * 4, kv.second.first.data(), kv.second.first.size() * 4, hipMemcpyHostToDevice, stream));
  std::vector<SplitGatherTask> g; uint32_t max_idx = 0;
  for (size_t i = 0; i < n_tasks; i++) {
    auto& e = by_n[tasks[i].n];
    if (e.first.empty()) continue;
    g.push_back(SplitGatherTask{tasks[i].src, d_samp + off[i], (const uint32_t*)(d_pool + e.second * 4), (uint32_t)e.first.size(), tasks[i].dtype,
                                plans[i].mode_kind, plans[i].mode_k, plans[i].mode_base, plans[i].mode_aux, plans[i].mode_aux2});
    max_idx = std::max<uint32_t>(max_idx, (uint32_t)e.first.size());
  }
  if (g.empty()) { for (size_t i = 0; i < n_tasks; i++) { plans[i].delta_kind = kDeltaNone; } return; }
  tp_lists.reset();
  {
    TracePhase tp("auto delta: sample split", stream);
    SplitGatherTask* d_g = (SplitGatherTask*)wsp.auto_tasks.ensure(g.size() * sizeof(SplitGatherTask));
    PCO_HIP_CHECK(hipMemcpyAsync(d_g, g.data(), g.size() * sizeof(SplitGatherTask), hipMemcpyHostToDevice, stream));
    const uint32_t bpt = std::max<uint32_t>(1, (max_idx + 255) / 256);
    if ((uint64_t)bpt * g.size() >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many chunks in one call"};
    hipLaunchKernelGGL(split_gather_kernel, dim3(bpt * (uint32_t)g.size()), dim3(256), 0, stream, d_g, bpt);
    PCO_HIP_CHECK(hipGetLastError());
  }
  // 3. trial encodes of the sample, in waves: no delta, lookback and consecutive orders 1..2 for every sampled chunk, then two more
  //    orders at a time for the chunks whose last trial was still an improvement (choose_auto_delta_encoding stops at the first order
  //    that is not)
  struct Cand { uint32_t delta_kind, order; };
  auto run_wave = [&](const std::vector<size_t>& chunks, const std::vector<Cand>& cands) -> const TrialSummary* {
    std::vector<PcoGfxEncodeTask> tt; std::vector<EncModePlan> tp; std::vector<EncPage> tpg;
    std::unique_ptr<TracePhase> tp_prep(g_trace ? new TracePhase("auto delta: trial task lists", stream) : nullptr);
    // (candidate-major: the trials of one kind are consecutive blocks of every kernel, so whatever a kind costs is spread over all XCDs --
    //  chunk-major with four kinds put each kind on two of the eight)
    for (const Cand& c : cands) {
      for (size_t i : chunks) {
        const size_t sn = by_n[tasks[i].n].first.size();
        const int bits = dtype_bits(tasks[i].dtype);
        const uint32_t udt = bits == 64 ? PCO_TYPE_U64 : (bits == 32 ? PCO_TYPE_U32 : (bits == 16 ? PCO_TYPE_U16 : PCO_TYPE_U8));
        EncModePlan p{}; p.mode_kind = kClassic; p.ubl_override = choose_unoptimized_bins_log(cfg.level, tasks[i].n);
        p.delta_kind = c.delta_kind;
        if (c.delta_kind == kDeltaLookback) { p.window_n_log = lookback_window_log(sn); p.state_n_log = 0; }
        else if (c.delta_kind == kDeltaConsecutive) p.delta_order = c.order;
        p.n_pages = 1; p.page_low = (uint32_t)sn; p.page_r = 0; p.page_first = (uint32_t)tt.size();
        EncPage pg{}; pg.chunk = (uint32_t)tt.size(); pg.n = sn; pg.flags = 0;
        tt.push_back(PcoGfxEncodeTask{d_samp + off[i], sn, nullptr, 0, udt, 0}); tp.push_back(p); tpg.push_back(pg);
      }
    }
    tp_prep.reset();
    EncWorkspace wst{};
    { TracePhase tpp("auto delta: trial encodes", stream); run_encode(tt.size(), tt.data(), tp, tpg, cfg, nullptr, nullptr, stream, &wst, 2); }
    TracePhase tp_sum("auto delta: summaries", stream);
    TrialSummary* d_sum = (TrialSummary*)wsp.auto_sum.ensure(tt.size() * sizeof(TrialSummary));
    // log2(w) for w = 0..4096 from the host's libm (the reference's f64::log2)
    static const std::vector<double> log2_tab = make_log2_table();
    double* d_log2 = (double*)wsp.auto_log2.ensure(log2_tab.size() * 8);
    PCO_HIP_CHECK(hipMemcpyAsync(d_log2, log2_tab.data(), log2_tab.size() * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(enc_trial_summary_kernel, dim3(((uint32_t)tt.size() + 63) / 64), dim3(64), 0, stream, wst, d_sum, (uint32_t)tt.size(), (const double*)d_log2);
    TrialSummary* sums = (TrialSummary*)wsp.h_sum.ensure(tt.size() * sizeof(TrialSummary) + 64);
    PCO_HIP_CHECK(hipMemcpyAsync(sums, d_sum, tt.size() * sizeof(TrialSummary), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
    for (size_t k = 0; k < tt.size(); k++) if (sums[k].status != PCO_GFX_OK) throw HostError{(int)sums[k].status, "Auto delta trial failed"};
    return sums;
  };
  std::vector<size_t> sampled;
  for (size_t i = 0; i < n_tasks; i++) {
    plans[i].delta_kind = kDeltaNone; plans[i].delta_order = 0; plans[i].window_n_log = 0; plans[i].state_n_log = 0;
    if (!by_n[tasks[i].n].first.empty()) sampled.push_back(i);
  }
  // 4. replay choose_auto_delta_encoding (wrapped/chunk_compressor.rs:310-360) on the size estimates
  std::vector<float> best(n_tasks, 0.0f); std::vector<uint8_t> more(n_tasks, 0);
  std::vector<size_t> sns(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) sns[i] = by_n[tasks[i].n].first.size();
  {
    // First wave: no delta, lookback, consecutive orders 1 and 2 -- choose_auto_delta_encoding stops at the first order that is no
    // improvement, and most data stops at 1 or 2 (an order-3 trial for everybody was a fifth of the trial time, wasted on them).
    const std::vector<Cand> wave_a = {{kDeltaNone, 0}, {kDeltaLookback, 0}, {kDeltaConsecutive, 1}, {kDeltaConsecutive, 2}};
    const TrialSummary* sums = run_wave(sampled, wave_a);
    TracePhase tp_dec("auto delta: decisions", stream);
    parallel_for_chunks(sampled.size(), [&](size_t k) {
      const size_t i = sampled[k];
      const size_t sn = sns[i]; const int bits = dtype_bits(tasks[i].dtype);
      auto s = [&](size_t j) -> const TrialSummary& { return sums[j * sampled.size() + k]; };   // (trial j of chunk k: candidate-major)
      float best_cost = (float)trial_size(s(0), bits, 0);
      const float penalty = 0.25f * (float)sn;
      if (best_cost > penalty) {
        const float lb_cost = (float)trial_size(s(1), bits, 0x80000000u | 1u) + penalty;
        if (lb_cost < best_cost) { plans[i].delta_kind = kDeltaLookback; plans[i].window_n_log = lookback_window_log(tasks[i].n); plans[i].state_n_log = 0; best_cost = lb_cost; }
      }
      bool open_ended = true;
      for (uint32_t order = 1; order <= 2; order++) {
        const float cost = (float)trial_size(s(1 + order), bits, order);
        if (cost < best_cost) { plans[i].delta_kind = kDeltaConsecutive; plans[i].delta_order = order; plans[i].window_n_log = 0; best_cost = cost; }
        else { open_ended = false; break; }
      }
      best[i] = best_cost; more[i] = open_ended ? 1 : 0;
    });
  }
  // Further waves, two orders at a time, only for the chunks whose last trial was still an improvement (high-order differences of noisy
  // data are the expensive trials: wide value ranges)
  for (uint32_t first = 3; first <= 7; first += 2) {
    std::vector<size_t> deeper;
    for (size_t i : sampled) if (more[i]) deeper.push_back(i);
    if (deeper.empty()) break;
    std::vector<Cand> wave; for (uint32_t o = first; o <= 7 && o < first + 2; o++) wave.push_back(Cand{kDeltaConsecutive, o});
    const TrialSummary* sums = run_wave(deeper, wave);
    parallel_for_chunks(deeper.size(), [&](size_t k) {
      const size_t i = deeper[k];
      const int bits = dtype_bits(tasks[i].dtype);
      float best_cost = best[i];
      bool open_ended = true;
      for (size_t j = 0; j < wave.size(); j++) {
        const uint32_t order = wave[j].order;
        const float cost = (float)trial_size(sums[j * deeper.size() + k], bits, order);
        if (cost < best_cost) { plans[i].delta_kind = kDeltaConsecutive; plans[i].delta_order = order; plans[i].window_n_log = 0; best_cost = cost; }
        else { open_ended = false; break; }
      }
      best[i] = best_cost; more[i] = open_ended ? 1 : 0;
    });
  }
}

static size_t workspace_budget_bytes();
// Dict mode (encode_dict.hip): every chunk's dictionary and index array, on the device, before anything else.  The chunks are then
// encoded as u32 chunks of their indices (`vt`, Classic mode: `ecfg`), Auto delta included; the final encode gets the dictionaries
// through ecfg.d_dict.  Scratch, only in Dict calls: 4 bytes of indices and up to dtype_bits / 8 of dictionary per number, and, for the
// chunks with more distinct latents than the LDS table holds, an HBM table of dict_hbm_slot_bytes(n_max) -- as many as a synchronous call
// finds it needs (one read-back), one per chunk for an asynchronous one.
static DictTask* build_dicts(size_t n_tasks, const PcoGfxEncodeTask* tasks, bool sync, hipStream_t stream, std::vector<PcoGfxEncodeTask>& vt, ResolvedConfig& ecfg) {
  Workspace& wsp = workspace();
  std::vector<DictTask> dt(n_tasks);
  uint64_t n_max = 0;
  size_t off = (n_tasks * sizeof(DictTask) + 255) & ~(size_t)255;
  const size_t off_ctr = off; off += 256;
  std::vector<size_t> idx_off(n_tasks), val_off(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) {
    n_max = std::max<uint64_t>(n_max, tasks[i].n);
    idx_off[i] = off; off += (tasks[i].n * 4 + 255) & ~(size_t)255;
    val_off[i] = off; off += (tasks[i].n * (size_t)(dtype_bits(tasks[i].dtype) / 8) + 255) & ~(size_t)255;
  }
  const size_t budget = workspace_budget_bytes();
  const size_t slot_bytes = dict_hbm_slot_bytes(n_max);
  if (off + (sync ? 0 : n_tasks * slot_bytes) > budget) throw HostError{PCO_GFX_DEVICE_ERROR, "Dict scratch exceeds the workspace budget (PCO_GFX_WORKSPACE_GB)", true};
  uint8_t* d = (uint8_t*)wsp.enc_dict.ensure(off);
  for (size_t i = 0; i < n_tasks; i++)
    dt[i] = DictTask{tasks[i].src, (uint32_t*)(d + idx_off[i]), d + val_off[i], tasks[i].n, tasks[i].dtype, 0u, kNoDictSlot, 0u};
  DictTask* d_dt = (DictTask*)d;
  uint32_t* d_over = (uint32_t*)(d + off_ctr);
  PCO_HIP_CHECK(hipMemcpyAsync(d_dt, dt.data(), n_tasks * sizeof(DictTask), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemsetAsync(d_over, 0, 4, stream));
  static const bool lds_ok = hipFuncSetAttribute((const void*)enc_dict_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDictLdsBytes) == hipSuccess;
  if (!lds_ok) throw HostError{PCO_GFX_DEVICE_ERROR, "cannot reserve LDS for enc_dict_lds_kernel"};
  const uint32_t nt = (uint32_t)n_tasks;
  PCO_TIMED_LAUNCH("enc_dict_lds_kernel", stream, enc_dict_lds_kernel, dim3(nt), dim3(kDictThreads), kDictLdsBytes, stream, d_dt, nt, d_over);
  uint32_t n_over = nt;
  if (sync) {
    PCO_HIP_CHECK(hipMemcpyAsync(&n_over, d_over, 4, hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
  if (n_over) {
    if (off + n_over * slot_bytes > budget) throw HostError{PCO_GFX_DEVICE_ERROR, "Dict scratch exceeds the workspace budget (PCO_GFX_WORKSPACE_GB)", true};
    uint8_t* d_slots = (uint8_t*)wsp.enc_dict_hbm.ensure(n_over * slot_bytes);
    PCO_TIMED_LAUNCH("enc_dict_hbm_kernel", stream, enc_dict_hbm_kernel, dim3(nt), dim3(kDictThreads), 0, stream, d_dt, nt, d_slots, (uint64_t)slot_bytes, n_max);
  }
  PCO_HIP_CHECK(hipGetLastError());
  vt.resize(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) vt[i] = PcoGfxEncodeTask{dt[i].idx, tasks[i].n, tasks[i].dst, tasks[i].dst_cap, PCO_TYPE_U32, 0};
  ecfg.mode_kind = PCO_MODE_CLASSIC;   // (ecfg.d_dict is set by the caller once the plans are resolved: the Auto-delta trials are plain u32 chunks)
  return d_dt;
}

// batched standalone chunks: one page per chunk, preamble + meta + page into task.dst
static void launch_encode(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, PcoGfxTaskResult* results,
                          PcoGfxTaskResult* d_results_user, hipStream_t stream) {
  if (n_tasks == 0) return;
  std::vector<EncModePlan> plans(n_tasks);
  std::vector<EncPage> pages(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) validate_task(tasks[i], cfg, true);
  std::vector<PcoGfxEncodeTask> vt; ResolvedConfig ecfg = cfg; DictTask* d_dict = nullptr;
  if (cfg.mode_kind == PCO_MODE_TRY_DICT) { d_dict = build_dicts(n_tasks, tasks, results != nullptr, stream, vt, ecfg); tasks = vt.data(); }
  { TracePhase tp("resolve_plans (total)", stream); resolve_plans(n_tasks, tasks, ecfg, plans, stream); }
  ecfg.d_dict = d_dict;
  TracePhase tp_final("final encode", stream);
  for (size_t i = 0; i < n_tasks; i++) {
    plans[i].n_pages = 1; plans[i].page_low = (uint32_t)tasks[i].n; plans[i].page_r = 0; plans[i].page_first = (uint32_t)i;
    EncPage p{}; p.chunk = (uint32_t)i; p.page_idx = 0; p.start = 0; p.n = tasks[i].n; p.dst = tasks[i].dst; p.dst_cap = tasks[i].dst_cap; p.flags = kPageFlagPreamble;
    pages[i] = p;
  }
  run_encode(n_tasks, tasks, plans, pages, ecfg, results, d_results_user, stream);
}

// Room for a ChunkMeta (metadata/chunk.rs:105-125): up to three variables of 2^unoptimized_bins_log bins of (ans_size_log + L::BITS + offset-bits
// field) bits each -- 256 bins up to level 8 (8 KB for three 64-bit variables), 4096 from level 9 on (43 KB for the primary, 25 KB for a lookback
// variable, the secondary never has more than 64: wrapped/chunk_compressor.rs:238-248).
static size_t wrapped_meta_cap(uint32_t level) { return level > 8 ? (size_t)96 << 10 : (size_t)16 << 10; }
static size_t wrapped_page_cap(int bits, size_t page_n) { return (guarantee_standalone_chunk_size(bits, page_n) + 64 + 15) & ~(size_t)15; }
// Dict mode: the ChunkMeta also holds the dictionary (up to one latent per number, behind a 4-byte header), and a page holds u32 indices
static bool dict_call(const ResolvedConfig& c) { return c.dict && c.mode_kind == PCO_MODE_TRY_DICT; }
static size_t chunk_meta_cap(const ResolvedConfig& c, int bits, size_t n) { return wrapped_meta_cap(c.level) + (dict_call(c) ? ((4 + n * (size_t)(bits / 8) + 15) & ~(size_t)15) : 0); }
static size_t chunk_page_cap(const ResolvedConfig& c, int bits, size_t page_n) { return wrapped_page_cap(dict_call(c) ? std::max(bits, 32) : bits, page_n); }

// The page lists of a wrapped call, chunk after chunk: sizes[first[i] .. first[i + 1]) are chunk i's pages (PagingSpec::Exact as given,
// else what EqualPagesUpTo cuts).  Built -- and every argument checked -- before anything is launched.
struct WrappedPaging { std::vector<uint64_t> sizes; std::vector<size_t> first; std::vector<uint8_t> exact; uint64_t page_max = 0; };
static void plan_wrapped_paging(size_t n_tasks, const PcoGfxWrappedTask* wt, const ResolvedConfig& cfg, WrappedPaging& pg) {
  pg.first.assign(n_tasks + 1, 0); pg.exact.assign(n_tasks, 0); pg.sizes.clear(); pg.page_max = 0;
  std::vector<size_t> pn;
  for (size_t i = 0; i < n_tasks; i++) {
    const PcoGfxWrappedTask& t = wt[i];
    validate_task(PcoGfxEncodeTask{t.src, t.n, t.dst, t.dst_cap, t.dtype, 0}, cfg, true);
    if ((uintptr_t)t.dst & 15) throw HostError{PCO_GFX_INVALID_ARGUMENT, "wrapped chunk " + std::to_string(i) + ": dst must be 16-byte aligned"};
    if ((t.n_pages != 0) != (t.page_sizes != nullptr)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "wrapped chunk " + std::to_string(i) + ": page_sizes must be NULL exactly when n_pages is 0"};
    const int bits = dtype_bits(t.dtype);
    uint64_t need = chunk_meta_cap(cfg, bits, t.n);
    if (t.n_pages) {   // PagingSpec::Exact (chunk_config.rs:162-180)
      uint64_t sum = 0; for (uint32_t k = 0; k < t.n_pages; k++) sum += t.page_sizes[k];
      if (sum != t.n) throw HostError{PCO_GFX_INVALID_ARGUMENT, "paging spec suggests " + std::to_string(sum) + " numbers but " + std::to_string(t.n) + " were given"};
      for (uint32_t k = 0; k < t.n_pages; k++) if (t.page_sizes[k] == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot write data page of 0 numbers"};
      pg.sizes.insert(pg.sizes.end(), t.page_sizes, t.page_sizes + t.n_pages); pg.exact[i] = 1;
    } else { n_per_page(cfg.max_page_n, t.n, pn); pg.sizes.insert(pg.sizes.end(), pn.begin(), pn.end()); }
    pg.first[i + 1] = pg.sizes.size();
    for (size_t k = pg.first[i]; k < pg.first[i + 1]; k++) { need += chunk_page_cap(cfg, bits, pg.sizes[k]); pg.page_max = std::max(pg.page_max, pg.sizes[k]); }
    if (need > t.dst_cap) throw HostError{PCO_GFX_INVALID_ARGUMENT, "wrapped chunk " + std::to_string(i) + ": dst_cap is below pco_gfx_wrapped_chunk_cap"};
  }
  if (pg.sizes.size() + n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many pages in one call"};
}

// batched wrapped chunks (pco_gfx_compress_wrapped_chunks[_ex]), chunks [at, at + n_tasks) of a call whose paging is planned: per chunk a
// ChunkMeta-only "page" and its data pages, all through ONE pass of the pipeline -- the (page, variable) items of every chunk are walked side by
// side, which is what pages buy (wrapped/chunk_compressor.rs:164-213).  infos == nullptr: asynchronous (d_infos alone, in stream order).
static void launch_encode_wrapped(size_t at, size_t n_tasks, const PcoGfxWrappedTask* wt, const WrappedPaging& pg, const ResolvedConfig& cfg, PcoGfxPageInfo* infos,
                                  PcoGfxPageInfo* d_infos, hipStream_t stream) {
  if (n_tasks == 0) return;
  wt += at;
  const bool sync = infos != nullptr;
  std::vector<EncModePlan> plans(n_tasks);
  std::vector<EncPage> pages;
  std::vector<PcoGfxEncodeTask> otasks(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) otasks[i] = PcoGfxEncodeTask{wt[i].src, wt[i].n, wt[i].dst, wt[i].dst_cap, wt[i].dtype, 0};
  const PcoGfxEncodeTask* tasks = otasks.data();
  std::vector<PcoGfxEncodeTask> vt; ResolvedConfig ecfg = cfg; DictTask* d_dict = nullptr;
  if (cfg.mode_kind == PCO_MODE_TRY_DICT) { d_dict = build_dicts(n_tasks, tasks, sync, stream, vt, ecfg); tasks = vt.data(); }
  resolve_plans(n_tasks, tasks, ecfg, plans, stream);
  ecfg.d_dict = d_dict;
  std::vector<uint64_t> offs;   // per entry of `pages`: its offset from the chunk's dst
  for (size_t i = 0; i < n_tasks; i++) {
    const int bits = dtype_bits(otasks[i].dtype);
    const size_t meta_cap = chunk_meta_cap(cfg, bits, tasks[i].n);
    const uint64_t* pn = pg.sizes.data() + pg.first[at + i]; const size_t np = pg.first[at + i + 1] - pg.first[at + i];
    uint64_t off = 0;
    { EncPage p{}; p.chunk = (uint32_t)i; p.n = 0; p.dst = tasks[i].dst; p.dst_cap = meta_cap; p.flags = kPageFlagMetaOnly; pages.push_back(p); offs.push_back(0); off = meta_cap; }
    plans[i].n_pages = (uint32_t)np; plans[i].page_low = (uint32_t)(tasks[i].n / np); plans[i].page_r = (uint32_t)(tasks[i].n % np);
    plans[i].page_first = (uint32_t)pages.size(); plans[i].exact_paging = pg.exact[at + i];
    uint64_t start = 0;
    for (size_t k = 0; k < np; k++) {
      const size_t cap = chunk_page_cap(cfg, bits, pn[k]);
      EncPage p{}; p.chunk = (uint32_t)i; p.page_idx = (uint32_t)k; p.start = start; p.n = pn[k]; p.dst = (uint8_t*)tasks[i].dst + off; p.dst_cap = cap; p.flags = 0;
      pages.push_back(p); offs.push_back(off); off += cap; start += pn[k];
    }
  }
  std::vector<PcoGfxTaskResult> res(sync ? pages.size() : 0);
  run_encode(n_tasks, tasks, plans, pages, ecfg, sync ? res.data() : nullptr, nullptr, stream, nullptr, 0, d_infos);
  if (sync) for (size_t k = 0; k < pages.size(); k++) infos[k] = PcoGfxPageInfo{offs[k], res[k].n_out, pages[k].n, res[k].status, res[k].aux};
}

// The encode workspace is ~8 bytes of scratch per byte of input in the worst case (full-width latents of up to three variables,
// two sort buffers, symbols, tANS fields): 130 GB for 16 GiB of numbers.  A synchronous call whose workspace would not fit the
// budget -- PCO_GFX_WORKSPACE_GB, default 80 % of the device memory that is free (plus what the workspace already holds) -- is
// run as consecutive sub-batches of chunks through the same buffers; a device allocation that fails anyway halves the sub-batch.
// (Asynchronous calls cannot be cut -- the caller owns the ordering -- and take what they need.)
static size_t workspace_budget_bytes() {
  static const char* env = std::getenv("PCO_GFX_WORKSPACE_GB");
  if (env && *env) return (size_t)(std::atof(env) * 1e9);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ~(size_t)0;
  Workspace& w = workspace();
  const size_t held = w.enc_lat.cap + w.enc_lat2.cap + w.enc_sort.cap + w.enc_ans.cap + w.enc_sym.cap + w.enc_answ.cap + w.enc_state.cap + w.enc_small.cap + w.enc_bat.cap + w.enc_run.cap + w.enc_fstate.cap + w.enc_lb.cap + w.enc_lbprops.cap + w.enc_walk.cap + w.enc_vlut.cap +
                      w.enc_dict.cap + w.enc_dict_hbm.cap;
  return (size_t)((free_b + held) * 0.8);
}
// `launch(at, k)` encodes chunks [at, at + k); `extra_per_task` is what the caller's chunks take beyond the standalone figure (the wrapped surface's
// per-page records), `key_salt` keeps the remembered footprints of different surfaces apart.  With measure_only the worst-case bytes of ONE pass
// over all chunks are returned and nothing is launched.
template <class Launch>
static size_t encode_in_passes(size_t n_tasks, uint64_t n_max, const ResolvedConfig& cfg, size_t extra_per_task, uint64_t key_salt, bool measure_only, hipStream_t stream, Launch&& launch) {
  const size_t stride = ((n_max + 255) & ~(uint64_t)255) + 256;
  const size_t slots = (cfg.mode_kind == PCO_MODE_CLASSIC ? 1 : 2) + ((cfg.delta_kind == PCO_DELTA_TRY_LOOKBACK || cfg.delta_kind == PCO_DELTA_AUTO) ? 1 : 0);
  // (a spec that may end in a lookback delta, and strict histograms, also take the two sort buffers -- 16 B per number -- and, for lookback, the six
  //  proposal streams (12 B per number), the last-index / count scratch and the walk records: left out of this figure until round 5, a call of 12 288
  //  mixed chunks under the default ChunkConfig ran into the allocation failure below at EVERY call, and releasing and re-allocating ~150 GB took
  //  0.7 s of an 0.8 s step)
  const bool may_lookback = cfg.delta_kind == PCO_DELTA_TRY_LOOKBACK || cfg.delta_kind == PCO_DELTA_AUTO;
  const size_t per_task = stride * (slots * (8 + 4 + 1 + 2) + 16 + ((may_lookback || cfg.strict_hist || cfg.delta_kind == PCO_DELTA_TRY_CONV1) ? 16 : 0) + (may_lookback ? 12 : 0)) + (may_lookback ? (size_t)700 << 10 : 0) + 3 * kWalkRecBytes +
                          sizeof(EncChunk) + 3 * plan_bytes_for(cfg.level > 8 ? kBigBins : kMaxBins) +
                          (dict_call(cfg) ? stride * 12 + dict_hbm_slot_bytes(n_max) : 0) +   // (Dict: indices, dictionary, an HBM table in the worst case)
                          extra_per_task;
  // (buffers are allocated with an eighth of slack; passes are balanced: the walkers' latency is paid once per pass whatever its size,
  //  so 7800 + 392 chunks cost what 2 x 7800 would).  The estimate above is the worst case of the spec -- Auto may end up with two
  //  variables and a lookback slot, or with one and none -- so what a call of the same spec and chunk size really took is remembered
  //  (per thread) and used from then on; if other data needs more after all, the allocation failure below halves the pass.
  size_t est = per_task + per_task / 8;
  if (measure_only) return est * n_tasks;
  static thread_local std::unordered_map<uint64_t, size_t> seen_per_task;   // size_t(-1): an attempt on the remembered figure failed, the worst case stays
  static thread_local std::unordered_map<uint64_t, size_t> pass_cap;         // ... and the pass size that then went through: later calls of the spec start there, not at the wall
  const uint64_t spec_key = ((uint64_t)cfg.mode_kind | ((uint64_t)cfg.delta_kind << 4) | ((uint64_t)cfg.level << 8) | ((uint64_t)(cfg.strict_hist ? 1u : 0u) << 12) | ((uint64_t)stride << 16)) ^ key_salt;   // (strict histograms take the two sort buffers: a footprint of their own)
  { auto f = seen_per_task.find(spec_key); if (f != seen_per_task.end() && f->second != ~(size_t)0) est = std::min(est, f->second + f->second / 8); }
  size_t batch = std::max<size_t>(64, std::min<size_t>(n_tasks, workspace_budget_bytes() / est));
  { auto f = pass_cap.find(spec_key); if (f != pass_cap.end()) batch = std::max<size_t>(64, std::min(batch, f->second)); }
  if (batch < n_tasks) { const size_t passes = (n_tasks + batch - 1) / batch; batch = std::max<size_t>(64, (n_tasks + passes - 1) / passes); }
  auto held_now = []() { Workspace& w = workspace(); return w.enc_lat.cap + w.enc_lat2.cap + w.enc_sort.cap + w.enc_ans.cap + w.enc_sym.cap + w.enc_answ.cap + w.enc_state.cap + w.enc_small.cap + w.enc_bat.cap + w.enc_run.cap + w.enc_fstate.cap + w.enc_lb.cap + w.enc_lbprops.cap + w.enc_walk.cap + w.enc_vlut.cap; };
  size_t largest_pass = 0; bool failed = false;
  for (size_t at = 0; at < n_tasks;) {
    const size_t k = std::min(batch, n_tasks - at);
    try {
      launch(at, k);
      at += k; largest_pass = std::max(largest_pass, k);
    } catch (const HostError& e) {
      if (!e.oom || batch <= 64) throw;
      (void)hipGetLastError();
      (void)hipStreamSynchronize(stream);   // kernels of the failed pass may still be using the buffers
      workspace().release_all();   // start over with half the chunks per pass
      batch = std::max<size_t>(64, batch / 2);
      failed = true;
    }
  }
  // (what the buffers hold is an upper bound of the need: they never shrink.  After a failed attempt the spec stays on the worst-case
  //  estimate for good, so that later calls do not walk into the same wall)
  if (failed) { seen_per_task[spec_key] = ~(size_t)0; if (largest_pass >= 64) pass_cap[spec_key] = largest_pass; }
  else if (largest_pass >= 64 && (!seen_per_task.count(spec_key) || seen_per_task[spec_key] != ~(size_t)0)) seen_per_task[spec_key] = held_now() / largest_pass + 1;
  return est * n_tasks;
}
static void encode_in_sub_batches(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, PcoGfxTaskResult* results,
                                  PcoGfxTaskResult* d_results, hipStream_t stream) {
  if (!results || n_tasks <= 64) { launch_encode(n_tasks, tasks, cfg, results, d_results, stream); return; }
  uint64_t n_max = 0; for (size_t i = 0; i < n_tasks; i++) n_max = std::max<uint64_t>(n_max, tasks[i].n);
  encode_in_passes(n_tasks, n_max, cfg, 0, 0, false, stream, [&](size_t at, size_t k) { launch_encode(k, tasks + at, cfg, results + at, d_results ? d_results + at : nullptr, stream); });
}
// What a wrapped chunk's pages add to the per-task figure: per piece the EncPage, its result and info, the final states and the body record, the
// Conv1 state, and the batch / run tables sized by the call's longest page.
static size_t wrapped_extra_per_task(size_t n_tasks, const WrappedPaging& pg) {
  const uint64_t max_batches = (pg.page_max + kBatchN - 1) / kBatchN;
  const size_t per_piece = sizeof(EncPage) + sizeof(PcoGfxTaskResult) + 12 * 4 + 16 + kConv1MaxOrder * sizeof(uint32_t) + 3 * (size_t)(max_batches + 1) * 8 + ((max_batches + kRunBatches - 1) / kRunBatches + 2) * 8;
  const size_t pieces = pg.sizes.size() + n_tasks;
  return (pieces * per_piece + n_tasks - 1) / std::max<size_t>(n_tasks, 1);
}
// the synchronous form of the wrapped writer in passes of whole chunks; infos / d_infos advance by the pieces of each pass
static void encode_wrapped_in_passes(size_t n_tasks, const PcoGfxWrappedTask* wt, const WrappedPaging& pg, const ResolvedConfig& cfg, PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos,
                                     hipStream_t stream) {
  if (!infos || n_tasks <= 64) { launch_encode_wrapped(0, n_tasks, wt, pg, cfg, infos, d_infos, stream); return; }
  uint64_t n_max = 0; for (size_t i = 0; i < n_tasks; i++) n_max = std::max<uint64_t>(n_max, wt[i].n);
  const size_t extra = wrapped_extra_per_task(n_tasks, pg);
  encode_in_passes(n_tasks, n_max, cfg, extra, (1ull << 13) | ((uint64_t)(extra >> 6) << 44), false, stream, [&](size_t at, size_t k) {
    const size_t piece0 = pg.first[at] + at;   // pieces before chunk `at`: its predecessors' pages and ChunkMetas
    launch_encode_wrapped(at, k, wt, pg, cfg, infos + piece0, d_infos ? d_infos + piece0 : nullptr, stream);
  });
}

// standalone::simple_compress / simple_compress_into on host buffers (standalone/simple.rs:22-91)
static size_t simple_compress_host(const void* nums, size_t n, unsigned char dtype, const ResolvedConfig& cfg, bool uniform_type,
                                   void* dst, size_t dst_cap, const size_t* exact_pages = nullptr, size_t n_exact = 0) {
  const int bits = dtype_bits(dtype);
  validate_config(cfg, bits);
  const size_t esz = (size_t)bits / 8;
  uint8_t* out = (uint8_t*)dst; size_t pos = 0;
  std::vector<size_t> pages;
  if (exact_pages) {   // PagingSpec::Exact decides where the chunks are cut (standalone/simple.rs:32-36, chunk_config.rs:162-180)
    pages.assign(exact_pages, exact_pages + n_exact);
    size_t sum = 0; for (size_t x : pages) sum += x;
    if (sum != n) throw HostError{PCO_GFX_INVALID_ARGUMENT, "paging spec suggests " + std::to_string(sum) + " numbers but " + std::to_string(n) + " were given"};
    for (size_t x : pages) if (x == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot write data page of 0 numbers"};
  } else n_per_page(cfg.max_page_n, n, pages);
  // a request that can be refused from its sizes alone is refused before a byte of dst is written (validate_task would refuse it after the header)
  for (size_t x : pages) if (x > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, "count may not exceed 2^24 per chunk"};
  size_t h = pco_gfx_write_standalone_header(out, dst_cap, n, uniform_type ? dtype : 0);
  if (h == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "destination too small"};
  pos += h;
  if (!pages.empty()) {
    require_device();
    Workspace& wsp = workspace();
    WorkspaceUse use(wsp, 0);
    uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(n * esz + 64);
    std::vector<size_t> caps(pages.size()), offs(pages.size());
    size_t total_cap = 0;
    for (size_t i = 0; i < pages.size(); i++) { caps[i] = (guarantee_standalone_chunk_size(bits, pages[i]) + 64 + 15) & ~(size_t)15; offs[i] = total_cap; total_cap += caps[i]; }
    uint8_t* d_out = (uint8_t*)wsp.io_out.ensure(total_cap);
    PCO_HIP_CHECK(hipMemcpyAsync(d_in, nums, n * esz, hipMemcpyHostToDevice, 0));
    std::vector<PcoGfxEncodeTask> tasks(pages.size());
    size_t start = 0;
    for (size_t i = 0; i < pages.size(); i++) { tasks[i] = PcoGfxEncodeTask{d_in + start * esz, pages[i], d_out + offs[i], caps[i], dtype, 0}; start += pages[i]; }
    std::vector<PcoGfxTaskResult> res(pages.size());
    launch_encode(pages.size(), tasks.data(), cfg, res.data(), nullptr, 0);
    for (size_t i = 0; i < pages.size(); i++) {
      if (res[i].status != PCO_GFX_OK) throw HostError{(int)res[i].status, "chunk " + std::to_string(i) + " failed to compress"};
      if (pos + res[i].n_out > dst_cap) throw HostError{PCO_GFX_INVALID_ARGUMENT, "destination too small"};
      PCO_HIP_CHECK(hipMemcpy(out + pos, d_out + offs[i], res[i].n_out, hipMemcpyDeviceToHost));
      pos += res[i].n_out;
    }
  }
  if (pos + 1 > dst_cap) throw HostError{PCO_GFX_INVALID_ARGUMENT, "destination too small"};
  out[pos++] = 0;
  return pos;
}

}  // namespace pcogfx

extern "C" {

enum PcoError pco_gfx_compress_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config,
                                      PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    require_device();
    {
      WorkspaceUse use(workspace(), (hipStream_t)stream);
      TracePhase tp_all("compress_chunks (total)", (hipStream_t)stream);
      encode_in_sub_batches(n_tasks, tasks, resolve_config(config), results, d_results, (hipStream_t)stream);
    }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "encode task " + std::to_string(i) + " failed");
      return PcoCompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

size_t pco_gfx_wrapped_n_pages(size_t n, uint64_t max_page_n) {
  if (n == 0) return 0;
  if (max_page_n == 0) max_page_n = 1u << 18;
  return (n + max_page_n - 1) / max_page_n;
}
size_t pco_gfx_wrapped_chunk_cap(size_t n, unsigned char dtype, const PcoChunkConfigEx* config) {
  const int bits = dtype_bits(dtype);
  if (!bits || n == 0) return 0;
  const ResolvedConfig cfg = resolve_config(config);
  std::vector<size_t> pn; n_per_page(cfg.max_page_n, n, pn);
  size_t total = chunk_meta_cap(cfg, bits, n);
  for (size_t x : pn) total += chunk_page_cap(cfg, bits, x);
  return total;
}
size_t pco_gfx_wrapped_chunk_cap_exact(const uint64_t* page_sizes, size_t n_pages, unsigned char dtype, const PcoChunkConfigEx* config) {
  const int bits = dtype_bits(dtype);
  if (!bits || !page_sizes || n_pages == 0) return 0;
  const ResolvedConfig cfg = resolve_config(config);
  size_t n = 0;
  for (size_t k = 0; k < n_pages; k++) { if (page_sizes[k] == 0) return 0; n += page_sizes[k]; }
  size_t total = chunk_meta_cap(cfg, bits, n);
  for (size_t k = 0; k < n_pages; k++) total += chunk_page_cap(cfg, bits, page_sizes[k]);
  return total;
}
static enum PcoError compress_wrapped_impl(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config, PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos, void* stream) {
  clear_error();
  try {
    require_device();
    if (!infos && !d_infos) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null infos and d_infos"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null tasks"};
    const ResolvedConfig cfg = resolve_config(config);
    WrappedPaging pg;
    plan_wrapped_paging(n_tasks, tasks, cfg, pg);
    const size_t n_infos = pg.sizes.size() + n_tasks;
    {
      WorkspaceUse use(workspace(), (hipStream_t)stream);
      encode_wrapped_in_passes(n_tasks, tasks, pg, cfg, infos, d_infos, (hipStream_t)stream);
    }
    if (infos) for (size_t k = 0; k < n_infos; k++) if (infos[k].status != PCO_GFX_OK) {
      set_error((int)infos[k].status, "wrapped encode: piece " + std::to_string(k) + " failed");
      return PcoCompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}
enum PcoError pco_gfx_compress_wrapped_chunks_ex(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config, PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos,
                                                 void* stream) {
  return compress_wrapped_impl(n_tasks, tasks, config, infos, d_infos, stream);
}
enum PcoError pco_gfx_compress_wrapped_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config, PcoGfxPageInfo* infos, void* stream) {
  PcoGfxPageInfo none{};   // (a call without chunks needs no infos)
  std::vector<PcoGfxWrappedTask> wt(tasks ? n_tasks : 0);
  for (size_t i = 0; i < wt.size(); i++) wt[i] = PcoGfxWrappedTask{tasks[i].src, tasks[i].n, tasks[i].dst, tasks[i].dst_cap, tasks[i].dtype, 0, nullptr};
  return compress_wrapped_impl(n_tasks, tasks ? wt.data() : nullptr, config, infos || n_tasks ? infos : &none, nullptr, stream);
}
size_t pco_gfx_wrapped_scratch_estimate(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config) {
  clear_error();
  try {
    if (n_tasks == 0 || !tasks) return 0;
    const ResolvedConfig cfg = resolve_config(config);
    WrappedPaging pg;
    plan_wrapped_paging(n_tasks, tasks, cfg, pg);
    uint64_t n_max = 0; for (size_t i = 0; i < n_tasks; i++) n_max = std::max<uint64_t>(n_max, tasks[i].n);
    return encode_in_passes(n_tasks, n_max, cfg, wrapped_extra_per_task(n_tasks, pg), 0, true, nullptr, [](size_t, size_t) {});
  } catch (const HostError& e) { set_error(e.status, e.msg); return 0; }
}

enum PcoError pco_gfx_compact_wrapped_chunks(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config, const PcoGfxPageInfo* d_infos, uint32_t gap, void* d_dst,
                                             uint64_t dst_cap, uint64_t dst_offset, uint64_t* d_offsets, uint64_t* total, void* stream_) {
  clear_error();
  try {
    require_device();
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_infos || !d_offsets || (!d_dst && dst_cap) || (n_tasks && !tasks)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: null array"};
    const ResolvedConfig cfg = resolve_config(config);
    std::vector<WcChunk> chunks(n_tasks);
    uint64_t n_pieces = 0;
    for (size_t i = 0; i < n_tasks; i++) {
      const uint64_t np = 1 + (tasks[i].n_pages ? tasks[i].n_pages : pco_gfx_wrapped_n_pages(tasks[i].n, cfg.max_page_n));
      if (n_pieces + np >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: too many pieces for one call"};
      chunks[i] = WcChunk{(const uint8_t*)tasks[i].dst, tasks[i].dst_cap, (uint32_t)n_pieces, (uint32_t)np};
      n_pieces += np;
    }
    Workspace& ws = workspace();
    WorkspaceUse use(ws, stream);
    // scratch: the overflow flag | the chunk records | per piece its chunk (or "dropped") | the slice prefix (n_pieces + 1)
    const size_t off_chunks = 64, off_pc = (off_chunks + n_tasks * sizeof(WcChunk) + 63) & ~(size_t)63, off_pfx = (off_pc + n_pieces * 4 + 63) & ~(size_t)63;
    uint8_t* d_base = (uint8_t*)ws.compact_tasks.ensure(off_pfx + (n_pieces + 1) * 4 + 64);
    uint32_t* d_over = (uint32_t*)d_base; WcChunk* d_chunks = (WcChunk*)(d_base + off_chunks); uint32_t* d_pc = (uint32_t*)(d_base + off_pc); uint32_t* d_pfx = (uint32_t*)(d_base + off_pfx);
    if (n_tasks) {
      PCO_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), n_tasks * sizeof(WcChunk), hipMemcpyHostToDevice, stream));
      PCO_TIMED_LAUNCH("wcompact_valid_kernel", stream, wcompact_valid_kernel, dim3((uint32_t)((n_tasks + 3) / 4)), dim3(256), 0, stream, d_chunks, d_infos, d_pc, (uint32_t)n_tasks);
    }
    PCO_TIMED_LAUNCH("wcompact_scan_kernel", stream, wcompact_scan_kernel, dim3(1), dim3(1024), 0, stream, d_infos, d_pc, (uint32_t)n_pieces, gap, dst_offset, dst_cap, d_offsets, d_pfx, d_over);
    if (n_pieces) {
      if (!ws.n_cus) { int dev = 0; hipDeviceProp_t pr; ws.n_cus = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256; }
      PCO_TIMED_LAUNCH("wcompact_copy_kernel", stream, wcompact_copy_kernel, dim3(4u * (uint32_t)ws.n_cus), dim3(256), 0, stream, d_chunks, d_infos, d_pc, d_offsets, d_pfx, (uint8_t*)d_dst, (uint32_t)n_pieces, gap);
    }
    PCO_HIP_CHECK(hipGetLastError());
    if (total) {
      uint32_t over = 0;
      PCO_HIP_CHECK(hipMemcpyAsync(total, d_offsets + n_pieces, 8, hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipStreamSynchronize(stream));
      if (over) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: destination too small"};
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

enum PcoError pco_gfx_simple_compress_into_ex(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config,
                                              int uniform_type, void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  if (!dtype_bits(dtype)) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    const size_t w = simple_compress_host(nums, n, dtype, resolve_config(config), uniform_type != 0, dst, dst_cap);
    if (n_written) *n_written = w;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

enum PcoError pco_gfx_simple_compress_into_exact(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config,
                                                 int uniform_type, const size_t* page_sizes, size_t n_pages, void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  if (!dtype_bits(dtype)) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    static const size_t none = 0;
    const size_t w = simple_compress_host(nums, n, dtype, resolve_config(config), uniform_type != 0, dst, dst_cap, page_sizes && n_pages ? page_sizes : &none, n_pages);
    if (n_written) *n_written = w;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

enum PcoError pco_standalone_simple_compress_into(const void* nums, size_t n, unsigned char dtype, const struct PcoChunkConfig* config,
                                                  void* dst, size_t dst_cap, size_t* n_written) {
  // pco_c/src/lib.rs:34-55: level + EqualPagesUpTo(max_page_n), Auto mode, Auto delta, enable_8_bit
  PcoChunkConfigEx ex{};
  ex.compression_level = config ? config->compression_level : 8;
  ex.max_page_n = config ? config->max_page_n : 0;
  ex.mode_kind = PCO_MODE_AUTO; ex.delta_kind = PCO_DELTA_AUTO; ex.enable_8_bit = 1;
  return pco_gfx_simple_compress_into_ex(nums, n, dtype, &ex, 1, dst, dst_cap, n_written);
}

}  // extern "C"

// =========================================================================================================
// wrapped surface (host buffers): ChunkCompressor / ChunkDecompressor handles
// =========================================================================================================
struct PcoGfxChunkCompressor {
  std::vector<uint8_t> meta;
  std::vector<std::vector<uint8_t>> pages;
  std::vector<size_t> page_n;
  size_t meta_size_hint = 0;
  std::vector<size_t> page_size_hints;
};
struct PcoGfxChunkDecompressor {
  std::vector<uint8_t> meta;
  uint8_t dtype = 0, format_major = 4;
};
struct PcoGfxPageDecompressor {
  std::vector<uint8_t> nums;   // the decoded page (host)
  size_t elem = 0, n = 0, pos = 0, consumed = 0;
  size_t n_ok = 0; int bad_status = 0;   // a page that failed inside its body: the numbers of the batches before the failing one, and the error the call that reaches it gets
};

namespace pcogfx {

static PcoGfxChunkCompressor* chunk_compressor_build(const void* nums, size_t n, unsigned char dtype, const ResolvedConfig& cfg, const size_t* exact_pages = nullptr, size_t n_exact = 0) {
  const int bits = dtype_bits(dtype);
  if (!bits) throw HostError{PCO_GFX_INVALID_ARGUMENT, "invalid dtype"};
  const size_t esz = (size_t)bits / 8;
  require_device();
  Workspace& wsp = workspace();
  WorkspaceUse use(wsp, 0);
  std::vector<size_t> pn;
  if (exact_pages) {   // PagingSpec::Exact (chunk_config.rs:162-180)
    pn.assign(exact_pages, exact_pages + n_exact);
    size_t sum = 0; for (size_t x : pn) sum += x;
    if (sum != n) throw HostError{PCO_GFX_INVALID_ARGUMENT, "paging spec suggests " + std::to_string(sum) + " numbers but " + std::to_string(n) + " were given"};
    for (size_t x : pn) if (x == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot write data page of 0 numbers"};
  } else n_per_page(cfg.max_page_n, n, pn);
  if (pn.empty()) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot compress empty chunk"};
  uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(n * esz + 64);
  PCO_HIP_CHECK(hipMemcpyAsync(d_in, nums, n * esz, hipMemcpyHostToDevice, 0));
  PcoGfxEncodeTask task{d_in, n, nullptr, 0, dtype, 0};
  validate_task(task, cfg, false);
  std::vector<EncModePlan> plans(1);
  std::vector<PcoGfxEncodeTask> vt; ResolvedConfig ecfg = cfg; DictTask* d_dict = nullptr;
  if (cfg.mode_kind == PCO_MODE_TRY_DICT) { d_dict = build_dicts(1, &task, true, 0, vt, ecfg); task = vt[0]; }
  resolve_plans(1, &task, ecfg, plans, 0);
  ecfg.d_dict = d_dict;
  plans[0].n_pages = (uint32_t)pn.size(); plans[0].page_low = (uint32_t)(n / pn.size()); plans[0].page_r = (uint32_t)(n % pn.size()); plans[0].page_first = 1;
  plans[0].exact_paging = exact_pages ? 1u : 0u;
  const size_t meta_cap = chunk_meta_cap(cfg, bits, n);
  std::vector<size_t> offs(pn.size() + 1); size_t total = meta_cap;
  for (size_t i = 0; i < pn.size(); i++) { offs[i] = total; total += chunk_page_cap(cfg, bits, pn[i]); }
  offs[pn.size()] = total;
  uint8_t* d_out = (uint8_t*)wsp.io_out.ensure(total);
  std::vector<EncPage> pages(pn.size() + 1);
  { EncPage p{}; p.chunk = 0; p.n = 0; p.dst = d_out; p.dst_cap = meta_cap; p.flags = kPageFlagMetaOnly; pages[0] = p; }
  size_t start = 0;
  for (size_t i = 0; i < pn.size(); i++) {
    EncPage p{}; p.chunk = 0; p.page_idx = (uint32_t)i; p.start = start; p.n = pn[i]; p.dst = d_out + offs[i]; p.dst_cap = offs[i + 1] - offs[i]; p.flags = 0;
    pages[i + 1] = p; start += pn[i];
  }
  std::vector<PcoGfxTaskResult> res(pages.size());
  EncWorkspace ws{};
  run_encode(1, &task, plans, pages, ecfg, res.data(), nullptr, 0, &ws);
  for (auto& r : res) if (r.status != PCO_GFX_OK) throw HostError{(int)r.status, "chunk failed to compress"};
  std::unique_ptr<PcoGfxChunkCompressor> cc(new PcoGfxChunkCompressor());
  cc->meta.resize(res[0].n_out);
  PCO_HIP_CHECK(hipMemcpy(cc->meta.data(), d_out, res[0].n_out, hipMemcpyDeviceToHost));
  cc->page_n = pn;
  for (size_t i = 0; i < pn.size(); i++) {
    cc->pages.emplace_back(res[i + 1].n_out);
    PCO_HIP_CHECK(hipMemcpy(cc->pages.back().data(), d_out + offs[i], res[i + 1].n_out, hipMemcpyDeviceToHost));
  }
  // size hints (metadata/chunk.rs:105-125, metadata/bins.rs:23-32, wrapped/chunk_compressor.rs:556-621): host arithmetic on the trained plan
  EncChunk ch; PCO_HIP_CHECK(hipMemcpy(&ch, ws.chunks, sizeof(EncChunk), hipMemcpyDeviceToHost));
  // the three plan regions of the chunk (PlanRef layout): only the optimized bins' weights and offset bits are needed here
  const size_t pbytes = plan_bytes_for(ws.plan_cap);
  std::vector<uint8_t> pv_raw(3 * pbytes);
  PCO_HIP_CHECK(hipMemcpy(pv_raw.data(), ws.plans, 3 * pbytes, hipMemcpyDeviceToHost));
  struct HostPlan { const uint32_t* bweight; const uint8_t* bob; } pv[3];
  for (int v = 0; v < 3; v++) { const uint8_t* b = pv_raw.data() + v * pbytes; pv[v].bweight = (const uint32_t*)(b + 28ull * ws.plan_cap); pv[v].bob = b + 40ull * ws.plan_cap + (2ull << kMaxEncTableLog); }
  const bool fb = ch.fallback != 0;
  size_t meta_bits = kBitsModeVariant + (4 + 5 + 5 + 64 + 32 * 32);
  if (!fb) meta_bits += (ch.mode_kind == kIntMult || ch.mode_kind == kFloatMult) ? (size_t)bits : (ch.mode_kind == kFloatQuant ? kBitsQuantK : 0);
  if (!fb && ch.dict_dtype) meta_bits += kBitsDictLen + 7 + (size_t)ch.dict_k * bits;   // Mode::Dict (metadata/mode.rs:219-229)
  size_t page_meta_bits = 0; double avg[3] = {0, 0, 0}; uint32_t nlps[3] = {0, 0, 0};
  for (int v = 0; v < 3; v++) {
    const bool present = fb ? v == 1 : ch.v[v].present != 0;
    if (!present) continue;
    const uint32_t lb = fb ? (uint32_t)bits : ch.v[v].latent_bits, asl = fb ? 0 : ch.v[v].ans_size_log, nb = fb ? 1 : ch.v[v].n_bins;
    meta_bits += kBitsAnsSizeLog + kBitsNBins + (size_t)nb * (asl + lb + offset_bits_bits(lb));
    if (!fb && v == 1) nlps[v] = (ch.delta_kind == kDeltaConsecutive || ch.delta_kind == kDeltaConv1) ? ch.delta_order : (ch.delta_kind == kDeltaLookback ? (1u << ch.state_n_log) : 0u);
    page_meta_bits += (size_t)asl * 4 + (size_t)lb * nlps[v];
    if (fb) avg[v] = (double)bits;
    else {
      const double tw = (double)(1ull << asl);
      for (uint32_t b = 0; b < nb; b++) {
        const double w = (double)pv[v].bweight[b];
        avg[v] += ((double)asl - std::log2(w) + (double)pv[v].bob[b]) * w / tw;
      }
    }
  }
  cc->meta_size_hint = (meta_bits + 7) / 8;
  for (size_t i = 0; i < pn.size(); i++) {
    size_t body_bits = 0;
    for (int v = 0; v < 3; v++) {
      const bool present = fb ? v == 1 : ch.v[v].present != 0;
      if (!present) continue;
      const size_t stored = v == 2 ? pn[i] : (pn[i] > nlps[1] ? pn[i] - nlps[1] : 0);
      body_bits += (size_t)std::ceil((double)stored * avg[v] * 1.2);
    }
    cc->page_size_hints.push_back((page_meta_bits + 7) / 8 + (body_bits + 7) / 8);
  }
  return cc.release();
}

}  // namespace pcogfx

extern "C" {

enum PcoError pco_chunk_compressor_new(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config, PcoGfxChunkCompressor** out) {
  clear_error();
  if (!dtype_bits(dtype)) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try { *out = chunk_compressor_build(nums, n, dtype, resolve_config(config)); return PcoSuccess; }
  catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}
enum PcoError pco_chunk_compressor_new_exact(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config, const size_t* page_sizes,
                                             size_t n_pages, PcoGfxChunkCompressor** out) {
  clear_error();
  if (!dtype_bits(dtype)) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    if (!page_sizes) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page_sizes is null"};
    static const size_t none = 0;
    *out = chunk_compressor_build(nums, n, dtype, resolve_config(config), n_pages ? page_sizes : &none, n_pages); return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}
size_t pco_chunk_compressor_meta_size(const PcoGfxChunkCompressor* cc) { return cc->meta.size(); }
size_t pco_chunk_compressor_page_size(const PcoGfxChunkCompressor* cc, size_t i) { return i < cc->pages.size() ? cc->pages[i].size() : 0; }
size_t pco_chunk_compressor_n_pages(const PcoGfxChunkCompressor* cc) { return cc->pages.size(); }
size_t pco_chunk_compressor_page_n(const PcoGfxChunkCompressor* cc, size_t i) { return i < cc->page_n.size() ? cc->page_n[i] : 0; }
size_t pco_chunk_compressor_meta_size_hint(const PcoGfxChunkCompressor* cc) { return cc->meta_size_hint; }
size_t pco_chunk_compressor_page_size_hint(const PcoGfxChunkCompressor* cc, size_t i) { return i < cc->page_size_hints.size() ? cc->page_size_hints[i] : 0; }
enum PcoError pco_chunk_compressor_write_meta(const PcoGfxChunkCompressor* cc, void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  if (cc->meta.size() > dst_cap) { set_error(PCO_GFX_INVALID_ARGUMENT, "destination too small"); return PcoCompressionError; }
  std::memcpy(dst, cc->meta.data(), cc->meta.size()); if (n_written) *n_written = cc->meta.size();
  return PcoSuccess;
}
enum PcoError pco_chunk_compressor_write_page(const PcoGfxChunkCompressor* cc, size_t page_idx, void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  if (page_idx >= cc->pages.size()) { set_error(PCO_GFX_INVALID_ARGUMENT, "page idx exceeds num pages"); return PcoCompressionError; }
  const auto& p = cc->pages[page_idx];
  if (p.size() > dst_cap) { set_error(PCO_GFX_INVALID_ARGUMENT, "destination too small"); return PcoCompressionError; }
  std::memcpy(dst, p.data(), p.size()); if (n_written) *n_written = p.size();
  return PcoSuccess;
}
void pco_chunk_compressor_free(PcoGfxChunkCompressor* cc) { delete cc; }

enum PcoError pco_chunk_decompressor_new(const void* src, size_t len, unsigned char dtype, uint8_t format_major,
                                         PcoGfxChunkDecompressor** out, size_t* consumed) {
  clear_error();
  const int bits = dtype_bits(dtype);
  if (!bits) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    require_device();
    Workspace& wsp = workspace();
    WorkspaceUse use(wsp, 0);
    uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(len + 64);
    PCO_HIP_CHECK(hipMemsetAsync(d_in + len, 0, 64, 0));
    if (len) PCO_HIP_CHECK(hipMemcpyAsync(d_in, src, len, hipMemcpyHostToDevice, 0));
    PcoGfxDecodeTask task{d_in, len, nullptr, 0, dtype, PCO_GFX_TASK_META_ONLY | ((uint32_t)format_major << 8)};
    PcoGfxTaskResult res{};
    launch_decode(1, &task, &res, nullptr, 0);
    if (res.status != PCO_GFX_OK) { set_error((int)res.status, "invalid chunk metadata"); return PcoDecompressionError; }
    auto* cd = new PcoGfxChunkDecompressor();
    cd->meta.assign((const uint8_t*)src, (const uint8_t*)src + res.consumed); cd->dtype = dtype; cd->format_major = format_major;
    *out = cd; if (consumed) *consumed = res.consumed;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}
static enum PcoError read_page_impl(PcoGfxChunkDecompressor* cd, const void* src, size_t len, size_t page_n, void* dst,
                                    size_t dst_cap, size_t* n_processed, size_t* consumed, int* partial_ok) {
  clear_error();
  try {
    if (dst_cap < page_n) throw HostError{PCO_GFX_INVALID_ARGUMENT, "dst must hold the whole page"};
    require_device();
    Workspace& wsp = workspace();
    WorkspaceUse use(wsp, 0);
    const int bits = dtype_bits(cd->dtype);
    const size_t ml = cd->meta.size();
    uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(ml + len + 64);
    uint8_t* d_out = (uint8_t*)wsp.io_out.ensure(page_n * (size_t)(bits / 8) + 64);
    PCO_HIP_CHECK(hipMemsetAsync(d_in + ml + len, 0, 64, 0));
    PCO_HIP_CHECK(hipMemcpyAsync(d_in, cd->meta.data(), ml, hipMemcpyHostToDevice, 0));
    if (len) PCO_HIP_CHECK(hipMemcpyAsync(d_in + ml, src, len, hipMemcpyHostToDevice, 0));
    PcoGfxDecodeTask task{d_in, ml + len, d_out, page_n, cd->dtype, PCO_GFX_TASK_WRAPPED_PAGE | ((uint32_t)cd->format_major << 8)};
    PcoGfxTaskResult res{};
    launch_decode(1, &task, &res, nullptr, 0);
    if (res.status != PCO_GFX_OK) {
      // (internal use by pco_page_decompressor_new, which passes partial_ok: the batches in front of the failing one are copied out anyway)
      if (partial_ok && (res.aux & 1u)) {
        if (res.n_out) PCO_HIP_CHECK(hipMemcpy(dst, d_out, res.n_out * (size_t)(bits / 8), hipMemcpyDeviceToHost));
        *partial_ok = 1; if (n_processed) *n_processed = res.n_out;
      }
      set_error((int)res.status, "page failed to decompress"); return PcoDecompressionError;
    }
    PCO_HIP_CHECK(hipMemcpy(dst, d_out, page_n * (size_t)(bits / 8), hipMemcpyDeviceToHost));
    if (n_processed) *n_processed = res.n_out;
    if (consumed) *consumed = res.consumed - ml;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}
enum PcoError pco_chunk_decompressor_read_page(PcoGfxChunkDecompressor* cd, const void* src, size_t len, size_t page_n, void* dst,
                                               size_t dst_cap, size_t* n_processed, size_t* consumed) {
  return read_page_impl(cd, src, len, page_n, dst, dst_cap, n_processed, consumed, nullptr);
}
void pco_chunk_decompressor_free(PcoGfxChunkDecompressor* cd) { delete cd; }

// PageDecompressor (wrapped/page_decompressor.rs:115-246): the page is decoded on the device when the handle is created (a page is
// one serial tANS stream; partial decodes would re-walk it) and `read` hands the numbers out at the reference's granularity -- with the
// reference's error timing: a page whose metadata is bad fails here, a page that goes wrong in batch k hands out the batches before k
// and fails on the call that reaches k (the last batch for the end-of-page checks).  (What differs: the footprint -- a page, not a batch.)
enum PcoError pco_page_decompressor_new(PcoGfxChunkDecompressor* cd, const void* src, size_t len, size_t page_n, PcoGfxPageDecompressor** out) {
  clear_error();
  try {
    const int bits = dtype_bits(cd->dtype);
    std::unique_ptr<PcoGfxPageDecompressor> pd(new PcoGfxPageDecompressor());
    pd->elem = (size_t)bits / 8; pd->n = page_n; pd->pos = 0;
    pd->nums.resize(std::max<size_t>(page_n, 1) * pd->elem);
    size_t n_done = 0, used = 0; int partial = 0;
    const PcoError code = read_page_impl(cd, src, len, page_n, pd->nums.data(), std::max<size_t>(page_n, 1), &n_done, &used, &partial);
    if (code != PcoSuccess && !partial) return code;
    pd->n_ok = code == PcoSuccess ? page_n : n_done;
    pd->bad_status = code == PcoSuccess ? 0 : pco_gfx_last_status();
    if (code != PcoSuccess) clear_error();
    pd->consumed = used;
    *out = pd.release();
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}
enum PcoError pco_page_decompressor_read(PcoGfxPageDecompressor* pd, void* dst, size_t dst_len, size_t* n_processed, int* finished) {
  clear_error();
  const size_t remaining = pd->n - pd->pos;
  if (dst_len % kBatchN != 0 && dst_len < remaining) {   // page_decompressor.rs:199-206
    set_error(PCO_GFX_INVALID_ARGUMENT, "num_dst's length must either be a multiple of 256 or be at least the count of numbers remaining (" +
                                            std::to_string(dst_len) + " < " + std::to_string(remaining) + ")");
    return PcoDecompressionError;
  }
  const size_t k = std::min(dst_len, remaining);
  if (pd->pos + k > pd->n_ok) {   // the call reaches the batch the page failed in: what came before it is written, the call fails
    const size_t good = pd->n_ok > pd->pos ? pd->n_ok - pd->pos : 0;
    if (good) std::memcpy(dst, pd->nums.data() + pd->pos * pd->elem, good * pd->elem);
    pd->pos = pd->n_ok;
    if (n_processed) *n_processed = 0;
    set_error(pd->bad_status, "page failed to decompress");
    return PcoDecompressionError;
  }
  if (k) std::memcpy(dst, pd->nums.data() + pd->pos * pd->elem, k * pd->elem);
  pd->pos += k;
  if (n_processed) *n_processed = k;
  if (finished) *finished = pd->pos == pd->n ? 1 : 0;
  return PcoSuccess;
}
size_t pco_page_decompressor_consumed(const PcoGfxPageDecompressor* pd) { return pd->consumed; }   /* into_src: bytes of the page */

// ChunkMeta accessors: a host-side read of the metadata bytes (metadata/chunk.rs:127-174, mode.rs:138-195, delta_encoding.rs:120-200,
// chunk_latent_var.rs:30-71).  O(bytes of metadata); nothing touches the device.
enum PcoError pco_gfx_chunk_meta_info(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, PcoGfxChunkMetaInfo* out) {
  clear_error();
  const int LB = dtype_bits(dtype);
  if (!LB || !out || (!meta && len)) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_info: bad argument"); return PcoInvalidType; }
  std::memset(out, 0, sizeof(*out));
  const uint8_t* p = (const uint8_t*)meta;
  uint64_t bit = 0; bool short_read = false;
  auto rd = [&](uint32_t n) -> uint64_t {   // little-endian bit stream (bit_reader.rs)
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; i++, bit++) { const uint64_t byte = bit >> 3; if (byte >= len) { short_read = true; continue; } v |= (uint64_t)((p[byte] >> (bit & 7)) & 1u) << i; }
    return v;
  };
  auto fail = [&](int st, const char* msg) { set_error(st, msg); return PcoDecompressionError; };
  out->mode_kind = (uint32_t)rd(kBitsModeVariant);
  if (out->mode_kind == kIntMult || out->mode_kind == kFloatMult) out->mode_base_latent = rd((uint32_t)LB);
  else if (out->mode_kind == kFloatQuant) out->mode_k = (uint32_t)rd(kBitsQuantK);
  else if (out->mode_kind == kDict) { if (short_read) return fail(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoSuccess; }   // (the dictionary follows: kinds only)
  else if (out->mode_kind != kClassic) return fail(short_read ? PCO_GFX_INSUFFICIENT_DATA : PCO_GFX_CORRUPTION, "unknown mode");
  if (format_major < 3) { out->delta_order = (uint32_t)rd(kBitsDeltaOrder); out->delta_kind = out->delta_order ? kDeltaConsecutive : kDeltaNone; }
  else {
    out->delta_kind = (uint32_t)rd(kBitsDeltaVariant);
    // (the reference's own validation, metadata/delta_encoding.rs:143-176: a zero order, a window beyond the maximum and a state beyond the window are Corruption)
    if (out->delta_kind == kDeltaConsecutive) {
      out->delta_order = (uint32_t)rd(kBitsDeltaOrder);
      if (!short_read && out->delta_order == 0) return fail(PCO_GFX_CORRUPTION, "Consecutive delta encoding order must not be 0");
      out->secondary_uses_delta = (uint32_t)rd(1);
    } else if (out->delta_kind == kDeltaLookback) {
      out->window_n_log = 1 + (uint32_t)rd(kBitsLookbackWindowLog); out->state_n_log = (uint32_t)rd(kBitsLookbackStateLog);
      if (!short_read && out->window_n_log > kMaxLookbackWindowLog) return fail(PCO_GFX_CORRUPTION, "lookback delta encoding window size log exceeds the maximum");
      if (!short_read && out->state_n_log > out->window_n_log) return fail(PCO_GFX_CORRUPTION, "lookback delta encoding state size log exceeds the window size log");
      out->secondary_uses_delta = (uint32_t)rd(1);
    }
    else if (out->delta_kind == kDeltaConv1) { if (short_read) return fail(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoSuccess; }   // (weights follow: kinds only)
    else if (out->delta_kind != kDeltaNone) return fail(short_read ? PCO_GFX_INSUFFICIENT_DATA : PCO_GFX_CORRUPTION, "unknown delta encoding");
  }
  out->present[0] = out->delta_kind == kDeltaLookback; out->present[1] = 1;
  out->present[2] = out->mode_kind == kIntMult || out->mode_kind == kFloatMult || out->mode_kind == kFloatQuant;
  for (int v = 0; v < 3; v++) {
    if (out->present[v]) {
      const uint32_t lb = v == 0 ? 32u : (uint32_t)LB;
      out->ans_size_log[v] = (uint32_t)rd(kBitsAnsSizeLog); out->n_bins[v] = (uint32_t)rd(kBitsNBins);
      bit += (uint64_t)out->n_bins[v] * (out->ans_size_log[v] + lb + offset_bits_bits((int)lb));
    }
    if (short_read || (bit + 7) / 8 > len) return fail(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short");
    out->n_vars_parsed = (uint32_t)v + 1;
  }
  out->meta_bytes = (bit + 7) / 8;
  return PcoSuccess;
}
enum PcoError pco_gfx_chunk_meta_conv1(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, uint32_t* quantization,
                                       int64_t* bias, int32_t* weights, uint32_t* order) {
  clear_error();
  const int LB = dtype_bits(dtype);
  if (!LB || !quantization || !bias || !weights || !order || (!meta && len)) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_conv1: bad argument"); return PcoInvalidType; }
  *order = 0; *quantization = 0; *bias = 0;
  const uint8_t* p = (const uint8_t*)meta;
  uint64_t bit = 0; bool short_read = false;
  auto rd = [&](uint32_t n) -> uint64_t {   // little-endian bit stream (bit_reader.rs)
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; i++, bit++) { const uint64_t byte = bit >> 3; if (byte >= len) { short_read = true; continue; } v |= (uint64_t)((p[byte] >> (bit & 7)) & 1u) << i; }
    return v;
  };
  const uint32_t mode_kind = (uint32_t)rd(kBitsModeVariant);
  if (mode_kind == kIntMult || mode_kind == kFloatMult) rd((uint32_t)LB);
  else if (mode_kind == kFloatQuant) rd(kBitsQuantK);
  else if (mode_kind != kClassic) { set_error(PCO_GFX_UNSUPPORTED, "chunk_meta_conv1: Dict or unknown mode"); return PcoDecompressionError; }
  if (format_major >= 3 && rd(kBitsDeltaVariant) == kDeltaConv1) {
    const uint32_t q = (uint32_t)rd(5);
    const uint64_t b = rd(64) ^ (1ull << 63);
    const uint32_t ord = (uint32_t)rd(5) + 1;
    for (uint32_t k = 0; k < ord; k++) weights[k] = (int32_t)((uint32_t)rd(32) ^ 0x80000000u);
    if (short_read) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
    *quantization = q; *bias = (int64_t)b; *order = ord;
  }
  if (short_read) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  return PcoSuccess;
}
enum PcoError pco_gfx_chunk_meta_dict(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, uint32_t* n_unique, void* values,
                                      size_t cap) {
  clear_error();
  const int LB = dtype_bits(dtype);
  if (!LB || !n_unique || (!meta && len) || (!values && cap)) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_dict: bad argument"); return PcoInvalidType; }
  (void)format_major;   // (the mode section is the same in every format version)
  *n_unique = 0;
  const uint8_t* p = (const uint8_t*)meta;
  if (len == 0) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  if ((p[0] & 0xfu) != kDict) return PcoSuccess;
  // 4-bit variant, 25-bit length, zeros to the byte, then the dictionary as whole little-endian latents
  if (len < 4) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  const uint32_t hdr = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  const uint32_t k = (hdr >> 4) & ((1u << kBitsDictLen) - 1);
  const size_t vb = (size_t)LB / 8;
  *n_unique = k;
  if ((size_t)k * vb > len - 4) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  if (k > cap) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_dict: values holds fewer than n_unique entries"); return PcoInvalidType; }
  std::memcpy(values, p + 4, (size_t)k * vb);
  return PcoSuccess;
}
enum PcoError pco_chunk_compressor_meta_info(const PcoGfxChunkCompressor* cc, unsigned char dtype, PcoGfxChunkMetaInfo* out) {
  if (!cc) { clear_error(); set_error(PCO_GFX_INVALID_ARGUMENT, "null handle"); return PcoCompressionError; }
  return pco_gfx_chunk_meta_info(cc->meta.data(), cc->meta.size(), dtype, 4, out);
}
enum PcoError pco_chunk_decompressor_meta_info(const PcoGfxChunkDecompressor* cd, PcoGfxChunkMetaInfo* out) {
  if (!cd) { clear_error(); set_error(PCO_GFX_INVALID_ARGUMENT, "null handle"); return PcoDecompressionError; }
  return pco_gfx_chunk_meta_info(cd->meta.data(), cd->meta.size(), cd->dtype, cd->format_major, out);
}
void pco_page_decompressor_free(PcoGfxPageDecompressor* pd) { delete pd; }

}  // extern "C"
