// pco_encode_passes.inc -- what the encode entry points call (included by pco_gfx.hip): the Dict build, the standalone and wrapped launchers,
// the wrapped paging plan, the passes of a call beyond the workspace budget, the host-buffer compressor.
namespace pcogfx {

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
  PCO_RESERVE_LDS(enc_dict_lds_kernel, kDictLdsBytes, "enc_dict_lds_kernel");
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

// A specs call (section 3c) brings its plans ready: nothing is resolved, and the Auto debug records of the call read all-zero
static void take_ready_plans(size_t n_tasks, const EncModePlan* ready, std::vector<EncModePlan>& plans) {
  plans.assign(ready, ready + n_tasks);
  workspace().auto_dbg.assign(std::min<size_t>(n_tasks, PCO_GFX_AUTO_DEBUG_MAX), PcoGfxAutoModeRecord{});
  workspace().auto_delta_dbg.assign(std::min<size_t>(n_tasks, PCO_GFX_AUTO_DEBUG_MAX), PcoGfxAutoDeltaRecord{});
}

// batched standalone chunks: one page per chunk, preamble + meta + page into task.dst.  `ready`: the chunks' plans from a spec array instead of
// from resolve_plans (mode and delta only: the paging fields are set here either way)
static void launch_encode(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, PcoGfxTaskResult* results,
                          PcoGfxTaskResult* d_results_user, hipStream_t stream, const EncModePlan* ready = nullptr) {
  if (n_tasks == 0) return;
  std::vector<EncModePlan> plans(n_tasks);
  std::vector<EncPage> pages(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) validate_task(tasks[i], cfg, true);
  if (cfg.verify) {   // what the verify behind the encode would refuse is refused before anything is launched
    uint64_t max_bytes = 0;
    for (size_t i = 0; i < n_tasks; i++) {
      const int bits = dtype_bits(tasks[i].dtype);
      // (the decode reads up to 16 bytes past a chunk; the encoders fill dst to within 8 of dst_cap: the documented dst_cap leaves the 16)
      if (tasks[i].dst_cap < guarantee_standalone_chunk_size(bits, tasks[i].n) + 16) throw HostError{PCO_GFX_INVALID_ARGUMENT, "encode task " + std::to_string(i) + ": a verified encode needs dst_cap >= pco_gfx_guarantee_chunk_size(n) + 16"};
      max_bytes = std::max<uint64_t>(max_bytes, tasks[i].n * (uint64_t)(bits / 8));
    }
    check_verify_grid(max_bytes, n_tasks);
  }
  const PcoGfxEncodeTask* const caller_tasks = tasks;   // (a Dict call encodes index chunks; a verify compares the caller's numbers)
  std::vector<PcoGfxEncodeTask> vt; ResolvedConfig ecfg = cfg; DictTask* d_dict = nullptr;
  if (cfg.mode_kind == PCO_MODE_TRY_DICT) { d_dict = build_dicts(n_tasks, tasks, results != nullptr, stream, vt, ecfg); tasks = vt.data(); }
  if (ready) take_ready_plans(n_tasks, ready, plans);
  else { TracePhase tp("resolve_plans (total)", stream); resolve_plans(n_tasks, tasks, ecfg, plans, stream); }
  ecfg.d_dict = d_dict;
  TracePhase tp_final("final encode", stream);
  for (size_t i = 0; i < n_tasks; i++) {
    plans[i].n_pages = 1; plans[i].page_low = (uint32_t)tasks[i].n; plans[i].page_r = 0; plans[i].page_first = (uint32_t)i;
    EncPage p{}; p.chunk = (uint32_t)i; p.page_idx = 0; p.start = 0; p.n = tasks[i].n; p.dst = tasks[i].dst; p.dst_cap = tasks[i].dst_cap; p.flags = kPageFlagPreamble;
    pages[i] = p;
  }
  run_encode(n_tasks, tasks, plans, pages, ecfg, results, d_results_user, stream);
  if (cfg.verify) {   // PCO_GFX_CFG_VERIFY: pco_gfx_verify_chunks' work behind the encode, over its results where they lie on the device, in place
    PcoGfxTaskResult* d_enc = d_results_user ? d_results_user : (PcoGfxTaskResult*)workspace().results.p;
    launch_verify(n_tasks, caller_tasks, d_enc, results, d_enc, stream);
  }
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
                                  PcoGfxPageInfo* d_infos, hipStream_t stream, const EncModePlan* ready = nullptr) {
  if (n_tasks == 0) return;
  wt += at;
  if (cfg.verify) check_verify_grid(pg.page_max * 8, pg.first[at + n_tasks] - pg.first[at]);   // (before anything is launched; a wrapped dst_cap always leaves the decode its 16 bytes)
  const bool sync = infos != nullptr;
  std::vector<EncModePlan> plans(n_tasks);
  std::vector<EncPage> pages;
  std::vector<PcoGfxEncodeTask> otasks(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) otasks[i] = PcoGfxEncodeTask{wt[i].src, wt[i].n, wt[i].dst, wt[i].dst_cap, wt[i].dtype, 0};
  const PcoGfxEncodeTask* tasks = otasks.data();
  std::vector<PcoGfxEncodeTask> vt; ResolvedConfig ecfg = cfg; DictTask* d_dict = nullptr;
  if (cfg.mode_kind == PCO_MODE_TRY_DICT) { d_dict = build_dicts(n_tasks, tasks, sync, stream, vt, ecfg); tasks = vt.data(); }
  if (ready) take_ready_plans(n_tasks, ready + at, plans);   // (`ready` is the whole call's, like `wt`)
  else resolve_plans(n_tasks, tasks, ecfg, plans, stream);
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
  // (a verify reads the piece directory on the device: a synchronous call without d_infos gets one in the workspace)
  if (cfg.verify && !d_infos) d_infos = (PcoGfxPageInfo*)workspace().verify_infos.ensure(pages.size() * sizeof(PcoGfxPageInfo));
  run_encode(n_tasks, tasks, plans, pages, ecfg, sync ? res.data() : nullptr, nullptr, stream, nullptr, 0, d_infos);
  if (sync) for (size_t k = 0; k < pages.size(); k++) infos[k] = PcoGfxPageInfo{offs[k], res[k].n_out, pages[k].n, res[k].status, res[k].aux};
  // PCO_GFX_CFG_VERIFY: pco_gfx_verify_wrapped_chunks' work behind the encode, over the directory in place
  if (cfg.verify) launch_verify_wrapped(n_tasks, wt, pg.sizes.data(), pg.first.data() + at, d_infos, infos, d_infos, stream);
}

// The encode workspace is ~8 bytes of scratch per byte of input in the worst case (full-width latents of up to three variables,
// two sort buffers, symbols, tANS fields): 130 GB for 16 GiB of numbers.  A synchronous call whose workspace would not fit the
// budget -- PCO_GFX_WORKSPACE_GB, default 80 % of the device memory that is free (plus what the workspace already holds) -- is
// run as consecutive sub-batches of chunks through the same buffers; a device allocation that fails anyway halves the sub-batch.
// (Asynchronous calls cannot be cut -- the caller owns the ordering -- and take what they need.)
// What the encode buffers of this thread's workspace hold.  (The budget counts the Dict pair; the remembered per-chunk footprint of
// encode_in_passes never has -- an oversight or intended, kept as it is until a test decides.)
static size_t encode_held_bytes(bool with_dict) {
  const Workspace& w = workspace();
  return w.enc_lat.cap + w.enc_lat2.cap + w.enc_sort.cap + w.enc_ans.cap + w.enc_sym.cap + w.enc_answ.cap + w.enc_state.cap + w.enc_small.cap + w.enc_bat.cap + w.enc_run.cap +
         w.enc_fstate.cap + w.enc_lb.cap + w.enc_lbprops.cap + w.enc_walk.cap + w.enc_vlut.cap + (with_dict ? w.enc_dict.cap + w.enc_dict_hbm.cap : 0);
}
static size_t workspace_budget_bytes() {
  static const char* env = std::getenv("PCO_GFX_WORKSPACE_GB");   // (read once per process)
  return scratch_budget_bytes(env, env && *env ? 0 : encode_held_bytes(true));
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
                          (cfg.verify ? verify_per_task_bytes(stride) : 0) +                  // (a verified encode: the decoded numbers and what the decode of a pass takes)
                          extra_per_task;
  // (buffers are allocated with an eighth of slack; passes are balanced: the walkers' latency is paid once per pass whatever its size,
  //  so 7800 + 392 chunks cost what 2 x 7800 would).  The estimate above is the worst case of the spec -- Auto may end up with two
  //  variables and a lookback slot, or with one and none -- so what a call of the same spec and chunk size really took is remembered
  //  (per thread) and used from then on; if other data needs more after all, the allocation failure below halves the pass.
  size_t est = per_task + per_task / 8;
  if (measure_only) return est * n_tasks;
  static thread_local std::unordered_map<uint64_t, size_t> seen_per_task;   // size_t(-1): an attempt on the remembered figure failed, the worst case stays
  static thread_local std::unordered_map<uint64_t, size_t> pass_cap;         // ... and the pass size that then went through: later calls of the spec start there, not at the wall
  const uint64_t spec_key = ((uint64_t)cfg.mode_kind | ((uint64_t)cfg.delta_kind << 4) | ((uint64_t)cfg.level << 8) | ((uint64_t)(cfg.strict_hist ? 1u : 0u) << 12) | ((uint64_t)(cfg.verify ? 1u : 0u) << 14) | ((uint64_t)stride << 16)) ^ key_salt;   // (strict histograms take the two sort buffers, a verify its scratch and the decode's buffers: footprints of their own; bit 13 is the wrapped surface's salt, bit 15 a specs call's)
  { auto f = seen_per_task.find(spec_key); if (f != seen_per_task.end() && f->second != ~(size_t)0) est = std::min(est, f->second + f->second / 8); }
  size_t batch = std::max<size_t>(64, std::min<size_t>(n_tasks, workspace_budget_bytes() / est));
  { auto f = pass_cap.find(spec_key); if (f != pass_cap.end()) batch = std::max<size_t>(64, std::min(batch, f->second)); }
  if (batch < n_tasks) { const size_t passes = (n_tasks + batch - 1) / batch; batch = std::max<size_t>(64, (n_tasks + passes - 1) / passes); }
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
  else if (largest_pass >= 64 && (!seen_per_task.count(spec_key) || seen_per_task[spec_key] != ~(size_t)0)) seen_per_task[spec_key] = (encode_held_bytes(false) + (cfg.verify ? verify_held_bytes() : 0)) / largest_pass + 1;
  return est * n_tasks;
}
// (`ready` and `fcfg`: a specs call's plans, and the config its footprint is planned and remembered under -- footprint_config, with a salt of its own)
static void encode_in_sub_batches(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, PcoGfxTaskResult* results,
                                  PcoGfxTaskResult* d_results, hipStream_t stream, const EncModePlan* ready = nullptr, const ResolvedConfig* fcfg = nullptr) {
  if (!results || n_tasks <= 64) { launch_encode(n_tasks, tasks, cfg, results, d_results, stream, ready); return; }
  uint64_t n_max = 0; for (size_t i = 0; i < n_tasks; i++) n_max = std::max<uint64_t>(n_max, tasks[i].n);
  encode_in_passes(n_tasks, n_max, fcfg ? *fcfg : cfg, 0, ready ? kSpecsKeySalt : 0, false, stream,
                   [&](size_t at, size_t k) { launch_encode(k, tasks + at, cfg, results + at, d_results ? d_results + at : nullptr, stream, ready ? ready + at : nullptr); });
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
                                     hipStream_t stream, const EncModePlan* ready = nullptr, const ResolvedConfig* fcfg = nullptr) {
  if (!infos || n_tasks <= 64) { launch_encode_wrapped(0, n_tasks, wt, pg, cfg, infos, d_infos, stream, ready); return; }
  uint64_t n_max = 0; for (size_t i = 0; i < n_tasks; i++) n_max = std::max<uint64_t>(n_max, wt[i].n);
  const size_t extra = wrapped_extra_per_task(n_tasks, pg);
  encode_in_passes(n_tasks, n_max, fcfg ? *fcfg : cfg, extra, (1ull << 13) | ((uint64_t)(extra >> 6) << 44) | (ready ? kSpecsKeySalt : 0), false, stream, [&](size_t at, size_t k) {
    const size_t piece0 = pg.first[at] + at;   // pieces before chunk `at`: its predecessors' pages and ChunkMetas
    launch_encode_wrapped(at, k, wt, pg, cfg, infos + piece0, d_infos ? d_infos + piece0 : nullptr, stream, ready);
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
