// pco_encode_auto.inc -- Auto specs (included by pco_gfx.hip): resolve_plans, i.e. ModeSpec::Auto and DeltaSpec::Auto resolved per chunk.
namespace pcogfx {

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

// The sample positions of a call's chunks by chunk length, pooled on the device: chunks of one length share one list.
struct SamplePool {
  std::unordered_map<uint64_t, std::pair<std::vector<uint32_t>, size_t>> by_n;   // n -> (positions, offset in the device pool)
  const uint8_t* d_pool = nullptr;
  size_t count(uint64_t n) const { return by_n.at(n).first.size(); }
  const uint32_t* d_idx(uint64_t n) const { return (const uint32_t*)(d_pool + by_n.at(n).second * 4); }
};
static void pool_sample_indices(SamplePool& sp, size_t n_tasks, const PcoGfxEncodeTask* tasks, std::vector<uint32_t> (*indices)(size_t), hipStream_t stream) {
  size_t pool = 0;
  for (size_t i = 0; i < n_tasks; i++) if (!sp.by_n.count(tasks[i].n)) { auto idx = indices(tasks[i].n); sp.by_n[tasks[i].n] = {idx, pool}; pool += idx.size(); }
  uint8_t* d = (uint8_t*)workspace().auto_idx.ensure(pool * 4 + 64);
  for (auto& kv : sp.by_n) if (!kv.second.first.empty()) PCO_HIP_CHECK(hipMemcpyAsync(d + kv.second.second * 4, kv.second.first.data(), kv.second.first.size() * 4, hipMemcpyHostToDevice, stream));
  sp.d_pool = d;
}

// ---------------- Auto mode ----------------
struct IntCand { uint64_t base; double per_adj; int slot; };            // slot: index of the chunk's stage-2 task, -1 = none
struct FloatCand { uint64_t base[2], inv[2]; int slot[2]; uint32_t bk; double best; int qslot; uint8_t host; };

// Auto mode on the device (auto_mode_kernels.hip) over the integer chunks `ints` and the float chunks `floats` of a call: what stage 1, the host's
// candidates, stage 2 and the bids hand to one another.
struct AutoModeTrial {
  const PcoGfxEncodeTask* tasks; hipStream_t stream; Workspace& wsp; const SamplePool& pool; const std::vector<size_t>& cnts;
  std::vector<size_t> ints, floats;
  size_t o_it = 0, o_ft = 0, o_ir = 0, o_fr = 0, o_st = 0, o_sr = 0;   // the device areas: stage-1 tasks, stage-1 results, stage-2 tasks and results
  uint8_t* d_all = nullptr; uint8_t* d_sbuf = nullptr;                    // ... and the float chunks' samples
  IntGcdResult* h_ir = nullptr; FloatStatsResult* h_fr = nullptr; const SavedResult* h_sr = nullptr;   // the results on the host
  std::vector<IntCand> icand; std::vector<FloatCand> fcand; std::vector<uint8_t> ihost;
};

// Stage 1: triple-GCD counts for integer chunks, the float statistics and the sample itself for float chunks.
static void auto_mode_stage1(AutoModeTrial& t) {
  const size_t ni = t.ints.size(), nf = t.floats.size(), ns_max = ni + 3 * nf;
  PCO_RESERVE_LDS(auto_float_stats_kernel, kAutoStage1LdsBytes, "the Auto mode kernels");
  PCO_RESERVE_LDS(auto_saved_kernel, kAutoSavedLdsBytes, "the Auto mode kernels");
  Layout at;
  t.o_it = at.place(ni * sizeof(IntGcdTask)); t.o_ft = at.place(nf * sizeof(FloatStatsTask)); t.o_ir = at.place(ni * sizeof(IntGcdResult)); t.o_fr = at.place(nf * sizeof(FloatStatsResult));
  t.o_st = at.place(ns_max * sizeof(SavedTask)); t.o_sr = at.place(ns_max * sizeof(SavedResult));
  const size_t dev_bytes = at.place(0);
  t.d_all = (uint8_t*)t.wsp.auto_tasks.ensure(dev_bytes);
  t.d_sbuf = (uint8_t*)t.wsp.auto_samp.ensure(std::max<size_t>(nf, 1) * kAutoCap * 8);
  const size_t res_bytes = t.o_st - t.o_ir;
  uint8_t* h_all = (uint8_t*)t.wsp.h_samp.ensure(std::max(t.o_ir, res_bytes) + 64);   // stage-1 task lists going up, then results coming down
  IntGcdTask* h_it = (IntGcdTask*)(h_all + t.o_it); FloatStatsTask* h_ft = (FloatStatsTask*)(h_all + t.o_ft);
  for (size_t k = 0; k < ni; k++) { const PcoGfxEncodeTask& e = t.tasks[t.ints[k]]; h_it[k] = IntGcdTask{e.src, t.pool.d_idx(e.n), (uint32_t)t.pool.count(e.n), e.dtype}; }
  for (size_t k = 0; k < nf; k++) { const PcoGfxEncodeTask& e = t.tasks[t.floats[k]]; h_ft[k] = FloatStatsTask{e.src, t.pool.d_idx(e.n), t.d_sbuf + k * (size_t)kAutoCap * 8, (uint32_t)t.pool.count(e.n), e.dtype}; }
  TracePhase tp_1("  mode: stage 1 (device statistics)", t.stream);
  PCO_HIP_CHECK(hipMemcpyAsync(t.d_all, h_all, t.o_ir, hipMemcpyHostToDevice, t.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(t.stream));   // (h_all is reused for the results)
  if (ni) hipLaunchKernelGGL(auto_int_gcd_kernel, dim3((uint32_t)ni), dim3(256), 0, t.stream, (const IntGcdTask*)(t.d_all + t.o_it), (IntGcdResult*)(t.d_all + t.o_ir));
  if (nf) hipLaunchKernelGGL(auto_float_stats_kernel, dim3((uint32_t)nf), dim3(kAutoT), kAutoStage1LdsBytes, t.stream, (const FloatStatsTask*)(t.d_all + t.o_ft), (FloatStatsResult*)(t.d_all + t.o_fr));
  PCO_HIP_CHECK(hipGetLastError());
  PCO_HIP_CHECK(hipMemcpyAsync(h_all, t.d_all + t.o_ir, res_bytes, hipMemcpyDeviceToHost, t.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(t.stream));
  t.h_ir = (IntGcdResult*)h_all; t.h_fr = (FloatStatsResult*)(h_all + (t.o_fr - t.o_ir));
}

// The host step between the stages: stage 1's statistics into candidate configurations (the host's libm: score_gcd, snap, the float-quant entropy).
static void auto_mode_candidates(AutoModeTrial& t) {
  const size_t ni = t.ints.size(), nf = t.floats.size();
  t.icand.assign(ni, IntCand{0, 0.0, -1}); t.fcand.resize(nf); t.ihost.assign(ni, 0);
  TracePhase tp_h("  mode: host candidates", t.stream);
  parallel_for_chunks(ni, [&](size_t k) {
    IntGcdResult& r = t.h_ir[k];
    if (r.overflow) { t.ihost[k] = 1; return; }
    uint64_t base; double score;
    if (autodetect::candidate_from_counts(r.e, r.n_entries, t.cnts[t.ints[k]] / 3, base, score)) { t.icand[k].base = base; t.icand[k].per_adj = score; t.icand[k].slot = 0; }
  });
  parallel_for_chunks(nf, [&](size_t k) {
    FloatCand& c = t.fcand[k]; c = FloatCand{}; c.slot[0] = c.slot[1] = c.qslot = -1;
    FloatStatsResult& r = t.h_fr[k];
    if (r.s_size < autodetect::kMinSample) return;
    if (r.overflow) { c.host = 1; return; }
    if (dtype_bits(t.tasks[t.floats[k]].dtype) == 64) autodetect::float_candidates<uint64_t>(r, c.base, c.inv, c.slot, c.bk, c.best, c.qslot);
    else autodetect::float_candidates<uint32_t>(r, c.base, c.inv, c.slot, c.bk, c.best, c.qslot);
  });
}

// Stage 2: what every candidate saves.
static void auto_mode_stage2(AutoModeTrial& t) {
  const size_t ni = t.ints.size(), nf = t.floats.size();
  std::vector<SavedTask> st; st.reserve(ni + 3 * nf);
  for (size_t k = 0; k < ni; k++) if (t.icand[k].slot == 0) {
    const PcoGfxEncodeTask& e = t.tasks[t.ints[k]];
    t.icand[k].slot = (int)st.size();
    st.push_back(SavedTask{e.src, t.pool.d_idx(e.n), 2u, e.dtype, (uint32_t)t.pool.count(e.n), 0u, 0, 0, t.icand[k].base, t.icand[k].per_adj});
  }
  for (size_t k = 0; k < nf; k++) {
    const uint32_t dtype = t.tasks[t.floats[k]].dtype; FloatCand& c = t.fcand[k]; const void* sb = t.d_sbuf + k * (size_t)kAutoCap * 8;
    for (int q = 0; q < 2; q++) if (c.slot[q] == 0) { c.slot[q] = (int)st.size(); st.push_back(SavedTask{sb, nullptr, 0u, dtype, t.h_fr[k].s_size, 0u, c.base[q], c.inv[q], 0, 0.0}); }
    if (c.qslot == 0) { c.qslot = (int)st.size(); st.push_back(SavedTask{sb, nullptr, 1u, dtype, t.h_fr[k].s_size, c.bk, 0, 0, 0, c.best}); }
  }
  if (st.empty()) return;
  TracePhase tp_2("  mode: stage 2 (bits saved per candidate)", t.stream);
  PCO_HIP_CHECK(hipMemcpyAsync(t.d_all + t.o_st, st.data(), st.size() * sizeof(SavedTask), hipMemcpyHostToDevice, t.stream));
  hipLaunchKernelGGL(auto_saved_kernel, dim3((uint32_t)st.size()), dim3(256), kAutoSavedLdsBytes, t.stream, (const SavedTask*)(t.d_all + t.o_st), (SavedResult*)(t.d_all + t.o_sr));
  PCO_HIP_CHECK(hipGetLastError());
  SavedResult* h = (SavedResult*)t.wsp.h_sum.ensure(st.size() * sizeof(SavedResult) + 64);
  PCO_HIP_CHECK(hipMemcpyAsync(h, t.d_all + t.o_sr, st.size() * sizeof(SavedResult), hipMemcpyDeviceToHost, t.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(t.stream));
  t.h_sr = h;
}

// The bids (data_types/unsigned.rs:28-37, float.rs:82-98; last maximum wins).  Chunks whose lists did not fit their slots go to `on_host`.
static void auto_mode_bids(const AutoModeTrial& t, std::vector<EncModePlan>& plans, std::vector<size_t>& on_host) {
  for (size_t k = 0; k < t.ints.size(); k++) {
    const size_t i = t.ints[k];
    if (t.ihost[k]) { on_host.push_back(i); continue; }
    if (t.icand[k].slot < 0) continue;
    const double est = t.h_sr[t.icand[k].slot].s_dbl / (double)t.cnts[i];
    if (est > 0.5) { plans[i].mode_kind = kIntMult; plans[i].mode_base = t.icand[k].base; }
  }
  for (size_t k = 0; k < t.floats.size(); k++) {
    const size_t i = t.floats[k]; const FloatCand& c = t.fcand[k];
    if (c.host) { on_host.push_back(i); continue; }
    const double total = (double)t.h_fr[k].s_size;
    double best = 0.0; int win = 0; int which = -1;
    bool found = false; double saved = 0.0;
    for (int q = 0; q < 2; q++) if (c.slot[q] >= 0) {
      const double v = (double)t.h_sr[c.slot[q]].s_int / total;
      if (v >= 0.5 && (!found || !(v < saved))) { found = true; saved = v; which = q; }
    }
    if (found && !(saved < best)) { best = saved; win = 1; }
    if (c.qslot >= 0) { const double v = t.h_sr[c.qslot].s_dbl / total; if (v > 1.5 && !(v < best)) { best = v; win = 2; } }
    if (win == 1) {
      const int bits = dtype_bits(t.tasks[i].dtype);
      const uint64_t bb = c.base[which], m = 1ull << (bits - 1);
      const bool finite = bits == 64 ? ((bb >> 52) & 0x7ff) != 0x7ff : ((bb >> 23) & 0xff) != 0xff;
      if (!finite || (bb & (m - 1)) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "The chosen mode was invalid for the number type"};
      plans[i].mode_kind = kFloatMult; plans[i].mode_aux2 = bb; plans[i].mode_aux = c.inv[which];
      plans[i].mode_base = (bb & m) ? (~bb & (bits == 64 ? ~0ull : 0xffffffffull)) : (bb ^ m);
    } else if (win == 2) { plans[i].mode_kind = kFloatQuant; plans[i].mode_k = c.bk; }
  }
}

// the test hook's records (pco_gfx_debug_auto_mode): copies of what the trial holds anyway
static void auto_mode_records(const AutoModeTrial& t, std::vector<PcoGfxAutoModeRecord>& dbg) {
  for (size_t k = 0; k < t.ints.size(); k++) {
    const size_t i = t.ints[k]; if (i >= dbg.size()) continue;
    PcoGfxAutoModeRecord& d = dbg[i];
    d.route = t.ihost[k] ? 4u : 1u; d.n_entries = t.h_ir[k].n_entries; d.overflow = t.h_ir[k].overflow;
    if (!t.ihost[k] && t.icand[k].slot >= 0) { const SavedResult& sr = t.h_sr[t.icand[k].slot]; d.cand_mask = 8u; d.base[3] = t.icand[k].base; d.s_int[3] = sr.s_int; std::memcpy(&d.s_dbl[3], &sr.s_dbl, 8); }
  }
  for (size_t k = 0; k < t.floats.size(); k++) {
    const size_t i = t.floats[k]; if (i >= dbg.size()) continue;
    PcoGfxAutoModeRecord& d = dbg[i]; const FloatStatsResult& r = t.h_fr[k]; const FloatCand& c = t.fcand[k];
    d.route = c.host ? 4u : (r.s_size < autodetect::kMinSample ? 0u : 2u); d.n_entries = r.n_entries; d.overflow = r.overflow; d.s_size = r.s_size;
    if (d.route != 2u) continue;
    d.tz5 = r.tz5; d.n_ints = r.n_ints; d.n_gcd = r.n_gcd; d.has_euclid = r.has_euclid; d.k = r.k; d.base_c = r.base_c;
    for (int q = 0; q < 3; q++) d.sim[q] = r.sim[q];
    for (int q = 0; q < 3; q++) {
      const int slot = q < 2 ? c.slot[q] : c.qslot; if (slot < 0) continue;
      const SavedResult& sr = t.h_sr[slot];
      d.cand_mask |= 1u << q; d.s_int[q] = sr.s_int; std::memcpy(&d.s_dbl[q], &sr.s_dbl, 8);
      if (q < 2) { d.base[q] = c.base[q]; d.inv[q] = c.inv[q]; } else d.bk = c.bk;
    }
  }
}

// detect_mode_for at the chunk's number width (a launch_width step: the width dispatch, nothing is launched)
struct DetectModeStep {
  const uint8_t* sample; size_t cnt; uint32_t dtype; EncModePlan& plan;
  template <class L>
  void launch() const { const L* s = (const L*)sample; detect_mode_for<L>(std::vector<L>(s, s + cnt), dtype, plan); }
};

// The host path: the chunks' samples gathered on the device and read back, the reference's detection on them.
static void auto_mode_on_host(const std::vector<size_t>& on_host, size_t n_tasks, const PcoGfxEncodeTask* tasks, const SamplePool& pool, const std::vector<size_t>& cnts,
                              std::vector<EncModePlan>& plans, hipStream_t stream) {
  Workspace& wsp = workspace();
  size_t total_bytes = 0;
  std::vector<size_t> off(on_host.size());
  for (size_t k = 0; k < on_host.size(); k++) { const size_t i = on_host[k]; off[k] = total_bytes; total_bytes += ((cnts[i] * (size_t)(dtype_bits(tasks[i].dtype) / 8)) + 15) & ~(size_t)15; }
  uint8_t* d_samp = (uint8_t*)wsp.auto_samp.ensure(total_bytes + 64);
  std::vector<GatherTask> g; uint32_t max_idx = 0;
  for (size_t k = 0; k < on_host.size(); k++) {
    const PcoGfxEncodeTask& e = tasks[on_host[k]];
    g.push_back(GatherTask{e.src, d_samp + off[k], pool.d_idx(e.n), (uint32_t)pool.count(e.n), (uint32_t)(dtype_bits(e.dtype) / 8)});
    max_idx = std::max<uint32_t>(max_idx, (uint32_t)pool.count(e.n));
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
    launch_width(width_group(tasks[i].dtype), DetectModeStep{h_samp + off[k], cnts[i], tasks[i].dtype, plans[i]});
  }, 1);   // (a detection is some 0.5 ms of libm and hashing: one chunk per grab)
}

// ModeSpec::Auto for every chunk of the call.
// Stage 1 on the device (auto_mode_kernels.hip): triple-GCD counts for integer chunks, the float statistics and the sample itself for
// float chunks.  The host turns them into candidate configurations (its libm: score_gcd, snap, the float-quant entropy), stage 2
// measures what every candidate saves, the host picks the bid.  Samples beyond kAutoCap numbers (chunks above 2^18), f16 and GCD lists
// that do not fit their slots take the host path on the sample itself.
static void resolve_auto_mode(size_t n_tasks, const PcoGfxEncodeTask* tasks, std::vector<EncModePlan>& plans, std::vector<PcoGfxAutoModeRecord>& dbg, hipStream_t stream) {
  TracePhase tp_mode("auto mode (sample + detect)", stream);
  SamplePool pool;
  pool_sample_indices(pool, n_tasks, tasks, autodetect::mode_sample_indices, stream);
  std::vector<size_t> cnts(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) cnts[i] = pool.count(tasks[i].n);
  std::vector<size_t> on_host;
  AutoModeTrial t{tasks, stream, workspace(), pool, cnts};
  for (size_t i = 0; i < n_tasks; i++) {
    plans[i].mode_kind = kClassic; plans[i].mode_k = 0; plans[i].mode_base = plans[i].mode_aux = plans[i].mode_aux2 = 0;
    if (cnts[i] < autodetect::kMinSample) continue;
    const bool is_float = dtype_kind(tasks[i].dtype) == kFloat;
    if (cnts[i] > kAutoCap || (is_float && dtype_bits(tasks[i].dtype) < 32)) on_host.push_back(i);
    else if (is_float) t.floats.push_back(i); else t.ints.push_back(i);
  }
  static const bool host_only = std::getenv("PCO_GFX_AUTO_MODE_ON_HOST") != nullptr;   // A/B switch
  if (host_only) { on_host.insert(on_host.end(), t.ints.begin(), t.ints.end()); on_host.insert(on_host.end(), t.floats.begin(), t.floats.end()); t.ints.clear(); t.floats.clear(); }
  for (size_t i : on_host) if (i < dbg.size()) dbg[i].route = 3;
  if (t.ints.size() + t.floats.size() > 0) {
    auto_mode_stage1(t);
    auto_mode_candidates(t);
    auto_mode_stage2(t);
    auto_mode_bids(t, plans, on_host);
    auto_mode_records(t, dbg);
    std::sort(on_host.begin(), on_host.end());
  }
  if (!on_host.empty()) auto_mode_on_host(on_host, n_tasks, tasks, pool, cnts, plans, stream);
}

// ---------------- Auto delta ----------------
struct DeltaCand { uint32_t delta_kind, order; };

// what the steps of DeltaSpec::Auto share: the delta samples (sampling.rs:27-60) of the call's chunks on the device
struct AutoDeltaCall {
  size_t n_tasks; const PcoGfxEncodeTask* tasks; const ResolvedConfig& cfg; hipStream_t stream; Workspace& wsp;
  SamplePool pool; std::vector<size_t> off; uint8_t* d_samp = nullptr;   // chunk i's sample: pool.count(tasks[i].n) latents at d_samp + off[i]
};

// 1 + 2. the delta samples: primary latents at the sampled positions, split on the fly from the source numbers.  False: no chunk has a sample.
static bool auto_delta_sample(AutoDeltaCall& a, const std::vector<EncModePlan>& plans) {
  std::unique_ptr<TracePhase> tp_lists(g_trace ? new TracePhase("auto delta: sample lists", a.stream) : nullptr);
  pool_sample_indices(a.pool, a.n_tasks, a.tasks, autodetect::delta_sample_indices, a.stream);
  size_t total_bytes = 0;
  a.off.resize(a.n_tasks);
  for (size_t i = 0; i < a.n_tasks; i++) { a.off[i] = total_bytes; total_bytes += ((a.pool.count(a.tasks[i].n) * (size_t)(dtype_bits(a.tasks[i].dtype) / 8)) + 15) & ~(size_t)15; }
  a.d_samp = (uint8_t*)a.wsp.auto_samp.ensure(total_bytes + 64);
  std::vector<SplitGatherTask> g; uint32_t max_idx = 0;
  for (size_t i = 0; i < a.n_tasks; i++) {
    const PcoGfxEncodeTask& e = a.tasks[i]; const uint32_t cnt = (uint32_t)a.pool.count(e.n);
    if (!cnt) continue;
    g.push_back(SplitGatherTask{e.src, a.d_samp + a.off[i], a.pool.d_idx(e.n), cnt, e.dtype, plans[i].mode_kind, plans[i].mode_k, plans[i].mode_base, plans[i].mode_aux, plans[i].mode_aux2});
    max_idx = std::max<uint32_t>(max_idx, cnt);
  }
  if (g.empty()) return false;
  tp_lists.reset();
  TracePhase tp("auto delta: sample split", a.stream);
  SplitGatherTask* d_g = (SplitGatherTask*)a.wsp.auto_tasks.ensure(g.size() * sizeof(SplitGatherTask));
  PCO_HIP_CHECK(hipMemcpyAsync(d_g, g.data(), g.size() * sizeof(SplitGatherTask), hipMemcpyHostToDevice, a.stream));
  const uint32_t bpt = std::max<uint32_t>(1, (max_idx + 255) / 256);
  if ((uint64_t)bpt * g.size() >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "too many chunks in one call"};
  hipLaunchKernelGGL(split_gather_kernel, dim3(bpt * (uint32_t)g.size()), dim3(256), 0, a.stream, d_g, bpt);
  PCO_HIP_CHECK(hipGetLastError());
  return true;
}

// the unsigned number type of a type's width (a sample of primary latents is encoded as such)
static uint32_t unsigned_type_of(uint32_t dtype) {
  static const uint32_t by_group[4] = {PCO_TYPE_U64, PCO_TYPE_U32, PCO_TYPE_U16, PCO_TYPE_U8};
  return by_group[width_group(dtype)];
}

// 3. One wave of trial encodes: the samples of `chunks` under every candidate of `cands`, through the pipeline up to train.  Returns the size
// summaries on the host, trial j of chunk k at [j * chunks.size() + k].
static const TrialSummary* auto_delta_trials(const AutoDeltaCall& a, const std::vector<size_t>& chunks, const std::vector<DeltaCand>& cands) {
  const hipStream_t stream = a.stream;
  std::vector<PcoGfxEncodeTask> tt; std::vector<EncModePlan> tp; std::vector<EncPage> tpg;
  std::unique_ptr<TracePhase> tp_prep(g_trace ? new TracePhase("auto delta: trial task lists", stream) : nullptr);
  // (candidate-major: the trials of one kind are consecutive blocks of every kernel, so whatever a kind costs is spread over all XCDs --
  //  chunk-major with four kinds put each kind on two of the eight)
  for (const DeltaCand& c : cands) {
    for (size_t i : chunks) {
      const size_t sn = a.pool.count(a.tasks[i].n);
      EncModePlan p{}; p.mode_kind = kClassic; p.ubl_override = choose_unoptimized_bins_log(a.cfg.level, a.tasks[i].n);
      p.delta_kind = c.delta_kind;
      if (c.delta_kind == kDeltaLookback) { p.window_n_log = lookback_window_log(sn); p.state_n_log = 0; }
      else if (c.delta_kind == kDeltaConsecutive) p.delta_order = c.order;
      p.n_pages = 1; p.page_low = (uint32_t)sn; p.page_r = 0; p.page_first = (uint32_t)tt.size();
      EncPage pg{}; pg.chunk = (uint32_t)tt.size(); pg.n = sn; pg.flags = 0;
      tt.push_back(PcoGfxEncodeTask{a.d_samp + a.off[i], sn, nullptr, 0, unsigned_type_of(a.tasks[i].dtype), 0}); tp.push_back(p); tpg.push_back(pg);
    }
  }
  tp_prep.reset();
  EncWorkspace wst{};
  { TracePhase tpp("auto delta: trial encodes", stream); run_encode(tt.size(), tt.data(), tp, tpg, a.cfg, nullptr, nullptr, stream, &wst, 2); }
  TracePhase tp_sum("auto delta: summaries", stream);
  TrialSummary* d_sum = (TrialSummary*)a.wsp.auto_sum.ensure(tt.size() * sizeof(TrialSummary));
  // log2(w) for w = 0..4096 from the host's libm (the reference's f64::log2)
  static const std::vector<double> log2_tab = make_log2_table();
  double* d_log2 = (double*)a.wsp.auto_log2.ensure(log2_tab.size() * 8);
  PCO_HIP_CHECK(hipMemcpyAsync(d_log2, log2_tab.data(), log2_tab.size() * 8, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(enc_trial_summary_kernel, dim3(((uint32_t)tt.size() + 63) / 64), dim3(64), 0, stream, wst, d_sum, (uint32_t)tt.size(), (const double*)d_log2);
  TrialSummary* sums = (TrialSummary*)a.wsp.h_sum.ensure(tt.size() * sizeof(TrialSummary) + 64);
  PCO_HIP_CHECK(hipMemcpyAsync(sums, d_sum, tt.size() * sizeof(TrialSummary), hipMemcpyDeviceToHost, stream));
  PCO_HIP_CHECK(hipStreamSynchronize(stream));
  for (size_t k = 0; k < tt.size(); k++) if (sums[k].status != PCO_GFX_OK) throw HostError{(int)sums[k].status, "Auto delta trial failed"};
  return sums;
}

// choose_auto_delta_encoding's walk up the consecutive orders (wrapped/chunk_compressor.rs:310-360): it stops at the first order that is no
// improvement.  trials[j * stride]: the summary of orders[j].  Returns whether every order was an improvement (the next wave goes on).
static bool take_consecutive_orders(EncModePlan& plan, float& best_cost, const TrialSummary* trials, size_t stride, const uint32_t* orders, size_t n_orders, int bits) {
  for (size_t j = 0; j < n_orders; j++) {
    const float cost = (float)trial_size(trials[j * stride], bits, orders[j]);
    if (!(cost < best_cost)) return false;
    plan.delta_kind = kDeltaConsecutive; plan.delta_order = orders[j]; plan.window_n_log = 0; best_cost = cost;
  }
  return true;
}

// the test hook's records (pco_gfx_debug_auto_delta): the size estimates of one wave's trials for one chunk, from the summaries the replay reads
// anyway.  trials[j * stride]: the summary of candidate first + j (0 no delta, 1 lookback, 1 + k order k), `flags`: trial_size's third argument.
static void auto_delta_record_wave(PcoGfxAutoDeltaRecord& d, const TrialSummary* trials, size_t stride, uint32_t first, const uint32_t* flags, size_t n_cands, int bits) {
  for (size_t j = 0; j < n_cands; j++) { d.eval_mask |= 1u << (first + j); d.cost[first + j] = (float)trial_size(trials[j * stride], bits, flags[j]); }
}

// DeltaSpec::Auto for every chunk of the call (the modes are resolved): trial encodes of a sample, in waves, and the reference's sequential
// decision replayed on their size estimates.
static void resolve_auto_delta(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, std::vector<EncModePlan>& plans, std::vector<PcoGfxAutoDeltaRecord>& dbg, hipStream_t stream) {
  AutoDeltaCall a{n_tasks, tasks, cfg, stream, workspace()};
  if (!auto_delta_sample(a, plans)) { for (size_t i = 0; i < n_tasks; i++) { plans[i].delta_kind = kDeltaNone; } return; }
  std::vector<size_t> sampled;
  for (size_t i = 0; i < n_tasks; i++) {
    plans[i].delta_kind = kDeltaNone; plans[i].delta_order = 0; plans[i].window_n_log = 0; plans[i].state_n_log = 0;
    if (a.pool.count(tasks[i].n)) sampled.push_back(i);
  }
  // 4. replay choose_auto_delta_encoding (wrapped/chunk_compressor.rs:310-360) on the size estimates
  std::vector<float> best(n_tasks, 0.0f); std::vector<uint8_t> more(n_tasks, 0);
  {
    // First wave: no delta, lookback, consecutive orders 1 and 2 -- choose_auto_delta_encoding stops at the first order that is no
    // improvement, and most data stops at 1 or 2 (an order-3 trial for everybody was a fifth of the trial time, wasted on them).
    const std::vector<DeltaCand> wave_a = {{kDeltaNone, 0}, {kDeltaLookback, 0}, {kDeltaConsecutive, 1}, {kDeltaConsecutive, 2}};
    const uint32_t orders_a[2] = {1, 2};
    const TrialSummary* sums = auto_delta_trials(a, sampled, wave_a);
    TracePhase tp_dec("auto delta: decisions", stream);
    parallel_for_chunks(sampled.size(), [&](size_t k) {
      const size_t i = sampled[k], stride = sampled.size();   // (trial j of chunk k: candidate-major)
      const size_t sn = a.pool.count(tasks[i].n); const int bits = dtype_bits(tasks[i].dtype);
      float best_cost = (float)trial_size(sums[k], bits, 0);
      const float penalty = 0.25f * (float)sn;
      if (best_cost > penalty) {
        const float lb_cost = (float)trial_size(sums[stride + k], bits, 0x80000000u | 1u) + penalty;
        if (lb_cost < best_cost) { plans[i].delta_kind = kDeltaLookback; plans[i].window_n_log = lookback_window_log(tasks[i].n); plans[i].state_n_log = 0; best_cost = lb_cost; }
      }
      more[i] = take_consecutive_orders(plans[i], best_cost, sums + 2 * stride + k, stride, orders_a, 2, bits) ? 1 : 0;
      best[i] = best_cost;
      if (i < dbg.size()) { const uint32_t flags_a[4] = {0, 0x80000000u | 1u, 1, 2}; dbg[i].sample_n = (uint32_t)sn; auto_delta_record_wave(dbg[i], sums + k, stride, 0, flags_a, 4, bits); }
    });
  }
  // Further waves, two orders at a time, only for the chunks whose last trial was still an improvement (high-order differences of noisy
  // data are the expensive trials: wide value ranges)
  for (uint32_t first = 3; first <= 7; first += 2) {
    std::vector<size_t> deeper;
    for (size_t i : sampled) if (more[i]) deeper.push_back(i);
    if (deeper.empty()) break;
    std::vector<DeltaCand> wave; std::vector<uint32_t> orders;
    for (uint32_t o = first; o <= 7 && o < first + 2; o++) { wave.push_back(DeltaCand{kDeltaConsecutive, o}); orders.push_back(o); }
    const TrialSummary* sums = auto_delta_trials(a, deeper, wave);
    parallel_for_chunks(deeper.size(), [&](size_t k) {
      const size_t i = deeper[k];
      more[i] = take_consecutive_orders(plans[i], best[i], sums + k, deeper.size(), orders.data(), orders.size(), dtype_bits(tasks[i].dtype)) ? 1 : 0;
      if (i < dbg.size()) auto_delta_record_wave(dbg[i], sums + k, deeper.size(), 1 + first, orders.data(), orders.size(), dtype_bits(tasks[i].dtype));
    });
  }
  for (size_t i = 0; i < dbg.size(); i++) { dbg[i].delta_kind = plans[i].delta_kind; dbg[i].delta_order = plans[i].delta_order; dbg[i].window_n_log = plans[i].window_n_log; }
}

// The plans of a call's chunks: the explicit specs as given, Auto mode and Auto delta resolved per chunk.
static void resolve_plans(size_t n_tasks, const PcoGfxEncodeTask* tasks, const ResolvedConfig& cfg, std::vector<EncModePlan>& plans, hipStream_t stream) {
  for (size_t i = 0; i < n_tasks; i++) { plans[i] = EncModePlan{}; plans[i].ubl_override = 0xffffffffu; }
  std::vector<PcoGfxAutoModeRecord>& dbg = workspace().auto_dbg;   // (pco_gfx_debug_auto_mode: the first chunks of THIS call, all-zero = route "none")
  dbg.assign(cfg.mode_kind == PCO_MODE_AUTO ? std::min<size_t>(n_tasks, PCO_GFX_AUTO_DEBUG_MAX) : 0, PcoGfxAutoModeRecord{});
  std::vector<PcoGfxAutoDeltaRecord>& ddbg = workspace().auto_delta_dbg;   // (pco_gfx_debug_auto_delta: likewise, all-zero = no sample)
  ddbg.assign(cfg.delta_kind == PCO_DELTA_AUTO ? std::min<size_t>(n_tasks, PCO_GFX_AUTO_DEBUG_MAX) : 0, PcoGfxAutoDeltaRecord{});
  if (cfg.mode_kind != PCO_MODE_AUTO) { for (size_t i = 0; i < n_tasks; i++) plan_mode_explicit(plans[i], cfg, tasks[i].dtype); }
  else resolve_auto_mode(n_tasks, tasks, plans, dbg, stream);
  if (cfg.delta_kind != PCO_DELTA_AUTO) { for (size_t i = 0; i < n_tasks; i++) plan_delta_explicit(plans[i], cfg, tasks[i].n); }
  else resolve_auto_delta(n_tasks, tasks, cfg, plans, ddbg, stream);
}

}  // namespace pcogfx
