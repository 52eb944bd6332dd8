// pco_gfx.hip -- the C ABI of libpco_gfx.so (see include/pco_gfx.h) and the launch logic.
// One translation unit: the gfx950 kernels are included below.  There is NO CPU codec here: without a
// HIP device every compute entry point fails with PCO_GFX_DEVICE_ERROR.
#include "pco_host.h"
#include "pco_half.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <sched.h>
#include <pthread.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <unordered_map>

#include "pco_auto_host.inc"
#include "decode_kernel.hip"
#include "decode_trail.hip"   // (includes decode_fast.hip, which includes decode_kernel.hip)
#include "encode_kernels.hip"
#include "encode_lookback.hip"
#include "encode_conv1.hip"
#include "encode_dict.hip"
#include "encode_hist_select.hip"
#include "encode_hist_literal.hip"
#include "auto_mode_kernels.hip"
#include "encode_fast.hip"
#include "encode_walkseg.hip"
#include "encode_walkpack.hip"
#include "stream_kernels.hip"
#include "stream_wrapped.hip"
#include "dir_resolve.hip"
#include "verify.hip"
#include "pco_launch.h"

namespace pcogfx {

static thread_local HostError g_err{PCO_GFX_OK, ""};
void set_error(int status, const std::string& msg) { g_err.status = status; g_err.msg = msg; }
void clear_error() { g_err.status = PCO_GFX_OK; g_err.msg.clear(); }

struct WorkspaceHolder {
  std::unordered_map<int, std::unique_ptr<Workspace>> by_device;   // one workspace per (thread, device)
  // A worker thread that exits gives its device and pinned memory back.  The main thread's holder is destroyed during process
  // teardown, when the HIP runtime may already be unloading: there the driver reclaims everything and nothing is touched.
  ~WorkspaceHolder() {
    const bool worker = (long)syscall(SYS_gettid) != (long)getpid();
    for (auto& kv : by_device) {
      if (worker) { int cur = 0; const bool sw = hipGetDevice(&cur) == hipSuccess && cur != kv.first && hipSetDevice(kv.first) == hipSuccess; kv.second->release_all(); if (kv.second->last_event) (void)hipEventDestroy(kv.second->last_event); if (sw) (void)hipSetDevice(cur); }
      else (void)kv.second.release();   // (leaked on purpose, see above)
    }
  }
};
static thread_local WorkspaceHolder g_ws_holder;
Workspace& workspace() {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) throw HostError{PCO_GFX_DEVICE_ERROR, std::string("no HIP device: ") + hipGetErrorString(e)};
  std::unique_ptr<Workspace>& slot = g_ws_holder.by_device[dev];
  if (!slot) { slot.reset(new Workspace()); slot->device = dev; }
  return *slot;
}

static void require_device() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
}

// ---- guarantees (host arithmetic only) ----
static size_t baseline_meta_max_size(int latent_bits) {  // wrapped/guarantee.rs:11-33 + metadata/chunk.rs:105-113
  const size_t delta_max_bits = 4 + 5 + 5 + 64 + 32 * 32;  // DeltaEncoding::MAX_BIT_SIZE
  const size_t var_bits = kBitsAnsSizeLog + kBitsNBins + (0 + (size_t)latent_bits + offset_bits_bits(latent_bits));
  return (kBitsModeVariant + delta_max_bits + var_bits + 7) / 8;
}
size_t guarantee_wrapped_chunk_size(int latent_bits, size_t n) { return baseline_meta_max_size(latent_bits) + (n * (size_t)latent_bits + 7) / 8; }
size_t guarantee_standalone_chunk_size(int latent_bits, size_t n) { return 1 + 3 + guarantee_wrapped_chunk_size(latent_bits, n); }
size_t guarantee_standalone_header_size() { return 4 + 1 + (kBitsVarintPower + 64 + 8 + 7) / 8 + 2; }
bool n_per_page(uint64_t max_page_n, size_t n, std::vector<size_t>& out) {
  out.clear();
  if (max_page_n == 0) max_page_n = 1u << 18;
  if (n == 0) return true;
  size_t n_pages = (n + max_page_n - 1) / max_page_n;
  size_t low = n / n_pages, r = n % n_pages;
  out.assign(n_pages, low);
  for (size_t i = 0; i < r; i++) out[i] = low + 1;
  return true;
}

static PcoError fail_with(const HostError& e, PcoError code) { set_error(e.status, e.msg); return code; }

// ---- optional per-kernel timing with HIP events on the launch stream (used by bench.py's roofline) ----
struct KernelProfile {
  bool on = false;
  struct Rec { const char* name; hipEvent_t a, b; };
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;   // events are reused from one profiled region to the next: creating two per launch showed up in host time
  bool take(hipEvent_t& e) { if (!pool.empty()) { e = pool.back(); pool.pop_back(); return true; } return hipEventCreate(&e) == hipSuccess; }
  void give(hipEvent_t e) { pool.push_back(e); }
};
static thread_local KernelProfile g_prof;
// Every timed launch and span of both translation units starts here (pco_launch.h, TimedSpan): the span's first event is recorded, its last --
// returned, null when timing is off -- by the caller once the launch is made
hipEvent_t profile_span_begin(const char* name, hipStream_t stream) {
  if (!g_prof.on) return nullptr;
  hipEvent_t a, b;
  if (!g_prof.take(a)) return nullptr;
  if (!g_prof.take(b)) { g_prof.give(a); return nullptr; }
  (void)hipEventRecord(a, stream);
  g_prof.recs.push_back({name, a, b});
  return b;
}

// ---------------------------------------------------------------------------------------------------------
// decode launch: launch_decode, the host driver of the whole-chunk and whole-page decode entry points -- the fast path over each width group
// (walkers, expanders under the walk, expanders), the single-kernel decoder behind it, and, for a synchronous call, the pass with history
// scratch for the tasks that came back asking for it
// ---------------------------------------------------------------------------------------------------------
static uint32_t g_decode_lds_bytes = 16 * 1024;  // dynamic LDS per wave (fixed area + tANS tables)
// The expanders of the common chunks run on a second stream UNDER the walk (decode_trail.hip); PCO_GFX_DEC_TRAIL=0 keeps the two kernels
// back to back (A/B switch).
static bool g_decode_trail = env_not_zero("PCO_GFX_DEC_TRAIL");
// measurement / test switches: 's' = the expanders on the walker's own stream (after it, nothing overlaps), 'n' = no expanders at all, 'd' = the expanders
// BEFORE the walkers (they time out waiting): in the last two every chunk marked for the expanders is given back to dec_expand_kernel
static char g_trail_debug = env_char("PCO_GFX_TRAIL_DEBUG");
static bool g_trail_always = env_first_is("PCO_GFX_DEC_TRAIL", '2');   // PCO_GFX_DEC_TRAIL=2: the expanders for calls of any size (tests)

// the workspace's second stream and the two events that fork it off the caller's stream and join it again
static void ensure_side_stream(Workspace& ws) {
  if (!ws.side_stream) PCO_HIP_CHECK(hipStreamCreateWithFlags(&ws.side_stream, hipStreamNonBlocking));
  if (!ws.side_stream2) PCO_HIP_CHECK(hipStreamCreateWithFlags(&ws.side_stream2, hipStreamNonBlocking));
  if (!ws.join_event2) PCO_HIP_CHECK(hipEventCreateWithFlags(&ws.join_event2, hipEventDisableTiming));
  if (!ws.fork_event) PCO_HIP_CHECK(hipEventCreateWithFlags(&ws.fork_event, hipEventDisableTiming));
  if (!ws.join_event) PCO_HIP_CHECK(hipEventCreateWithFlags(&ws.join_event, hipEventDisableTiming));
  if (!ws.n_cus) { hipDeviceProp_t prop; PCO_HIP_CHECK(hipGetDeviceProperties(&prop, ws.device)); ws.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256; }
}

// blocks of the general one-wave-per-task kernel: each owns kTblWsBytes (832 KB) of global table scratch for tANS tables beyond its LDS,
// so the grid is what that scratch scales with -- 4096 blocks are four rounds of what the CUs hold at once, the kernel strides over the rest
constexpr size_t kGeneralGrid = 4096;
// The expanders under the walk pay from about a thousand chunks on: the publishing walker's chain is ~0.9 ms longer than the plain
// one's whatever the call holds, and that buys the expansion -- 0.7 us a chunk at scale.  Smaller calls (the host-buffer entry points
// decode one chunk per call) walk, then expand.
constexpr uint32_t kTrailMinChunks = 1024;

// the names pco_gfx_profile_* reports, per width group
enum { kNameTrailSpan, kNameWalkPub, kNameWalkRest, kNameTrail, kNameTrail2, kNameWalk, kNameWalk4, kNameExpand, kNameExpandLb, kNameGeneral, kDecodeNames };
#define PCO_DECODE_NAMES(w) {"dec_walk+trail<" w ">", "~dec_walk_kernel<" w ">", "~dec_walk_kernel(rest)<" w ">", "~dec_trail_kernel<" w ">", "~dec_trail2_kernel<" w ">", \
                             "dec_walk_kernel<" w ">", "dec_walk4_kernel<" w ">", "dec_expand_kernel<" w ">", "dec_expand_lb_kernel<" w ">", "pco_decode_kernel<" w ">"}
static const char* const kDecodeKernelNames[4][kDecodeNames] = {PCO_DECODE_NAMES("u64"), PCO_DECODE_NAMES("u32"), PCO_DECODE_NAMES("u16"), PCO_DECODE_NAMES("u8")};
#undef PCO_DECODE_NAMES

// what the steps of one decode call share
struct DecodeCall {
  Workspace& ws; hipStream_t stream; const PcoGfxDecodeTask* d_tasks; PcoGfxTaskResult* d_results; const MetaRef* d_metas;
};

// The fast path over one width group (decode_fast.hip): walk with 8 chunks per wave (the common chunks expanded on the side stream meanwhile), then
// with 4 for the chunks whose tables did not fit, then expand the rest.
struct FastDecodeStep {
  const DecodeCall& c; const char* const* names; uint32_t cnt, grid; const uint32_t* idp; DecPlan* d_plans; uint8_t* d_bins; uint8_t* d_sym; uint64_t sym_stride;
  uint64_t* d_offpos; uint64_t offpos_stride;
  bool use_trail; uint32_t trail_grid; uint32_t* d_progress; uint32_t* d_givebacks;   // the expanders under the walk: their grid, the hand-over words, the give-back counter

  template <class L>
  void launch() const {
    const uint32_t n_wb = (cnt + 7) / 8;
    PCO_RESERVE_LDS((dec_walk_kernel<L, 8>), 4 * WalkCfg<8>::kWalkLdsBytes, "dec_walk_kernel");
    PCO_RESERVE_LDS((dec_walk_kernel<L, 4>), 4 * WalkCfg<4>::kWalkLdsBytes, "dec_walk_kernel");
    if (use_trail) walk_under_expanders<L>(n_wb);
    else PCO_TIMED_LAUNCH(names[kNameWalk], c.stream, (dec_walk_kernel<L, 8>), dim3((n_wb + 3) / 4), dim3(256), 4 * WalkCfg<8>::kWalkLdsBytes, c.stream,
                          c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, 0u, c.d_results, (uint32_t*)nullptr, c.d_metas);
    PCO_TIMED_LAUNCH(names[kNameWalk4], c.stream, (dec_walk_kernel<L, 4>), dim3((cnt + 15) / 16), dim3(256), 4 * WalkCfg<4>::kWalkLdsBytes, c.stream,
                     c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, kStatusRetryK4, c.d_results, (uint32_t*)nullptr, c.d_metas);
    PCO_TIMED_LAUNCH(names[kNameExpand], c.stream, (dec_expand_kernel<L, false>), dim3(grid), dim3(256), kExpLdsBytes, c.stream,
                     c.d_tasks, c.d_results, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, (const uint32_t*)d_progress, d_givebacks);
    PCO_TIMED_LAUNCH(names[kNameExpandLb], c.stream, (dec_expand_kernel<L, true>), dim3(grid), dim3(256), kExpLbLdsBytes, c.stream,
                     c.d_tasks, c.d_results, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, (const uint32_t*)d_progress, d_givebacks);
  }

  // the 8-chunk walk as two walkers side by side and the expanders on the workspace's second stream, joined again on the caller's
  template <class L>
  void walk_under_expanders(uint32_t n_wb) const {
    Workspace& ws = c.ws; const hipStream_t stream = c.stream;
    TimedSpan span(names[kNameTrailSpan], stream);
    const dim3 trail_blocks(trail_grid), trail_threads(64 * kTrailWaves);
    if (g_trail_debug == 'd') {   // test switch: the expanders BEFORE the walkers on the caller's stream -- every wave times out waiting for a walker that has not started
      hipLaunchKernelGGL((dec_trail_kernel<L, false>), trail_blocks, trail_threads, 0, stream, c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_progress, n_wb, c.d_metas);
      hipLaunchKernelGGL((dec_trail_kernel<L, true>), trail_blocks, trail_threads, 0, stream, c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_progress, n_wb, c.d_metas);
    }
    PCO_HIP_CHECK(hipEventRecord(ws.fork_event, stream));
    // four walker waves per workgroup, the CU's whole LDS: one walker per SIMD by construction (decode_fast.hip, walk_lds)
    PCO_RESERVE_LDS(dec_walk_trail_kernel<L>, 4 * WalkCfg<8>::kWalkLdsBytes, "dec_walk_trail_kernel");
    PCO_TIMED_LAUNCH(names[kNameWalkPub], stream, (dec_walk_trail_kernel<L>), dim3((n_wb + 3) / 4), dim3(256), 4 * WalkCfg<8>::kWalkLdsBytes, stream,
                     c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, c.d_results, d_progress, c.d_metas);
    // the blocks without a candidate for the expanders: the ordinary walker, beside the two (every block runs in exactly one of the walkers).
    // Launched second: where no block is a candidate the publishing walker's blocks say so and leave at once, and the expanders with them
    // (launched first it held the LDS, they queued behind it: 1.8 instead of 1.3 ms per 16384 one-bin chunks).  Where every block is a
    // candidate its own blocks queue behind the publishing walker's LDS and then leave at once: its time in a profile is that wait
    PCO_HIP_CHECK(hipStreamWaitEvent(ws.side_stream2, ws.fork_event, 0));
    PCO_TIMED_LAUNCH(names[kNameWalkRest], ws.side_stream2, (dec_walk_kernel<L, 8>), dim3((n_wb + 3) / 4), dim3(256), 4 * WalkCfg<8>::kWalkLdsBytes, ws.side_stream2,
                     c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, 0u, c.d_results, d_progress, c.d_metas);
    PCO_HIP_CHECK(hipEventRecord(ws.join_event2, ws.side_stream2));
    hipStream_t ts = g_trail_debug == 's' ? stream : ws.side_stream;
    PCO_HIP_CHECK(hipStreamWaitEvent(ws.side_stream, ws.fork_event, 0));
    // one kernel per kind of walker block (classic chunks only / a chunk with two latent variables among them), one after the other on the
    // expanders' stream: the blocks of the kind a call does not have leave at once
    if (g_trail_debug != 'n' && g_trail_debug != 'd') {
      PCO_TIMED_LAUNCH(names[kNameTrail], ts, (dec_trail_kernel<L, false>), trail_blocks, trail_threads, 0, ts,
                       c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_progress, n_wb, c.d_metas);
      PCO_TIMED_LAUNCH(names[kNameTrail2], ts, (dec_trail_kernel<L, true>), trail_blocks, trail_threads, 0, ts,
                       c.d_tasks, idp, cnt, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride, d_progress, n_wb, c.d_metas);
    }
    PCO_HIP_CHECK(hipEventRecord(ws.join_event, ws.side_stream));
    PCO_HIP_CHECK(hipStreamWaitEvent(stream, ws.join_event, 0));
    PCO_HIP_CHECK(hipStreamWaitEvent(stream, ws.join_event2, 0));
  }
};

// The single-kernel decoder over one width group.  The first pass takes what the fast path left (`filt`: its plans, or null without one) and hands
// back what wants scratch; the second runs over exactly those tasks, with the history scratch.
struct GeneralDecodeStep {
  const DecodeCall& c; const char* name; uint32_t cnt; const uint32_t* idp; uint8_t* tbl; const uint32_t* filt; uint32_t fstride, retry_status; uint8_t* d_hist;
  const uint64_t* d_hoff; uint32_t need_hist;

  template <class L>
  void launch() const {
    PCO_TIMED_LAUNCH(name, c.stream, pco_decode_kernel<L>, dim3((uint32_t)std::min<size_t>(cnt, kGeneralGrid)), dim3(64), g_decode_lds_bytes, c.stream, c.d_tasks, c.d_results, idp, cnt,
                     g_decode_lds_bytes - kLdsFixed, tbl, filt, fstride, retry_status, d_hist, d_hoff, need_hist, c.d_metas);
  }
};

static void read_decode_results(const DecodeCall& c, size_t n_tasks, PcoGfxTaskResult* results) {
  PCO_HIP_CHECK(hipMemcpyAsync(results, c.d_results, n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, c.stream));
  PCO_HIP_CHECK(hipStreamSynchronize(c.stream));
}

// The device arrays of a decode call, side by side in the workspace's task buffer: tasks | ids (grouped by number width: the caller fills them, a mixed
// call only) | ChunkMeta references (wrapped pages away from their ChunkMeta) | a directory call's piece pairs.  Placed and uploaded; a directory
// call's sources and ChunkMeta references are resolved on the device; so are the source lengths of a verify call (verify.hip), whose wrapped form
// uploads its piece pairs beside the rest.
struct DecodeArrays { PcoGfxDecodeTask* d_tasks; uint32_t* d_ids; const MetaRef* d_metas; };
static DecodeArrays upload_decode_arrays(Workspace& ws, size_t n_tasks, const PcoGfxDecodeTask* tasks, const MetaRef* metas, const DirLaunch* dir, const VerifyPatch* verify, hipStream_t stream) {
  Layout at;
  const size_t tasks_off = at.place(n_tasks * sizeof(PcoGfxDecodeTask)), ids_off = at.place(n_tasks * sizeof(uint32_t));
  const size_t metas_off = at.place(metas || dir ? n_tasks * sizeof(MetaRef) : 0), pieces_off = dir ? at.place(n_tasks * sizeof(DirPieces)) : 0;
  const size_t bad_meta_off = dir && dir->chunks ? at.place(16) : 0;   // (a chunk directory call: the one-byte ChunkMeta of a refusal by Corruption, dir_resolve.hip)
  const size_t vpieces_off = verify && verify->pieces ? at.place(n_tasks * sizeof(VerifyPiece)) : 0;
  uint8_t* d_base = (uint8_t*)ws.tasks.ensure(at.end + 64);
  PcoGfxDecodeTask* d_tasks = (PcoGfxDecodeTask*)(d_base + tasks_off);
  if (metas) PCO_HIP_CHECK(hipMemcpyAsync(d_base + metas_off, metas, n_tasks * sizeof(MetaRef), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_tasks, tasks, n_tasks * sizeof(PcoGfxDecodeTask), hipMemcpyHostToDevice, stream));
  if (dir) {
    if (n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page directory: too many tasks"};
    PCO_HIP_CHECK(hipMemcpyAsync(d_base + pieces_off, dir->pieces, n_tasks * sizeof(DirPieces), hipMemcpyHostToDevice, stream));
    if (dir->chunks)
      PCO_TIMED_LAUNCH("dir_resolve_chunks_kernel", stream, dir_resolve_chunks_kernel<false>, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_tasks,
                       (MetaRef*)(d_base + metas_off), (const DirPieces*)(d_base + pieces_off), (const RangeRef*)nullptr, (uint32_t)n_tasks, dir->args, d_base + bad_meta_off);
    else
      PCO_TIMED_LAUNCH("dir_resolve_kernel", stream, dir_resolve_kernel<false>, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, d_tasks, (MetaRef*)(d_base + metas_off),
                       (const DirPieces*)(d_base + pieces_off), (const RangeRef*)nullptr, (uint32_t)n_tasks, dir->args);
  }
  if (verify) {
    if (n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: too many tasks"};
    const dim3 grid((uint32_t)((n_tasks + 255) / 256));
    if (verify->pieces) {   // (wrapped: `metas` holds placeholders)
      PCO_HIP_CHECK(hipMemcpyAsync(d_base + vpieces_off, verify->pieces, n_tasks * sizeof(VerifyPiece), hipMemcpyHostToDevice, stream));
      PCO_TIMED_LAUNCH("verify_resolve_kernel", stream, verify_resolve_wrapped_kernel, grid, dim3(256), 0, stream, d_tasks, (MetaRef*)(d_base + metas_off), (const VerifyPiece*)(d_base + vpieces_off),
                       verify->d_infos, (uint32_t)n_tasks);
    } else
      PCO_TIMED_LAUNCH("verify_resolve_kernel", stream, verify_resolve_kernel, grid, dim3(256), 0, stream, d_tasks, verify->d_encoded, (uint32_t)n_tasks);
  }
  return DecodeArrays{d_tasks, (uint32_t*)(d_base + ids_off), metas || dir ? (const MetaRef*)(d_base + metas_off) : nullptr};
}

// (defined behind launch_decode: the kernels are instantiated in the order of their first use, the fast path of every width first)
static void retry_with_history(const DecodeCall& c, size_t n_tasks, const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results);

// metas (HOST array of n_tasks entries, or nullptr): where each PCO_GFX_TASK_WRAPPED_PAGE task's ChunkMeta lives when it is not in front of the page
// dir (or nullptr; then metas is nullptr): the tasks' sources are null, and dir_resolve_kernel fills them and the ChunkMeta references on the
// device from the directory and dir->pieces (dir_resolve.hip)
// verify (or nullptr; then dir is nullptr): the decode behind an encode -- the tasks' source lengths, and for wrapped pages their sources and ChunkMeta
// references, are taken on the device from the encode's results (verify.hip)
static void launch_decode(size_t n_tasks, const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results,
                          PcoGfxTaskResult* d_results_user, hipStream_t stream, const MetaRef* metas = nullptr, const DirLaunch* dir = nullptr, const VerifyPatch* verify = nullptr) {
  if (n_tasks == 0) return;
  Workspace& ws = workspace();
  // group task ids by number width: one kernel instantiation per width present in the batch
  std::vector<uint32_t> ids[4];
  for (size_t i = 0; i < n_tasks; i++) {
    const int g = width_group(tasks[i].dtype);
    if (g < 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "decode: invalid number type"};
    ids[g].push_back((uint32_t)i);
  }
  PcoGfxTaskResult* d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)ws.results.ensure(n_tasks * sizeof(PcoGfxTaskResult));
  const DecodeArrays arr = upload_decode_arrays(ws, n_tasks, tasks, metas, dir, verify, stream);
  PcoGfxDecodeTask* d_tasks = arr.d_tasks; const uint32_t* d_ids = arr.d_ids; const MetaRef* d_metas = arr.d_metas;
  // (a call of one width passes a null id list and uploads none)
  const bool mixed = (ids[0].size() != n_tasks) && (ids[1].size() != n_tasks) && (ids[2].size() != n_tasks) && (ids[3].size() != n_tasks);
  std::vector<uint32_t> flat; size_t id_off[5] = {0, 0, 0, 0, 0};
  if (mixed) {
    flatten_groups(ids, flat, id_off);
    PCO_HIP_CHECK(hipMemcpyAsync(arr.d_ids, flat.data(), flat.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  }
  size_t max_grid = 0;
  for (int g = 0; g < 4; g++) max_grid = std::max(max_grid, std::min<size_t>(ids[g].size(), kGeneralGrid));
  // (synchronous calls: the table scratch only in the second pass, for the tasks that asked for it -- kStatusNeedHist covers both kinds of scratch)
  uint8_t* tbl = results ? nullptr : (uint8_t*)ws.tbl_ws.ensure(max_grid * kTblWsBytes);
  // Fast path (decode_fast.hip): walk 8 chunks per wave, then expand one chunk per wave; whatever it cannot take
  // (multi-chunk streams, big tANS tables, wrapped pages, ...) is finished by the single-kernel decoder.
  uint64_t max_cap = 0; bool plain = true;
  for (size_t i = 0; i < n_tasks; i++) { max_cap = std::max<uint64_t>(max_cap, tasks[i].dst_cap); if (tasks[i].flags & PCO_GFX_TASK_META_ONLY) plain = false; }   // (wrapped pages walk and expand like chunks)
  const uint64_t sym_stride = ((max_cap + 255) & ~(uint64_t)255) + 256, offpos_stride = sym_stride / 256 + 2;
  const bool fast = plain && n_tasks * 3 * sym_stride <= ((size_t)48 << 30);
  DecPlan* d_plans = nullptr; uint8_t* d_bins = nullptr; uint8_t* d_sym = nullptr; uint64_t* d_offpos = nullptr;
  if (fast) {
    d_plans = (DecPlan*)ws.dec_plans.ensure(n_tasks * sizeof(DecPlan));
    d_bins = (uint8_t*)ws.dec_bins.ensure(n_tasks * kBinsAreaPerTask);
    d_sym = (uint8_t*)ws.dec_sym.ensure(n_tasks * 3 * sym_stride + 64);
    d_offpos = (uint64_t*)ws.dec_offpos.ensure(n_tasks * 3 * offpos_stride * 8);
  }
  const DecodeCall call{ws, stream, d_tasks, d_results, d_metas};
  const uint32_t need_hist = results ? kStatusNeedHist : (uint32_t)PCO_GFX_UNSUPPORTED;   // (only a synchronous call can come back with the scratch)
  for (int g = 0; g < 4; g++) {
    if (ids[g].empty()) continue;
    const uint32_t cnt = (uint32_t)ids[g].size();
    const uint32_t* idp = mixed ? d_ids + id_off[g] : nullptr;
    if (fast) {
      const uint32_t n_wb = (cnt + 7) / 8;
      uint32_t* d_progress = nullptr;
      uint32_t* d_givebacks = nullptr;   // device counter: chunks marked for the expanders under the walk that dec_expand_kernel had to take (pco_gfx_trail_givebacks)
      const bool use_trail = g_decode_trail && (cnt >= kTrailMinChunks || g_trail_debug != '\0' || g_trail_always);
      if (use_trail) {
        ensure_side_stream(ws);
        d_progress = (uint32_t*)ws.dec_progress.ensure((size_t)n_wb * kTrailProgressStride * sizeof(uint32_t));
        PCO_HIP_CHECK(hipMemsetAsync(d_progress, 0, (size_t)n_wb * kTrailProgressStride * sizeof(uint32_t), stream));
        if (!ws.dec_stats.p) { ws.dec_stats.ensure(256); PCO_HIP_CHECK(hipMemsetAsync(ws.dec_stats.p, 0, 256, stream)); }   // (in stream order: nothing synchronous inside an asynchronous call)
        d_givebacks = (uint32_t*)ws.dec_stats.p;
      }
      // (persistent expander grid: at most four blocks of four waves per CU, so that every walker block finds its wave slot, registers and LDS
      //  whatever the order in which the two kernels' blocks arrive)
      const uint32_t trail_grid = use_trail ? std::min<uint32_t>(n_wb, (uint32_t)ws.n_cus * 4u) : 0u;
      launch_width(g, FastDecodeStep{call, kDecodeKernelNames[g], cnt, (uint32_t)std::min<size_t>(cnt, kGeneralGrid), idp, d_plans, d_bins, d_sym, sym_stride, d_offpos, offpos_stride,
                                     use_trail, trail_grid, d_progress, d_givebacks});
    }
    launch_width(g, GeneralDecodeStep{call, kDecodeKernelNames[g][kNameGeneral], cnt, idp, tbl, fast ? (const uint32_t*)d_plans : nullptr, (uint32_t)(sizeof(DecPlan) / 4), kStatusRetryLegacy,
                                      nullptr, nullptr, need_hist});
    PCO_HIP_CHECK(hipGetLastError());
  }
  if (!results) return;
  read_decode_results(call, n_tasks, results);
  retry_with_history(call, n_tasks, tasks, results);
}

// Tasks handed back for want of scratch (tANS tables beyond the LDS budget; a lookback delta whose secondary variable is delta'd too: its history needs dst_cap latents):
// once more through the single-kernel decoder, with the scratch.  The format allows the combination; no encoder writes it.
static void retry_with_history(const DecodeCall& c, size_t n_tasks, const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results) {
  std::vector<uint32_t> again[4];
  for (size_t i = 0; i < n_tasks; i++) if (results[i].status == kStatusNeedHist) again[width_group(tasks[i].dtype)].push_back((uint32_t)i);
  std::vector<uint32_t> flat_ids; size_t goff[5];
  flatten_groups(again, flat_ids, goff);
  const size_t n_again = flat_ids.size();
  if (!n_again) return;
  std::vector<uint64_t> offs; uint64_t hist_bytes = 0;
  for (uint32_t i : flat_ids) { offs.push_back(hist_bytes); hist_bytes += ((tasks[i].dst_cap * (uint64_t)(dtype_bits(tasks[i].dtype) / 8)) + 255) & ~(uint64_t)255; }
  uint8_t* d_hist = (uint8_t*)c.ws.dec_hist.ensure(hist_bytes + n_again * 12 + 256);
  uint64_t* d_hoff = (uint64_t*)(d_hist + ((hist_bytes + 15) & ~(uint64_t)15));
  uint32_t* d_again = (uint32_t*)(d_hoff + n_again);
  PCO_HIP_CHECK(hipMemcpyAsync(d_hoff, offs.data(), n_again * 8, hipMemcpyHostToDevice, c.stream));
  PCO_HIP_CHECK(hipMemcpyAsync(d_again, flat_ids.data(), n_again * 4, hipMemcpyHostToDevice, c.stream));
  uint8_t* tbl = (uint8_t*)c.ws.tbl_ws.ensure(std::min<size_t>(n_again, kGeneralGrid) * kTblWsBytes);
  for (int g = 0; g < 4; g++) {
    const uint32_t cnt = (uint32_t)(goff[g + 1] - goff[g]);
    if (!cnt) continue;
    launch_width(g, GeneralDecodeStep{c, kDecodeKernelNames[g][kNameGeneral], cnt, d_again + goff[g], tbl, nullptr, 0u, 0u, d_hist, d_hoff + goff[g], (uint32_t)PCO_GFX_UNSUPPORTED});
  }
  PCO_HIP_CHECK(hipGetLastError());
  read_decode_results(c, n_tasks, results);
}

}  // namespace pcogfx

using namespace pcogfx;

extern "C" {

int pco_gfx_last_status(void) { return g_err.status; }
const char* pco_gfx_last_error(void) { return g_err.msg.c_str(); }
int pco_gfx_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
void pco_gfx_release_workspace(void) {   // this thread's workspace on the current device
  try { Workspace& w = workspace(); if (w.has_last && w.last_event) (void)hipEventSynchronize(w.last_event); w.release_all(); } catch (...) {}
}

size_t pco_gfx_workspace_bytes(void) {
  try {
    static const bool trace = std::getenv("PCO_GFX_TRACE") != nullptr;
    if (trace) fprintf(stderr, "[pco_gfx trace] workspace: %s\n", workspace().device_report().c_str());
    return workspace().device_bytes();
  } catch (...) { return 0; }
}

static unsigned long long trail_stat(int which) {
  try {
    Workspace& w = workspace();
    const unsigned long long acc = which == 0 ? w.acc_givebacks : w.acc_marked;
    if (!w.dec_stats.p) return acc;
    if (w.has_last && w.last_event) (void)hipEventSynchronize(w.last_event);
    uint32_t v[2] = {0, 0};
    if (hipMemcpy(v, w.dec_stats.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return acc;
    return acc + v[which];
  } catch (...) { return 0; }
}
unsigned long long pco_gfx_trail_givebacks(void) { return trail_stat(0); }
unsigned long long pco_gfx_trail_marked(void) { return trail_stat(1); }
unsigned long long pco_gfx_strict_histogram_fallbacks(void) {
  try {
    Workspace& w = workspace();
    if (!w.enc_strict.p) return w.acc_strict;
    if (w.has_last && w.last_event) (void)hipEventSynchronize(w.last_event);
    uint32_t v = 0;
    if (hipMemcpy(&v, w.enc_strict.p, 4, hipMemcpyDeviceToHost) != hipSuccess) return w.acc_strict;
    return w.acc_strict + v;
  } catch (...) { return 0; }
}

// Kernel timing: begin() arms per-launch HIP events on this thread; end() synchronises and returns one
// (name, milliseconds) pair per kernel launched since begin().  Names are written NUL-separated.
void pco_gfx_profile_begin(void) {
  for (auto& r : g_prof.recs) { g_prof.give(r.a); g_prof.give(r.b); }
  g_prof.recs.clear(); g_prof.on = true;
}
int pco_gfx_profile_end(char* names, size_t names_cap, float* ms, int cap) {
  g_prof.on = false;
  int n = 0; size_t pos = 0;
  for (auto& r : g_prof.recs) {
    float t = 0.f;
    (void)hipEventSynchronize(r.b);
    (void)hipEventElapsedTime(&t, r.a, r.b);
    if (n < cap) {
      const size_t len = std::strlen(r.name) + 1;
      if (names && pos + len <= names_cap) { std::memcpy(names + pos, r.name, len); pos += len; }
      if (ms) ms[n] = t;
      n++;
    }
    g_prof.give(r.a); g_prof.give(r.b);
  }
  g_prof.recs.clear();
  return n;
}

size_t pco_gfx_guarantee_file_size(size_t n, unsigned char dtype, uint64_t max_page_n) {
  const int bits = dtype_bits(dtype);
  if (!bits) return 0;
  std::vector<size_t> pages;
  n_per_page(max_page_n, n, pages);
  size_t res = guarantee_standalone_header_size() + 1;
  for (size_t p : pages) res += guarantee_standalone_chunk_size(bits, p);
  return res;
}
size_t pco_standalone_guarantee_file_size(size_t n, unsigned char dtype) { return pco_gfx_guarantee_file_size(n, dtype, 0); }
size_t pco_gfx_guarantee_chunk_size(size_t n, unsigned char dtype) {
  const int bits = dtype_bits(dtype);
  return bits ? guarantee_standalone_chunk_size(bits, n) : 0;
}

size_t pco_gfx_write_standalone_header(void* dst, size_t dst_cap, uint64_t n_hint, unsigned char uniform_dtype) {
  // standalone/compressor.rs:12-16,85-105 + wrapped/file_compressor.rs:54-59
  HostBitWriter w;
  w.write(0x216f6370u, 32); w.write(3, 8); w.write(uniform_dtype, 8);
  const uint32_t power = n_hint == 0 ? 1 : (64 - (uint32_t)__builtin_clzll(n_hint));
  w.write(power - 1, kBitsVarintPower); w.write(n_hint, power); w.finish_byte();
  w.write(4, 8); w.write(1, 8);
  if (w.bytes() > dst_cap) return 0;
  std::memcpy(dst, w.buf.data(), w.bytes());
  return w.bytes();
}
size_t pco_gfx_write_standalone_footer(void* dst, size_t dst_cap) {
  if (dst_cap < 1) return 0;
  *(uint8_t*)dst = 0;
  return 1;
}
size_t pco_wrapped_write_header(void* dst, size_t dst_cap) {
  if (dst_cap < 2) return 0;
  ((uint8_t*)dst)[0] = 4; ((uint8_t*)dst)[1] = 1;
  return 2;
}
enum PcoError pco_wrapped_read_header(const void* src, size_t len, size_t* consumed, uint8_t* major, uint8_t* minor) {
  clear_error();
  const uint8_t* p = (const uint8_t*)src;
  if (len < 1) { set_error(PCO_GFX_INSUFFICIENT_DATA, "empty header"); return PcoDecompressionError; }
  uint8_t mj = p[0], mn = 0; size_t used = 1;
  if (mj >= 4) { if (len < 2) { set_error(PCO_GFX_INSUFFICIENT_DATA, "short header"); return PcoDecompressionError; } mn = p[1]; used = 2; }
  if (mj > 4) { set_error(PCO_GFX_CORRUPTION, "file's format version definitely cannot be decompressed"); return PcoDecompressionError; }
  if (consumed) *consumed = used; if (major) *major = mj; if (minor) *minor = mn;
  return PcoSuccess;
}

enum PcoError pco_gfx_decompress_chunks(size_t n_tasks, const PcoGfxDecodeTask* tasks, PcoGfxTaskResult* results,
                                        PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    require_device();
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_decode(n_tasks, tasks, results, d_results, (hipStream_t)stream); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "decode task " + std::to_string(i) + " failed");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}

enum PcoError pco_gfx_decompress_pages(size_t n_tasks, const PcoGfxPageTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    require_device();
    std::vector<PcoGfxDecodeTask> dt(n_tasks); std::vector<MetaRef> refs(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxPageTask& t = tasks[i];
      if (t.format_major > 4) throw HostError{PCO_GFX_CORRUPTION, "page task " + std::to_string(i) + ": the file's format version definitely cannot be decompressed"};   // wrapped/file_decompressor.rs:31-36
      if (t.meta == nullptr || t.page == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page task " + std::to_string(i) + ": null ChunkMeta or page"};
      dt[i] = PcoGfxDecodeTask{t.page, t.page_len, t.dst, t.page_n, t.dtype, PCO_GFX_TASK_WRAPPED_PAGE | (t.format_major << 8)};
      refs[i] = MetaRef{t.meta, t.meta_len};
    }
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_decode(n_tasks, dt.data(), results, d_results, (hipStream_t)stream, refs.data()); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "page task " + std::to_string(i) + " failed");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}

// include/pco_gfx.h section 4e: every argument is checked before anything is launched (and before a device is asked for)
enum PcoError pco_gfx_decompress_pages_dir(size_t n_tasks, const PcoGfxDirPageTask* tasks, const PcoGfxDirectory* dir, PcoGfxTaskResult* results,
                                           PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page directory: null task array"};
    DirLaunch dl{checked_directory(dir, "page"), nullptr};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page directory: results and d_results are both null"};
    std::vector<PcoGfxDecodeTask> dt(n_tasks); std::vector<DirPieces> pieces(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxDirPageTask& t = tasks[i];
      const std::string who = "directory page task " + std::to_string(i);
      if (t.format_major > 4) throw HostError{PCO_GFX_CORRUPTION, who + ": the file's format version definitely cannot be decompressed"};   // wrapped/file_decompressor.rs:31-36
      check_piece_pair(t.meta_piece, t.page_piece, dl.args.n_pieces, who);
      if (dtype_bits(t.dtype) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
      if (t.page_n == 0 || t.page_n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a page holds 1 ..= 2^24 numbers"};
      if (t.dst == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null dst"};
      dt[i] = PcoGfxDecodeTask{nullptr, 0, t.dst, t.page_n, t.dtype, PCO_GFX_TASK_WRAPPED_PAGE | (t.format_major << 8)};
      pieces[i] = DirPieces{t.meta_piece, t.page_piece};
    }
    if (n_tasks == 0) return PcoSuccess;
    require_device();
    dl.pieces = pieces.data();
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_decode(n_tasks, dt.data(), results, d_results, (hipStream_t)stream, nullptr, &dl); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "directory page task " + std::to_string(i) + " failed");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}

// include/pco_gfx.h section 4l: pco_gfx_decompress_pages_dir's checks and call, with each task's one piece a standalone chunk
enum PcoError pco_gfx_decompress_chunks_dir(size_t n_tasks, const PcoGfxDirPageTask* tasks, const PcoGfxDirectory* dir, PcoGfxTaskResult* results,
                                            PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "chunk directory: null task array"};
    DirLaunch dl{checked_directory(dir, "chunk"), nullptr, true};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "chunk directory: results and d_results are both null"};
    std::vector<PcoGfxDecodeTask> dt(n_tasks); std::vector<DirPieces> pieces(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxDirPageTask& t = tasks[i];
      const std::string who = "directory chunk task " + std::to_string(i);
      if (t.format_major > 4) throw HostError{PCO_GFX_CORRUPTION, who + ": the file's format version definitely cannot be decompressed"};
      check_chunk_piece(t.meta_piece, t.page_piece, dl.args.n_pieces, who);
      if (dtype_bits(t.dtype) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
      if (t.page_n == 0 || t.page_n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a chunk holds 1 ..= 2^24 numbers"};
      if (t.dst == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null dst"};
      dt[i] = PcoGfxDecodeTask{nullptr, 0, t.dst, t.page_n, t.dtype, PCO_GFX_TASK_WRAPPED_PAGE | (t.format_major << 8)};
      pieces[i] = DirPieces{t.meta_piece, t.page_piece};
    }
    if (n_tasks == 0) return PcoSuccess;
    require_device();
    dl.pieces = pieces.data();
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_decode(n_tasks, dt.data(), results, d_results, (hipStream_t)stream, nullptr, &dl); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "directory chunk task " + std::to_string(i) + " failed");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}

// ... and the same split of a chunk in HOST memory: pco_chunk_dir.h's two functions with gap 0, and no n to compare the preamble's with
enum PcoError pco_gfx_standalone_chunk_split(const void* chunk, size_t len, unsigned char dtype, uint8_t format_major, uint64_t* n, uint64_t* meta_len, uint64_t* page_len) {
  clear_error();
  if (!chunk || !n || !meta_len || !page_len || dtype_bits(dtype) == 0) { set_error(PCO_GFX_INVALID_ARGUMENT, "standalone_chunk_split: bad argument"); return PcoInvalidType; }
  *n = 0; *meta_len = 0; *page_len = 0;
  if (format_major > 4) { set_error(PCO_GFX_CORRUPTION, "standalone_chunk_split: the file's format version definitely cannot be decompressed"); return PcoDecompressionError; }
  uint64_t n_read = 0;
  const DirVerdict v = chunk_split_verdict((const uint8_t*)chunk, (const uint8_t*)chunk, len, dtype, 0, format_major, &n_read);
  if (v.status != kDirOk) {
    set_error((int)v.status, v.status == kDirCorruption ? "standalone_chunk_split: not a chunk of this number type, or an unknown mode or delta encoding" : "standalone_chunk_split: the chunk is cut short");
    return PcoDecompressionError;
  }
  *n = n_read; *meta_len = v.meta_len; *page_len = v.page_len;
  return PcoSuccess;
}

enum PcoError pco_gfx_compact_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoGfxTaskResult* d_results, void* d_dst,
                                     uint64_t dst_cap, uint64_t dst_offset, uint64_t* d_offsets, uint64_t* total, void* stream_) {
  clear_error();
  try {
    require_device();
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_results || !d_offsets || (!d_dst && dst_cap)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: null device array"};
    if (n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: too many chunks"};
    Workspace& ws = workspace();
    WorkspaceUse use(ws, stream);
    uint8_t* d_base = (uint8_t*)ws.compact_tasks.ensure(n_tasks * sizeof(PcoGfxEncodeTask) + 64);
    uint32_t* d_over = (uint32_t*)d_base; PcoGfxEncodeTask* d_tasks = (PcoGfxEncodeTask*)(d_base + 64);
    uint64_t max_cap = 0;
    for (size_t i = 0; i < n_tasks; i++) max_cap = std::max<uint64_t>(max_cap, tasks[i].dst_cap);
    if (n_tasks) PCO_HIP_CHECK(hipMemcpyAsync(d_tasks, tasks, n_tasks * sizeof(PcoGfxEncodeTask), hipMemcpyHostToDevice, stream));
    PCO_TIMED_LAUNCH("compact_scan_kernel", stream, compact_scan_kernel, dim3(1), dim3(1024), 0, stream, d_results, (uint32_t)n_tasks, dst_offset, dst_cap, d_offsets, d_over);
    if (n_tasks) {
      const uint64_t slice = 64 * 1024;   // one block per 64 KiB of a chunk: >> 256 blocks in flight for any many-chunk call
      const uint32_t slices = (uint32_t)std::max<uint64_t>(1, (max_cap + slice - 1) / slice);
      if ((uint64_t)slices * n_tasks >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: too many chunks for one call"};
      PCO_TIMED_LAUNCH("compact_copy_kernel", stream, compact_copy_kernel, dim3((uint32_t)(slices * n_tasks)), dim3(256), 0, stream, d_tasks, d_results, d_offsets, (uint8_t*)d_dst, d_over, (uint32_t)n_tasks, slice, slices);
    }
    PCO_HIP_CHECK(hipGetLastError());
    if (total) {
      uint32_t over = 0;
      PCO_HIP_CHECK(hipMemcpyAsync(total, d_offsets + n_tasks, 8, hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipMemcpyAsync(&over, d_over, 4, hipMemcpyDeviceToHost, stream));
      PCO_HIP_CHECK(hipStreamSynchronize(stream));
      if (over) throw HostError{PCO_GFX_INVALID_ARGUMENT, "compact: destination too small"};
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

// standalone/decompressor.rs:85-137 on the host: where the first chunk starts and which format version the file declares.  Anything out
// of the ordinary (old layouts without a version byte, a foreign uniform type, padding that is not zero, truncation) returns false and the
// device's own parser reports it.
static bool parse_standalone_header_host(const uint8_t* p, size_t len, unsigned char dtype, size_t& off, uint32_t& fmt_major) {
  if (len < 6 || p[0] != 'p' || p[1] != 'c' || p[2] != 'o' || p[3] != '!') return false;
  const uint32_t sv = p[4];
  if (sv < 2 || sv > 3) return false;
  size_t pos = 5;
  if (sv >= 3) { const uint32_t uniform = p[pos++]; if (uniform != 0 && uniform != dtype) return false; }
  if (pos + 9 > len) return false;
  uint64_t bits = 0; for (int i = 0; i < 9 && i < 8; i++) bits |= (uint64_t)p[pos + i] << (8 * i);
  const uint32_t power = 1 + (uint32_t)(bits & 63u);
  const uint32_t vbits = kBitsVarintPower + power, vbytes = (vbits + 7) / 8;
  if (vbits & 7) {   // the padding up to the byte boundary must be zero
    const uint32_t last = p[pos + vbytes - 1];
    if ((last >> (vbits & 7)) != 0) return false;
  }
  pos += vbytes;
  if (pos >= len) return false;
  fmt_major = p[pos++];
  if (fmt_major > 4) return false;
  if (fmt_major >= 4) pos++;
  if (pos > len) return false;
  off = pos;
  return true;
}

enum PcoError pco_standalone_simple_decompress_into(const void* compressed, size_t compressed_len, unsigned char dtype,
                                                    void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  const int bits = dtype_bits(dtype);
  if (!bits) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    require_device();
    Workspace& ws = workspace();
    WorkspaceUse use(ws, 0);   // (ordered behind an asynchronous batched call of this thread that may still be running on another stream)
    uint8_t* d_in = (uint8_t*)ws.io_in.ensure(compressed_len + 64);
    const size_t esz = (size_t)(bits / 8), out_bytes = dst_cap * esz;
    uint8_t* d_out = (uint8_t*)ws.io_out.ensure(out_bytes + 64);
    PCO_HIP_CHECK(hipMemsetAsync(d_in + compressed_len, 0, 64, 0));
    if (compressed_len) PCO_HIP_CHECK(hipMemcpyAsync(d_in, compressed, compressed_len, hipMemcpyHostToDevice, 0));
    // A file stores no chunk lengths: chunk k + 1 starts where chunk k's bit stream ends, so the chunks of one file decode one after the
    // other whatever does the decoding (standalone/decompressor.rs:233-301).  Each goes through the two-kernel path on its own (one
    // PCO_GFX_TASK_ONE_CHUNK task per chunk, ~4 ms of tANS chain latency each); handing the whole file to the single-kernel decoder, one
    // wave walking and expanding chunk after chunk, cost 14 ms per 2^18-number chunk.
    size_t off = 0, done = 0; uint32_t fmt_major = 4;
    const bool by_chunk = parse_standalone_header_host((const uint8_t*)compressed, compressed_len, dtype, off, fmt_major);
    if (!by_chunk) {
      PcoGfxDecodeTask task{d_in, compressed_len, d_out, dst_cap, dtype, PCO_GFX_TASK_HAS_FILE_HEADER};
      PcoGfxTaskResult res{};
      launch_decode(1, &task, &res, nullptr, 0);
      if (res.status != PCO_GFX_OK) {
        // a too-small dst is PcoDecompressionError, like pco_c/src/lib.rs:110-112
        set_error((int)res.status, "decompression failed");
        return PcoDecompressionError;
      }
      done = res.n_out;
    } else {
      for (;;) {
        if (off >= compressed_len) { set_error(PCO_GFX_INSUFFICIENT_DATA, "decompression failed: the file ends without its terminator"); return PcoDecompressionError; }
        if (((const uint8_t*)compressed)[off] == 0) break;   // the terminator where a chunk's type byte would be: a file without (further) chunks (standalone/decompressor.rs:190-200)
        // (a chunk holds at most 2^24 numbers: the scratch launch_decode sizes from dst_cap stays a chunk's, whatever the caller's buffer)
        PcoGfxDecodeTask task{d_in + off, compressed_len - off, d_out + done * esz, std::min<size_t>(dst_cap - done, kMaxEntries), dtype, PCO_GFX_TASK_ONE_CHUNK | (fmt_major << 8)};
        PcoGfxTaskResult res{};
        launch_decode(1, &task, &res, nullptr, 0);
        if (res.status != PCO_GFX_OK) { set_error((int)res.status, "decompression failed"); return PcoDecompressionError; }
        done += res.n_out; off += res.consumed;
        if (res.aux & 1u) { if (res.consumed == 0) break; continue; }   // another chunk follows
        // the last chunk: the file must still hold its terminator byte (standalone/decompressor.rs:190-200: chunk_preamble fails with
        // InsufficientData on a file that ends right behind a chunk); the kernels report it consumed through aux bit 1
        if (!(res.aux & 2u)) { set_error(PCO_GFX_INSUFFICIENT_DATA, "decompression failed: the file ends without its terminator"); return PcoDecompressionError; }
        break;
      }
    }
    if (done) PCO_HIP_CHECK(hipMemcpy(dst, d_out, done * esz, hipMemcpyDeviceToHost));
    if (n_written) *n_written = done;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}

}  // extern "C"

// the encode side, by concern (host code; pco_launch.h and DESIGN.md, "Host drivers")
#include "pco_encode_config.inc"    // PcoChunkConfigEx resolved and validated, explicit plans
#include "pco_encode_specs.inc"     // PcoGfxChunkSpec <-> plan, a spec's validation (section 3c)
#include "pco_gfx_encode_api.inc"   // run_encode: EncodeCall and the phases of one pass of the pipeline
#include "pco_encode_auto.inc"      // resolve_plans: Auto mode, Auto delta
#include "pco_verify_host.inc"      // the verified encode: launch_verify[_wrapped], pco_gfx_verify_chunks / _wrapped_chunks
#include "pco_encode_passes.inc"    // Dict build, launch_encode, wrapped paging, pass cutting
#include "pco_encode_entry.inc"     // the extern "C" encode entry points
#include "pco_encode_specs_entry.inc"   // ... and section 3c's: resolve, spec from a ChunkMeta, encode from specs
#include "pco_wrapped_handles.inc"  // pco_chunk_compressor_* / pco_page_decompressor_* handles
#include "pco_meta_info.inc"        // pco_gfx_chunk_meta_info
#include "pco_gfx_comm.inc"

// Test hook: stage 1 of Auto mode detection on floats (auto_float_stats_kernel) on a host array taken as the sample, in order.
// out: s_size, tz5, n_gcd, sim[3], hist[56], then has_euclid, k, n_ints, base_c (lo, hi).  Lets the GPU tests check the device's
// arithmetic against an IEEE reference (numpy).
extern "C" int pco_gfx_debug_float_screen(const void* values, size_t n, uint32_t dtype, uint32_t* out) {
  using namespace pcogfx;
  if (n == 0 || n > kAutoCap || dtype_kind(dtype) != kFloat || dtype_bits(dtype) < 32) return PCO_GFX_INVALID_ARGUMENT;
  const size_t eb = dtype_bits(dtype) / 8;
  void* d_vals = nullptr; void* d_sbuf = nullptr; uint32_t* d_idx = nullptr; FloatStatsTask* d_task = nullptr; FloatStatsResult* d_res = nullptr;
  std::vector<uint32_t> idx(n); for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
  int rc = PCO_GFX_OK;
  if (hipFuncSetAttribute((const void*)auto_float_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kAutoStage1LdsBytes) != hipSuccess) return PCO_GFX_DEVICE_ERROR;
  if (hipMalloc(&d_vals, n * eb) != hipSuccess || hipMalloc(&d_sbuf, kAutoCap * 8) != hipSuccess || hipMalloc((void**)&d_idx, n * 4) != hipSuccess || hipMalloc((void**)&d_task, sizeof(FloatStatsTask)) != hipSuccess || hipMalloc((void**)&d_res, sizeof(FloatStatsResult)) != hipSuccess) rc = PCO_GFX_DEVICE_ERROR;
  if (rc == PCO_GFX_OK) {
    const FloatStatsTask t{d_vals, d_idx, d_sbuf, (uint32_t)n, dtype};
    static FloatStatsResult r;
    if (hipMemcpy(d_vals, values, n * eb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_idx, idx.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_task, &t, sizeof(t), hipMemcpyHostToDevice) != hipSuccess) rc = PCO_GFX_DEVICE_ERROR;
    else {
      hipLaunchKernelGGL(auto_float_stats_kernel, dim3(1), dim3(kAutoT), kAutoStage1LdsBytes, 0, d_task, d_res);
      if (hipMemcpy(&r, d_res, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess) rc = PCO_GFX_DEVICE_ERROR;
      else {
        out[0] = r.s_size; out[1] = r.tz5; out[2] = r.n_gcd; out[3] = r.sim[0]; out[4] = r.sim[1]; out[5] = r.sim[2]; for (int i = 0; i < 56; i++) out[6 + i] = r.hist[i];
        out[62] = r.has_euclid; out[63] = (uint32_t)r.k; out[64] = r.n_ints; out[65] = (uint32_t)r.base_c; out[66] = (uint32_t)(r.base_c >> 32);
      }
    }
  }
  (void)hipFree(d_vals); (void)hipFree(d_sbuf); (void)hipFree(d_idx); (void)hipFree(d_task); (void)hipFree(d_res);
  return rc;
}

// Test hook: which kernel decided each page of the calling thread's last lookback pass (the skip list of enc_lookback_hash_kernel's screen and
// the redo list enc_lookback_pipe_kernel and enc_lookback_seq_kernel leave in enc_lb), in the order of the call's lookback pages.  Reads only.
extern "C" int64_t pco_gfx_debug_lookback_routes(uint8_t* out, size_t cap) {
  using namespace pcogfx;
  Workspace& w = workspace();
  const size_t n = w.lb_n;
  if (n == 0 || !w.enc_lb.p || (std::max(w.lb_redo_off, w.lb_skip_off) + n) * 4 > w.enc_lb.cap) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  std::vector<uint32_t> redo(n), skip(n);
  const uint32_t* base = (const uint32_t*)w.enc_lb.p;
  if (hipMemcpy(redo.data(), base + w.lb_redo_off, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(skip.data(), base + w.lb_skip_off, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  for (size_t k = 0; k < n && k < cap; k++) out[k] = redo[k] ? 2 : (skip[k] ? 1 : 0);   // (a screened page enc_lookback_seq_kernel declined keeps its redo flag: the one-wave kernel decided it)
  return (int64_t)n;
}

// Test hook: the unoptimized histogram of one variable of one chunk of the calling thread's last encode pass, as the histogram kernels left it in
// the chunk's plan region (hlower / hupper / hcount: enc_train_kernel and enc_train_big_kernel read them, nothing writes them again), with what
// EncVar says of it.  Reads only.
extern "C" int64_t pco_gfx_debug_histogram(uint32_t task, uint32_t var, uint64_t* lower, uint64_t* upper, uint32_t* count, size_t cap, uint32_t* info) {
  using namespace pcogfx;
  if (var >= 3 || info == nullptr || (cap != 0 && (lower == nullptr || upper == nullptr || count == nullptr))) return -(int64_t)PCO_GFX_INVALID_ARGUMENT;
  Workspace& w = workspace();
  const size_t nt = w.hist_nt; const uint64_t pcap = w.hist_plan_cap, pb = plan_bytes_for(w.hist_plan_cap);
  if (nt == 0 || task >= nt || !w.enc_state.p || w.hist_plans_off < nt * sizeof(EncChunk) || w.hist_plans_off + nt * 3 * pb > w.enc_state.cap) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  EncChunk ch;
  if (hipMemcpy(&ch, (const EncChunk*)w.enc_state.p + task, sizeof(EncChunk), hipMemcpyDeviceToHost) != hipSuccess) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  const EncVar& ev = ch.v[var];
  info[0] = ev.n_lat; info[1] = var == 2 ? std::min(ch.unopt_bins_log, 6u) : ch.unopt_bins_log; info[2] = ev.hist_path; info[3] = ch.status;
  if (!ev.present || ev.n_hist > pcap) return 0;
  const size_t k = std::min<size_t>(ev.n_hist, cap);
  const uint8_t* plan = (const uint8_t*)w.enc_state.p + w.hist_plans_off + ((size_t)task * 3 + var) * pb;   // (PlanRef: u64 hlower[cap] hupper[cap] ... u32 hcount[cap] at 24 * cap)
  if (k != 0 && (hipMemcpy(lower, plan, k * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(upper, plan + 8 * pcap, k * 8, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(count, plan + 24 * pcap, k * 4, hipMemcpyDeviceToHost) != hipSuccess)) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  return (int64_t)ev.n_hist;
}

// Test hook: which pack kernel wrote each page of the calling thread's last encode pass, from what enc_scan_kernel left in EncPage::pad (bit 0:
// the page did not fit; bit 8: the fast path sized it, with the lean kernel's shape in bits 4-7; neither: the page was left to enc_page_kernel --
// the host uploads pad as 0 and nothing else writes it).  Reads only.
extern "C" int64_t pco_gfx_debug_pack_routes(uint8_t* out, size_t cap) {
  using namespace pcogfx;
  if (cap != 0 && out == nullptr) return -(int64_t)PCO_GFX_INVALID_ARGUMENT;
  Workspace& w = workspace();
  const size_t n = w.pack_np;
  if (n == 0 || !w.enc_small.p || w.pack_pages_off + n * sizeof(EncPage) > w.enc_small.cap) return 0;
  if (hipDeviceSynchronize() != hipSuccess) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  const size_t k = std::min(n, cap);
  std::vector<EncPage> pages(k);
  if (k != 0 && hipMemcpy(pages.data(), (const uint8_t*)w.enc_small.p + w.pack_pages_off, k * sizeof(EncPage), hipMemcpyDeviceToHost) != hipSuccess) return -(int64_t)PCO_GFX_DEVICE_ERROR;
  for (size_t i = 0; i < k; i++) { const uint32_t pad = pages[i].pad; out[i] = (pad & 1u) ? 0xfe : ((pad & 0x100u) ? (uint8_t)((pad >> 4) & 0xfu) : 0xff); }
  return (int64_t)n;
}

// Test hook: what Auto mode detection held on the host for the first chunks of the calling thread's last encode call (resolve_plans keeps
// the copies in the workspace).  Launches nothing, reads nothing from the device.
extern "C" int64_t pco_gfx_debug_auto_mode(PcoGfxAutoModeRecord* out, size_t cap) {
  using namespace pcogfx;
  try {
    const std::vector<PcoGfxAutoModeRecord>& v = workspace().auto_dbg;
    for (size_t k = 0; k < v.size() && k < cap; k++) out[k] = v[k];
    return (int64_t)v.size();
  } catch (const HostError& e) { return -(int64_t)e.status; }
}

// Test hook: what the Auto delta trials cost and what the replayed decision chose for the first chunks of the calling thread's last encode call
// (resolve_auto_delta keeps the copies in the workspace).  Launches nothing, reads nothing from the device.
extern "C" int64_t pco_gfx_debug_auto_delta(PcoGfxAutoDeltaRecord* out, size_t cap) {
  using namespace pcogfx;
  try {
    const std::vector<PcoGfxAutoDeltaRecord>& v = workspace().auto_delta_dbg;
    for (size_t k = 0; k < v.size() && k < cap; k++) out[k] = v[k];
    return (int64_t)v.size();
  } catch (const HostError& e) { return -(int64_t)e.status; }
}
