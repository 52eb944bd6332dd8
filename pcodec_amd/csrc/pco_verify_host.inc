// pco_verify_host.inc -- the verified encode (included by pco_gfx.hip; include/pco_gfx.h section 3b): launch_verify / launch_verify_wrapped, which
// the encode launchers call behind a flagged encode and the two public entry points call on their own -- one implementation -- and those entry points.
namespace pcogfx {

// what the buffers a verify takes hold, beside the encode buffers (the remembered footprint of a flagged call in passes)
static size_t verify_held_bytes() {
  const Workspace& w = workspace();
  return w.verify_scratch.cap + w.verify_small.cap + w.verify_infos.cap + w.tasks.cap + w.dec_plans.cap + w.dec_bins.cap + w.dec_sym.cap + w.dec_offpos.cap + w.dec_progress.cap + w.tbl_ws.cap;
}
// ... and what they take per chunk of at most `stride` numbers in the worst case: the scratch slot, three symbol streams and their offset positions, the
// bin area and plan of the fast decode path, and the task, item and result records
static size_t verify_per_task_bytes(size_t stride) {
  return stride * 8 + 3 * stride + 3 * (stride / 256 + 2) * 8 + kBinsAreaPerTask + sizeof(DecPlan) + sizeof(PcoGfxDecodeTask) + sizeof(MetaRef) + sizeof(VerifyItem) + sizeof(VerifyPiece) +
         3 * sizeof(PcoGfxTaskResult) + 64;
}

// The compare kernel's grid is (64 KiB pieces of the longest item) x items, below 2^31 blocks: the limit of a verify call, checked by a flagged
// encode before it launches anything (include/pco_gfx.h section 3b)
static void check_verify_grid(uint64_t max_item_bytes, uint64_t n_items) {
  const uint64_t pieces = (std::max<uint64_t>(max_item_bytes, 1) + 65535) / 65536;
  if (pieces * n_items >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: too many chunks for one call (2^31 / ceil(longest chunk's bytes / 64 KiB) at most)"};
}

// The items of one verify: their scratch slots handed out, the device arrays placed, the first-difference words set.
struct VerifyArrays { VerifyItem* d_items; unsigned long long* d_first; PcoGfxTaskResult* d_dec; uint8_t* d_extra; uint8_t* d_scratch; uint32_t pieces; };
static uint32_t log2_width(uint32_t dtype) { const int b = dtype_bits(dtype); return b == 64 ? 3u : (b == 32 ? 2u : (b == 16 ? 1u : 0u)); }
// items[i].dec holds the item's OFFSET into the scratch on entry and its address on return; `extra_bytes` more are placed behind the arrays (d_extra)
static VerifyArrays place_verify_arrays(Workspace& ws, std::vector<VerifyItem>& items, size_t scratch_bytes, size_t extra_bytes, hipStream_t stream) {
  const size_t n = items.size();
  Layout at;
  const size_t items_off = at.place(n * sizeof(VerifyItem)), first_off = at.place(n * 8), dec_off = at.place(n * sizeof(PcoGfxTaskResult)), extra_off = at.place(extra_bytes);
  uint8_t* d_small = (uint8_t*)ws.verify_small.ensure(at.end + 64);
  uint8_t* d_scratch = (uint8_t*)ws.verify_scratch.ensure(scratch_bytes + 64);
  uint64_t max_bytes = 1;
  for (auto& it : items) { it.dec = d_scratch + (size_t)(uintptr_t)it.dec; max_bytes = std::max<uint64_t>(max_bytes, it.n << it.esz_log); }
  const uint64_t pieces = (max_bytes + kVerifyPieceBytes - 1) / kVerifyPieceBytes;
  if (pieces * n >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: too many chunks for one call (2^31 / ceil(longest chunk's bytes / 64 KiB) at most)"};
  PCO_HIP_CHECK(hipMemcpyAsync(d_small + items_off, items.data(), n * sizeof(VerifyItem), hipMemcpyHostToDevice, stream));
  PCO_HIP_CHECK(hipMemsetAsync(d_small + first_off, 0xff, n * 8, stream));
  return VerifyArrays{(VerifyItem*)(d_small + items_off), (unsigned long long*)(d_small + first_off), (PcoGfxTaskResult*)(d_small + dec_off), d_small + extra_off, d_scratch, (uint32_t)pieces};
}
static void launch_verify_compare(const VerifyArrays& a, size_t n_items, hipStream_t stream) {
  PCO_TIMED_LAUNCH("verify_compare_kernel", stream, verify_compare_kernel, dim3((uint32_t)(a.pieces * n_items)), dim3(256), 0, stream, (const VerifyItem*)a.d_items, (const PcoGfxTaskResult*)a.d_dec,
                   a.d_first, (uint32_t)n_items, a.pieces);
}

// Standalone chunks.  d_encoded: the encode's results on the device.  results (HOST, or nullptr: asynchronous) / d_out (DEVICE; may be d_encoded, or
// nullptr with results: workspace) receive the verdicts.
static void launch_verify(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoGfxTaskResult* d_encoded, PcoGfxTaskResult* results, PcoGfxTaskResult* d_out, hipStream_t stream) {
  if (n_tasks == 0) return;
  Workspace& ws = workspace();
  std::vector<VerifyItem> items(n_tasks); std::vector<PcoGfxDecodeTask> dt(n_tasks);
  size_t scratch = 0;
  for (size_t i = 0; i < n_tasks; i++) {
    const PcoGfxEncodeTask& t = tasks[i];
    const uint32_t lg = log2_width(t.dtype);
    items[i] = VerifyItem{t.src, (const void*)(uintptr_t)scratch, t.n, lg, 0};
    scratch += ((t.n << lg) + 255) & ~(size_t)255;
  }
  const VerifyArrays a = place_verify_arrays(ws, items, scratch, d_out ? 0 : n_tasks * sizeof(PcoGfxTaskResult), stream);
  if (!d_out) d_out = (PcoGfxTaskResult*)a.d_extra;
  // the decode of the bytes just written: a chunk's length is patched in on the device (verify_resolve_kernel), bounded by what its dst holds
  for (size_t i = 0; i < n_tasks; i++) dt[i] = PcoGfxDecodeTask{tasks[i].dst, tasks[i].dst_cap - 16, (void*)items[i].dec, tasks[i].n, tasks[i].dtype, 0};
  const VerifyPatch patch{d_encoded, nullptr, nullptr};
  std::vector<PcoGfxTaskResult> dec_host(results ? n_tasks : 0);
  launch_decode(n_tasks, dt.data(), results ? dec_host.data() : nullptr, a.d_dec, stream, nullptr, nullptr, &patch);
  launch_verify_compare(a, n_tasks, stream);
  PCO_TIMED_LAUNCH("verify_finish_kernel", stream, verify_finish_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, (const VerifyItem*)a.d_items, d_encoded,
                   (const PcoGfxTaskResult*)a.d_dec, (const unsigned long long*)a.d_first, d_out, (uint32_t)n_tasks);
  PCO_HIP_CHECK(hipGetLastError());
  if (results) {
    PCO_HIP_CHECK(hipMemcpyAsync(results, d_out, n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
}

// Wrapped chunks: chunk i's pages are sizes[first[i] .. first[i + 1]) numbers long; its pieces -- the ChunkMeta's, then one per page -- are entries
// first[i] - first[0] + i and on of d_encoded, the encode's piece directory on the device.  infos / d_out as results / d_out above.
static void launch_verify_wrapped(size_t n_tasks, const PcoGfxWrappedTask* wt, const uint64_t* sizes, const size_t* first, const PcoGfxPageInfo* d_encoded, PcoGfxPageInfo* infos,
                                  PcoGfxPageInfo* d_out, hipStream_t stream) {
  if (n_tasks == 0) return;
  Workspace& ws = workspace();
  const size_t n_pages = first[n_tasks] - first[0], n_pieces = n_pages + n_tasks;
  std::vector<VerifyItem> items(n_pages); std::vector<PcoGfxDecodeTask> dt(n_pages); std::vector<MetaRef> refs(n_pages); std::vector<VerifyPiece> pieces(n_pages);
  std::vector<VerifyChunk> chunks(n_tasks); std::vector<uint32_t> dtypes(n_pages);
  size_t scratch = 0, k = 0;
  for (size_t i = 0; i < n_tasks; i++) {
    const PcoGfxWrappedTask& t = wt[i];
    const uint32_t lg = log2_width(t.dtype), piece0 = (uint32_t)(first[i] - first[0] + i);
    chunks[i] = VerifyChunk{piece0, (uint32_t)(first[i + 1] - first[i]), (uint32_t)k, 0};
    uint64_t start = 0;
    for (size_t p = first[i]; p < first[i + 1]; p++, k++) {
      items[k] = VerifyItem{(const uint8_t*)t.src + (start << lg), (const void*)(uintptr_t)scratch, sizes[p], lg, 0};
      pieces[k] = VerifyPiece{(const uint8_t*)t.dst, t.dst_cap, piece0, piece0 + 1 + (uint32_t)(p - first[i])};
      dtypes[k] = t.dtype; scratch += ((sizes[p] << lg) + 255) & ~(size_t)255; start += sizes[p];
    }
  }
  const VerifyArrays a = place_verify_arrays(ws, items, scratch, n_tasks * sizeof(VerifyChunk) + 16 + (d_out ? 0 : n_pieces * sizeof(PcoGfxPageInfo)), stream);
  VerifyChunk* d_chunks = (VerifyChunk*)a.d_extra;
  if (!d_out) d_out = (PcoGfxPageInfo*)(a.d_extra + ((n_tasks * sizeof(VerifyChunk) + 15) & ~(size_t)15));
  PCO_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), n_tasks * sizeof(VerifyChunk), hipMemcpyHostToDevice, stream));
  // every page a task of its own, its source and its ChunkMeta reference filled in on the device from the directory (verify_resolve_kernel)
  for (size_t j = 0; j < n_pages; j++) {
    dt[j] = PcoGfxDecodeTask{pieces[j].dst, 0, (void*)items[j].dec, items[j].n, dtypes[j], PCO_GFX_TASK_WRAPPED_PAGE | (4u << 8)};
    refs[j] = MetaRef{pieces[j].dst, 0};
  }
  const VerifyPatch patch{nullptr, d_encoded, pieces.data()};
  std::vector<PcoGfxTaskResult> dec_host(infos ? n_pages : 0);
  launch_decode(n_pages, dt.data(), infos ? dec_host.data() : nullptr, a.d_dec, stream, refs.data(), nullptr, &patch);
  launch_verify_compare(a, n_pages, stream);
  PCO_TIMED_LAUNCH("verify_finish_kernel", stream, verify_finish_wrapped_kernel, dim3((uint32_t)((n_tasks + 255) / 256)), dim3(256), 0, stream, (const VerifyChunk*)d_chunks,
                   (const VerifyItem*)a.d_items, d_encoded, (const PcoGfxTaskResult*)a.d_dec, (const unsigned long long*)a.d_first, d_out, (uint32_t)n_tasks);
  PCO_HIP_CHECK(hipGetLastError());
  if (infos) {
    PCO_HIP_CHECK(hipMemcpyAsync(infos, d_out, n_pieces * sizeof(PcoGfxPageInfo), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
}

// the host checks both entry points share, on one chunk's numbers and destination
static void check_verify_task(const void* src, uint64_t n, uint32_t dtype, const void* dst, uint64_t dst_cap, const std::string& who) {
  if (n == 0 || n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a chunk holds 1 ..= 2^24 numbers"};
  if (dtype_bits(dtype) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
  if (dst_cap < 16) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": dst_cap is below 16"};
  if (src == nullptr || dst == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null src or dst"};
  if ((uintptr_t)src & (uintptr_t)(dtype_bits(dtype) / 8 - 1)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": src must be naturally aligned"};   // (as validate_task asks of an encode)
}

}  // namespace pcogfx

extern "C" {

enum PcoError pco_gfx_verify_chunks(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoGfxTaskResult* d_encoded, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results,
                                    void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: null task array"};
    if (!d_encoded) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: null d_encoded"};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: results and d_results are both null"};
    for (size_t i = 0; i < n_tasks; i++) check_verify_task(tasks[i].src, tasks[i].n, tasks[i].dtype, tasks[i].dst, tasks[i].dst_cap, "verify task " + std::to_string(i));
    if (n_tasks == 0) return PcoSuccess;
    require_device();
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_verify(n_tasks, tasks, d_encoded, results, d_results, (hipStream_t)stream); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "verify task " + std::to_string(i) + (results[i].status == PCO_GFX_CORRUPTION ? " does not read back to its source" : " was not encoded"));
      return PcoCompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

enum PcoError pco_gfx_verify_wrapped_chunks(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config, const PcoGfxPageInfo* d_encoded, PcoGfxPageInfo* infos,
                                            PcoGfxPageInfo* d_infos, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: null task array"};
    if (!d_encoded) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: null d_encoded"};
    if (!infos && !d_infos) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: infos and d_infos are both null"};
    const uint64_t max_page_n = config && config->max_page_n ? config->max_page_n : (1u << 18);
    std::vector<uint64_t> sizes; std::vector<size_t> first(n_tasks + 1, 0), pn;
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxWrappedTask& t = tasks[i];
      const std::string who = "verify wrapped chunk " + std::to_string(i);
      check_verify_task(t.src, t.n, t.dtype, t.dst, t.dst_cap, who);
      if ((t.n_pages != 0) != (t.page_sizes != nullptr)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": page_sizes must be NULL exactly when n_pages is 0"};
      if (t.n_pages) {
        uint64_t sum = 0;
        for (uint32_t k = 0; k < t.n_pages; k++) { if (t.page_sizes[k] == 0 || t.page_sizes[k] > t.n) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a page of 0 numbers, or of more than the chunk's"}; sum += t.page_sizes[k]; }
        if (sum != t.n) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": the page sizes do not sum to n"};
        sizes.insert(sizes.end(), t.page_sizes, t.page_sizes + t.n_pages);
      } else { n_per_page(max_page_n, t.n, pn); sizes.insert(sizes.end(), pn.begin(), pn.end()); }
      first[i + 1] = sizes.size();
    }
    const size_t n_pieces = sizes.size() + n_tasks;
    if (n_pieces >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "verify: too many pieces for one call"};
    if (n_tasks == 0) return PcoSuccess;
    require_device();
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_verify_wrapped(n_tasks, tasks, sizes.data(), first.data(), d_encoded, infos, d_infos, (hipStream_t)stream); }
    if (infos) for (size_t k = 0; k < n_pieces; k++) if (infos[k].status != PCO_GFX_OK) {
      set_error((int)infos[k].status, "verify: wrapped piece " + std::to_string(k) + (infos[k].status == PCO_GFX_CORRUPTION ? " does not read back to its source" : " was not encoded"));
      return PcoCompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

}  // extern "C"
