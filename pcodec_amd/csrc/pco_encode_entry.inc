// pco_encode_entry.inc -- the extern "C" encode entry points of the C ABI (included by pco_gfx.hip, behind pco_encode_passes.inc).
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
