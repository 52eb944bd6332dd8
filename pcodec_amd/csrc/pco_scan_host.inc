// pco_scan_host.inc -- include/pco_gfx.h section 4m: the chunk directory of standalone streams, scanned on the device (scan.hip).  ONE launch, one wave
// per stream; the global table scratch is taken up front in both forms, as an asynchronous decode takes it.  A driver of its own, which shares nothing
// with the partial decode but the single-kernel decoder's LDS and grid bounds (pco_partial_driver.inc); pco_gfx_ranges.hip includes it behind scan.hip.

namespace pcogfx {
namespace {

void launch_scan(size_t n_tasks, const PcoGfxScanTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results_user, hipStream_t stream) {
  Workspace& ws = workspace();
  PcoGfxScanTask* d_tasks = (PcoGfxScanTask*)ws.tasks.ensure(n_tasks * sizeof(PcoGfxScanTask) + 64);
  PcoGfxTaskResult* d_results = d_results_user ? d_results_user : (PcoGfxTaskResult*)ws.results.ensure(n_tasks * sizeof(PcoGfxTaskResult));
  const size_t grid = std::min<size_t>(n_tasks, kPartialGeneralGrid);
  uint8_t* tbl = (uint8_t*)ws.tbl_ws.ensure(grid * kTblWsBytes);
  PCO_HIP_CHECK(hipMemcpyAsync(d_tasks, tasks, n_tasks * sizeof(PcoGfxScanTask), hipMemcpyHostToDevice, stream));
  PCO_TIMED_LAUNCH("pco_scan_kernel", stream, pco_scan_kernel, dim3((uint32_t)grid), dim3(64), kPartialDecodeLdsBytes, stream, (const PcoGfxScanTask*)d_tasks, d_results, (uint32_t)n_tasks,
                   kPartialDecodeLdsBytes - kLdsFixed, tbl);
  PCO_HIP_CHECK(hipGetLastError());
  if (results) {
    PCO_HIP_CHECK(hipMemcpyAsync(results, d_results, n_tasks * sizeof(PcoGfxTaskResult), hipMemcpyDeviceToHost, stream));
    PCO_HIP_CHECK(hipStreamSynchronize(stream));
  }
}

}  // namespace
}  // namespace pcogfx

extern "C" enum PcoError pco_gfx_scan_chunks(size_t n_tasks, const PcoGfxScanTask* tasks, PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "scan: null task array"};
    if (!results && !d_results) throw HostError{PCO_GFX_INVALID_ARGUMENT, "scan: results and d_results are both null"};
    for (size_t i = 0; i < n_tasks; i++) {
      const PcoGfxScanTask& t = tasks[i];
      const std::string who = "scan task " + std::to_string(i);
      if (t.src == nullptr || t.d_offsets == nullptr || t.d_counts == nullptr) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": null src, d_offsets or d_counts"};
      if (t.max_chunks == 0 || t.max_chunks >= (1u << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": max_chunks must be 1 ..= 2^31 - 1"};
      if (width_group(t.dtype) < 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": invalid number type"};
      if (t.reserved != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": reserved must be 0"};
      if (t.flags & ~(PCO_GFX_TASK_HAS_FILE_HEADER | 0xff00u)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": unknown flag bits"};
      if (((uintptr_t)t.d_offsets & 7u) || ((uintptr_t)t.d_counts & 3u)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": d_offsets must be 8-byte and d_counts 4-byte aligned"};
    }
    if (n_tasks >= ((size_t)1 << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, "scan: too many tasks for one call"};
    if (n_tasks == 0) return PcoSuccess;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) throw HostError{PCO_GFX_DEVICE_ERROR, "libpco_gfx: no MI355X/HIP device visible; this library has no CPU fallback"};
    { WorkspaceUse use(workspace(), (hipStream_t)stream); launch_scan(n_tasks, tasks, results, d_results, (hipStream_t)stream); }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "scan task " + std::to_string(i) + " failed behind " + std::to_string(results[i].n_out) + " chunks");
      return PcoDecompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { set_error(e.status, e.msg); return PcoDecompressionError; }
}
