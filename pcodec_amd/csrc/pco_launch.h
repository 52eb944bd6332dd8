// pco_launch.h -- what the host drivers of both translation units (pco_gfx.hip, pco_gfx_ranges.hip) launch kernels with: the timed launch, the
// dynamic-LDS reservation, the width dispatch, the placement of a call's device arrays and the scratch budget.  Host code only; include it
// behind the kernels.
#pragma once
#include "pco_host.h"
#include "pco_dev.h"

namespace pcogfx {

// ---- timing (pco_gfx_profile_begin / _end) ----
// The span's first event is recorded here (pco_gfx.hip, which owns the per-thread profile); its last -- returned, null when timing is off -- by
// the caller once the launches are made.
hipEvent_t profile_span_begin(const char* name, hipStream_t stream);
struct TimedSpan {   // RAII: what is launched on `stream` in its scope is reported under `name`
  hipStream_t s; hipEvent_t b;
  TimedSpan(const char* name, hipStream_t stream) : s(stream), b(profile_span_begin(name, stream)) {}
  ~TimedSpan() { if (b) (void)hipEventRecord(b, s); }
  TimedSpan(const TimedSpan&) = delete;
  TimedSpan& operator=(const TimedSpan&) = delete;
};
#define PCO_TIMED_LAUNCH(name, stream, ...) do { pcogfx::TimedSpan _t(name, stream); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// ---- dynamic LDS beyond the default limit ----
// Once per process and use site (a function-local static; in a template, one per instantiation); a kernel with a comma in its name goes in
// parentheses.  Several kernels reserved under one name fail with one message.
#define PCO_RESERVE_LDS(kernel, bytes, name)                                                                                                       \
  do {                                                                                                                                             \
    static const bool _lds_ok = hipFuncSetAttribute((const void*)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)) == hipSuccess; \
    if (!_lds_ok) throw pcogfx::HostError{PCO_GFX_DEVICE_ERROR, std::string("cannot reserve LDS for ") + (name)};                                  \
  } while (0)

// ---- number widths ----
inline int width_group(uint32_t dtype) { const int b = dtype_bits(dtype); return b == 64 ? 0 : (b == 32 ? 1 : (b == 16 ? 2 : (b == 8 ? 3 : -1))); }

// The one place a width group becomes a number type.  (A named template and steps with a member template, not a generic lambda around the
// launches: pco_host.h, env_is_one.)
template <class Step>
void launch_width(int g, const Step& step) {
  switch (g) {
    case 0: step.template launch<uint64_t>(); break;
    case 1: step.template launch<uint32_t>(); break;
    case 2: step.template launch<uint16_t>(); break;
    default: step.template launch<uint8_t>(); break;
  }
}

// task ids by width group -> one list, group g at [off[g], off[g + 1])
inline void flatten_groups(const std::vector<uint32_t> (&ids)[4], std::vector<uint32_t>& flat, size_t (&off)[5]) {
  for (int g = 0; g < 4; g++) { off[g] = flat.size(); flat.insert(flat.end(), ids[g].begin(), ids[g].end()); }
  off[4] = flat.size();
}

// the device arrays of a call, side by side in one buffer, each 16-byte aligned
struct Layout {
  size_t end = 0;
  size_t place(size_t bytes) { const size_t at = (end + 15) & ~(size_t)15; end = at + bytes; return at; }
};

// ---- scratch budget ----
// What the scratch of one call (or pass) may take: PCO_GFX_WORKSPACE_GB, else 80 % of the device memory that is free plus `held`, what the
// caller's buffers hold already.  `env` is the variable as the caller read it -- the encode side once per process, the partial-page side at
// every call (a test narrows it in mid-process).
inline size_t scratch_budget_bytes(const char* env, size_t held) {
  if (env && *env) return (size_t)(std::atof(env) * 1e9);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return ~(size_t)0;
  return (size_t)((free_b + held) * 0.8);
}

}  // namespace pcogfx
