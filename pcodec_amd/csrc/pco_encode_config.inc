// pco_encode_config.inc -- the encode configuration (included by pco_gfx.hip): PcoChunkConfigEx resolved and validated, the plans of explicit specs.
namespace pcogfx {

struct ResolvedConfig {
  uint32_t level;
  uint32_t mode_kind; double mode_f64; uint64_t mode_u64;
  uint32_t delta_kind, delta_order;
  uint64_t max_page_n; bool enable_8_bit;
  bool strict_hist;   // PCO_GFX_CFG_STRICT_HISTOGRAM: enc_hist_literal_kernel replays the reference's quickselect behind the fast histograms
  bool conv1 = false;           // PCO_GFX_CFG_CONV1: DeltaSpec::TryConv1 is encoded (encode_conv1.hip) instead of refused
  bool dict = false;            // PCO_GFX_CFG_DICT: ModeSpec::TryDict is encoded (encode_dict.hip) instead of refused
  bool verify = false;          // PCO_GFX_CFG_VERIFY: every chunk is decoded again behind the encode and compared with its source (pco_verify_host.inc)
  DictTask* d_dict = nullptr;   // the final encode of a Dict call: the dictionaries build_dicts made (the chunks are u32 index chunks by then)
  uint32_t unknown_flags = 0;   // bits of PcoChunkConfigEx::flags this library does not know (rejected by validate_config)
};

// PCO_GFX_STRICT_HISTOGRAM=1 in the environment turns the strict histogram on for every call (the reference's own three-function C ABI has no
// field for it)
// (a plain function, and not a const variable: a namespace-scope `static const bool x = [] { ... }();` in this translation unit was compiled
//  with ANOTHER lambda's body -- g_decode_trail's, which made every call strict; hipcc numbers host and device lambdas differently there)
static bool g_strict_hist_env = env_is_one("PCO_GFX_STRICT_HISTOGRAM");
// PCO_GFX_VERIFY=1 likewise turns the verified encode on for every call
static bool g_verify_env = env_is_one("PCO_GFX_VERIFY");
static ResolvedConfig resolve_config(const PcoChunkConfigEx* c) {
  ResolvedConfig r{8, PCO_MODE_AUTO, 0.0, 0, PCO_DELTA_AUTO, 0, 1u << 18, true, g_strict_hist_env};
  r.verify = g_verify_env;
  if (c) {
    r.level = c->compression_level; r.mode_kind = c->mode_kind; r.mode_f64 = c->mode_f64; r.mode_u64 = c->mode_u64;
    r.delta_kind = c->delta_kind; r.delta_order = c->delta_order; r.max_page_n = c->max_page_n ? c->max_page_n : (1u << 18);
    r.enable_8_bit = c->enable_8_bit != 0;
    r.strict_hist = g_strict_hist_env || (c->flags & PCO_GFX_CFG_STRICT_HISTOGRAM) != 0;
    r.conv1 = (c->flags & PCO_GFX_CFG_CONV1) != 0;
    r.dict = (c->flags & PCO_GFX_CFG_DICT) != 0;
    r.verify = g_verify_env || (c->flags & PCO_GFX_CFG_VERIFY) != 0;
    r.unknown_flags = c->flags & ~(uint32_t)(PCO_GFX_CFG_STRICT_HISTOGRAM | PCO_GFX_CFG_CONV1 | PCO_GFX_CFG_DICT | PCO_GFX_CFG_VERIFY);
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
static void validate_task(const PcoGfxEncodeTask& t, const ResolvedConfig& cfg, bool device_dst) {
  const int bits = dtype_bits(t.dtype);
  if (!bits) throw HostError{PCO_GFX_INVALID_ARGUMENT, "invalid dtype"};
  validate_config(cfg, bits);
  if (t.n == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot compress empty chunk"};
  if (t.n > kMaxEntries) throw HostError{PCO_GFX_INVALID_ARGUMENT, "count may not exceed 2^24 per chunk"};
  if ((device_dst && ((uintptr_t)t.dst & 7)) || ((uintptr_t)t.src & (bits / 8 - 1))) throw HostError{PCO_GFX_INVALID_ARGUMENT, "dst must be 8-byte aligned and src naturally aligned"};
}

}  // namespace pcogfx
