// pco_encode_specs.inc -- PcoGfxChunkSpec (header section 3c; included by pco_gfx.hip behind pco_encode_config.inc): a chunk's resolved mode and
// delta as a value the caller keeps -- the conversion EncModePlan <-> spec, a spec's validation, the config a specs call may carry.  Host arithmetic only.
namespace pcogfx {

// What resolve_plans left in a plan, as a spec.  Lossless: window_n_log is lookback_window_log(n), state_n_log is 0, ubl_override belongs to the
// level, the paging fields to the launcher; FloatMult's ordered-latent base is a function of its bit pattern.
static PcoGfxChunkSpec spec_from_plan(const EncModePlan& p) {
  PcoGfxChunkSpec s{};
  switch (p.mode_kind) {
    case kClassic: s.mode_kind = PCO_MODE_CLASSIC; break;
    case kIntMult: s.mode_kind = PCO_MODE_TRY_INT_MULT; s.mode_base = p.mode_base; break;
    case kFloatMult: s.mode_kind = PCO_MODE_TRY_FLOAT_MULT; s.mode_base = p.mode_aux2; s.mode_inv = p.mode_aux; break;
    case kFloatQuant: s.mode_kind = PCO_MODE_TRY_FLOAT_QUANT; s.mode_k = p.mode_k; break;
    default: throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot carry a dictionary"};
  }
  switch (p.delta_kind) {
    case kDeltaNone: s.delta_kind = PCO_DELTA_NOOP; break;
    case kDeltaConsecutive: s.delta_kind = PCO_DELTA_TRY_CONSECUTIVE; s.delta_order = p.delta_order; break;
    case kDeltaLookback: s.delta_kind = PCO_DELTA_TRY_LOOKBACK; break;
    default: throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot carry a Conv1 fit"};
  }
  return s;
}

// The FloatMult base of a spec (a bit pattern in the number type) as the double ResolvedConfig::mode_f64 holds: exact for every finite base, so
// plan_mode_explicit's cast gives the pattern back
static double spec_base_as_f64(uint64_t pattern, int bits) {
  if (bits == 64) { double d; std::memcpy(&d, &pattern, 8); return d; }
  if (bits == 32) { const uint32_t b = (uint32_t)pattern; float f; std::memcpy(&f, &b, 4); return (double)f; }
  return (double)F16::raw((uint16_t)pattern).to_f32();
}

// The explicit ResolvedConfig a spec expresses (mode and delta only)
static ResolvedConfig config_of_spec(const PcoGfxChunkSpec& s, uint32_t dtype) {
  ResolvedConfig c{};
  c.mode_kind = s.mode_kind; c.delta_kind = s.delta_kind; c.delta_order = s.delta_order;
  if (s.mode_kind == PCO_MODE_TRY_INT_MULT) c.mode_u64 = s.mode_base;
  else if (s.mode_kind == PCO_MODE_TRY_FLOAT_QUANT) c.mode_u64 = s.mode_k;
  else if (s.mode_kind == PCO_MODE_TRY_FLOAT_MULT) c.mode_f64 = spec_base_as_f64(s.mode_base, dtype_bits(dtype));
  return c;
}

// One spec against its task's number type, in the order section 3c documents; every message names the task
static void validate_spec(size_t i, const PcoGfxChunkSpec& s, uint32_t dtype) {
  const std::string who = "chunk spec " + std::to_string(i) + ": ";
  const int bits = dtype_bits(dtype);
  if (!bits) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "invalid dtype"};
  const uint32_t kind = dtype_kind(dtype);
  const bool mode_ok = s.mode_kind == PCO_MODE_CLASSIC || s.mode_kind == PCO_MODE_TRY_INT_MULT || s.mode_kind == PCO_MODE_TRY_FLOAT_MULT || s.mode_kind == PCO_MODE_TRY_FLOAT_QUANT;
  const bool delta_ok = s.delta_kind == PCO_DELTA_NOOP || s.delta_kind == PCO_DELTA_TRY_CONSECUTIVE || s.delta_kind == PCO_DELTA_TRY_LOOKBACK;
  if (!mode_ok) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "mode_kind must be Classic, TryIntMult, TryFloatMult or TryFloatQuant (a spec is a resolved mode: never Auto, Dict or unknown)"};
  if (!delta_ok) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "delta_kind must be NoOp, TryConsecutive or TryLookback (a spec is a resolved delta: never Auto, Conv1 or unknown)"};
  if (s.mode_kind == PCO_MODE_TRY_INT_MULT && kind == kFloat) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "unable to use int mult mode on floats"};
  if ((s.mode_kind == PCO_MODE_TRY_FLOAT_MULT || s.mode_kind == PCO_MODE_TRY_FLOAT_QUANT) && kind != kFloat) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "unable to use float mode for ints"};
  const uint64_t width_mask = bits == 64 ? ~0ull : ((1ull << bits) - 1);
  if (s.mode_kind == PCO_MODE_TRY_INT_MULT && (s.mode_base & width_mask) == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "The chosen mode was invalid for the number type (an int mult base of 0)"};
  if (s.mode_kind == PCO_MODE_TRY_FLOAT_MULT) {   // the base: a finite non-zero bit pattern of the number type
    const int mant = bits == 64 ? 52 : (bits == 32 ? 23 : 10);
    const uint64_t exp_mask = (width_mask >> 1) & ~((1ull << mant) - 1);
    if ((s.mode_base & ~width_mask) || (s.mode_inv & ~width_mask) || (s.mode_base & exp_mask) == exp_mask || (s.mode_base & (width_mask >> 1)) == 0)
      throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "The chosen mode was invalid for the number type (a float mult base must be a finite non-zero bit pattern of the number type)"};
  }
  if (s.mode_kind == PCO_MODE_TRY_FLOAT_QUANT) {
    const uint32_t prec = bits == 64 ? 52 : (bits == 32 ? 23 : 10);
    if (s.mode_k == 0 || s.mode_k > prec) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "The chosen mode was invalid for the number type (a float quant k outside 1..precision)"};
  }
  if (s.delta_kind == PCO_DELTA_TRY_CONSECUTIVE && (s.delta_order == 0 || s.delta_order > 7)) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "consecutive delta order must be 1..7"};
  if (s.reserved != 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "reserved must be 0"};
  if (s.mode_inv != 0 && s.mode_kind != PCO_MODE_TRY_FLOAT_MULT) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + "mode_inv belongs to TryFloatMult and must be 0 otherwise"};
}

// The plan of a validated spec: plan_mode_explicit / plan_delta_explicit under the config the spec expresses, and the inverse the spec carries
// in place of 1 / base when it carries one
static void plan_from_spec(EncModePlan& p, const PcoGfxChunkSpec& s, uint32_t dtype, uint64_t n) {
  p = EncModePlan{};
  const ResolvedConfig c = config_of_spec(s, dtype);
  plan_mode_explicit(p, c, dtype);
  plan_delta_explicit(p, c, n);
  if (s.mode_kind == PCO_MODE_TRY_FLOAT_MULT && s.mode_inv != 0) p.mode_aux = s.mode_inv;
}

// The config beside a spec array: level, paging, enable_8_bit and the flags that are not a mode.  Its own mode and delta must be Auto -- a spec is
// never silently overridden -- and a spec cannot carry what the CONV1 and DICT bits turn on.
static ResolvedConfig resolve_specs_config(const PcoChunkConfigEx* config) {
  const ResolvedConfig cfg = resolve_config(config);
  if (cfg.mode_kind != PCO_MODE_AUTO || cfg.delta_kind != PCO_DELTA_AUTO) throw HostError{PCO_GFX_INVALID_ARGUMENT, "a specs call takes mode and delta from its specs: config->mode_kind and config->delta_kind must be Auto (0)"};
  if (cfg.conv1 || cfg.dict) throw HostError{PCO_GFX_INVALID_ARGUMENT, "a specs call cannot carry PCO_GFX_CFG_CONV1 or PCO_GFX_CFG_DICT: a spec holds neither a fit nor a dictionary"};
  return cfg;
}

// The ready plans of a specs call, every spec checked: before a device is asked for
template <class Task>   // (PcoGfxEncodeTask or PcoGfxWrappedTask)
static void plans_from_specs(size_t n_tasks, const Task* tasks, const PcoGfxChunkSpec* specs, std::vector<EncModePlan>& plans) {
  plans.resize(n_tasks);
  for (size_t i = 0; i < n_tasks; i++) { validate_spec(i, specs[i], tasks[i].dtype); plan_from_spec(plans[i], specs[i], tasks[i].dtype, tasks[i].n); }
}

// What encode_in_passes plans a specs call's scratch with: the shape of its specs, not Auto's worst case
static ResolvedConfig footprint_config(const ResolvedConfig& cfg, const std::vector<EncModePlan>& plans) {
  ResolvedConfig f = cfg; bool two = false, lookback = false;
  for (const EncModePlan& p : plans) { two |= p.mode_kind != kClassic; lookback |= p.delta_kind == kDeltaLookback; }
  f.mode_kind = two ? PCO_MODE_TRY_INT_MULT : PCO_MODE_CLASSIC; f.delta_kind = lookback ? PCO_DELTA_TRY_LOOKBACK : PCO_DELTA_NOOP;
  return f;
}
static const uint64_t kSpecsKeySalt = 1ull << 15;   // (encode_in_passes' spec_key: bit 15 is nobody else's)

}  // namespace pcogfx
