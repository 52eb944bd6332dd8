// pco_encode_specs_entry.inc -- the extern "C" entry points of header section 3c (included by pco_gfx.hip, behind pco_encode_entry.inc): resolve a
// call's Auto specs once, build a spec from a ChunkMeta, encode later calls from a per-chunk spec array.  No kernel of its own: the encode is
// launch_encode / launch_encode_wrapped with the plans ready.
extern "C" {

enum PcoError pco_gfx_resolve_chunk_specs(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config, PcoGfxChunkSpec* specs, void* stream_) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null tasks"};
    if (n_tasks && !specs) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null specs"};
    const ResolvedConfig cfg = resolve_config(config);
    if (cfg.mode_kind == PCO_MODE_TRY_DICT) throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot carry a dictionary (ModeSpec::TryDict)"};
    if (cfg.delta_kind == PCO_DELTA_TRY_CONV1) throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot carry a Conv1 fit (DeltaSpec::TryConv1)"};
    // the encode's own validation; dst and dst_cap are not the resolution's business
    std::vector<PcoGfxEncodeTask> rt(n_tasks);
    for (size_t i = 0; i < n_tasks; i++) { rt[i] = PcoGfxEncodeTask{tasks[i].src, tasks[i].n, nullptr, 0, tasks[i].dtype, 0}; validate_task(rt[i], cfg, true); }
    std::vector<EncModePlan> plans(n_tasks);
    if (cfg.mode_kind != PCO_MODE_AUTO && cfg.delta_kind != PCO_DELTA_AUTO) {   // both explicit: host arithmetic, no device
      for (size_t i = 0; i < n_tasks; i++) { plans[i] = EncModePlan{}; plan_mode_explicit(plans[i], cfg, rt[i].dtype); plan_delta_explicit(plans[i], cfg, rt[i].n); }
    } else if (n_tasks) {
      require_device();
      hipStream_t stream = (hipStream_t)stream_;
      WorkspaceUse use(workspace(), stream);
      TracePhase tp("resolve_plans (total)", stream);
      resolve_plans(n_tasks, rt.data(), cfg, plans, stream);
      PCO_HIP_CHECK(hipStreamSynchronize(stream));   // (synchronous whatever the resolution launched last)
    }
    for (size_t i = 0; i < n_tasks; i++) specs[i] = spec_from_plan(plans[i]);
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

enum PcoError pco_gfx_chunk_spec_from_meta(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, PcoGfxChunkSpec* spec) {
  if (!spec) { clear_error(); set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_spec_from_meta: null spec"); return PcoInvalidType; }
  PcoGfxChunkMetaInfo mi;
  const enum PcoError e = pco_gfx_chunk_meta_info(meta, len, dtype, format_major, &mi);
  if (e != PcoSuccess) return e;
  try {
    if (mi.mode_kind == kDict) throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot carry a dictionary (Dict mode)"};
    if (mi.delta_kind == kDeltaConv1) throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot carry a Conv1 fit"};
    if (mi.secondary_uses_delta) throw HostError{PCO_GFX_UNSUPPORTED, "a chunk spec cannot say secondary_uses_delta (no ModeSpec / DeltaSpec writes it)"};
    EncModePlan p{};
    p.mode_kind = mi.mode_kind; p.mode_k = mi.mode_k; p.mode_base = mi.mode_base_latent;
    p.delta_kind = mi.delta_kind; p.delta_order = mi.delta_order;
    if (mi.mode_kind == kFloatMult) {   // the base's bit pattern from its ordered latent (to_latent_ordered's inverse); the inverse is not in the metadata
      const int bits = dtype_bits(dtype);
      const uint64_t mask = bits == 64 ? ~0ull : ((1ull << bits) - 1), top = 1ull << (bits - 1);
      p.mode_aux2 = (mi.mode_base_latent & top) ? (mi.mode_base_latent ^ top) : (~mi.mode_base_latent & mask);
      p.mode_aux = 0;
    }
    *spec = spec_from_plan(p);
    return PcoSuccess;
  } catch (const HostError& he) { return fail_with(he, PcoCompressionError); }
}

enum PcoError pco_gfx_compress_chunks_specs(size_t n_tasks, const PcoGfxEncodeTask* tasks, const PcoChunkConfigEx* config, const PcoGfxChunkSpec* specs,
                                            PcoGfxTaskResult* results, PcoGfxTaskResult* d_results, void* stream) {
  clear_error();
  try {
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null tasks"};
    if (n_tasks && !specs) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null specs"};
    const ResolvedConfig cfg = resolve_specs_config(config);
    std::vector<EncModePlan> plans;
    plans_from_specs(n_tasks, tasks, specs, plans);
    const ResolvedConfig fcfg = footprint_config(cfg, plans);
    require_device();
    {
      WorkspaceUse use(workspace(), (hipStream_t)stream);
      TracePhase tp_all("compress_chunks_specs (total)", (hipStream_t)stream);
      encode_in_sub_batches(n_tasks, tasks, cfg, results, d_results, (hipStream_t)stream, plans.data(), &fcfg);
    }
    if (results) for (size_t i = 0; i < n_tasks; i++) if (results[i].status != PCO_GFX_OK) {
      set_error((int)results[i].status, "encode task " + std::to_string(i) + " failed");
      return PcoCompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

enum PcoError pco_gfx_compress_wrapped_chunks_specs(size_t n_tasks, const PcoGfxWrappedTask* tasks, const PcoChunkConfigEx* config, const PcoGfxChunkSpec* specs,
                                                    PcoGfxPageInfo* infos, PcoGfxPageInfo* d_infos, void* stream) {
  clear_error();
  try {
    if (!infos && !d_infos) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null infos and d_infos"};
    if (n_tasks && !tasks) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null tasks"};
    if (n_tasks && !specs) throw HostError{PCO_GFX_INVALID_ARGUMENT, "null specs"};
    const ResolvedConfig cfg = resolve_specs_config(config);
    std::vector<EncModePlan> plans;
    plans_from_specs(n_tasks, tasks, specs, plans);
    const ResolvedConfig fcfg = footprint_config(cfg, plans);
    require_device();
    WrappedPaging pg;
    plan_wrapped_paging(n_tasks, tasks, cfg, pg);
    const size_t n_infos = pg.sizes.size() + n_tasks;
    {
      WorkspaceUse use(workspace(), (hipStream_t)stream);
      encode_wrapped_in_passes(n_tasks, tasks, pg, cfg, infos, d_infos, (hipStream_t)stream, plans.data(), &fcfg);
    }
    if (infos) for (size_t k = 0; k < n_infos; k++) if (infos[k].status != PCO_GFX_OK) {
      set_error((int)infos[k].status, "wrapped encode: piece " + std::to_string(k) + " failed");
      return PcoCompressionError;
    }
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}

}  // extern "C"
