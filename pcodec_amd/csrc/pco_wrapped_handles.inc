// pco_wrapped_handles.inc -- the wrapped surface on host buffers (included by pco_gfx.hip): pco_chunk_compressor_* / pco_chunk_decompressor_* /
// pco_page_decompressor_* handles.
struct PcoGfxChunkCompressor {
  std::vector<uint8_t> meta;
  std::vector<std::vector<uint8_t>> pages;
  std::vector<size_t> page_n;
  size_t meta_size_hint = 0;
  std::vector<size_t> page_size_hints;
};
struct PcoGfxChunkDecompressor {
  std::vector<uint8_t> meta;
  uint8_t dtype = 0, format_major = 4;
};
struct PcoGfxPageDecompressor {
  std::vector<uint8_t> nums;   // the decoded page (host)
  size_t elem = 0, n = 0, pos = 0, consumed = 0;
  size_t n_ok = 0; int bad_status = 0;   // a page that failed inside its body: the numbers of the batches before the failing one, and the error the call that reaches it gets
};

namespace pcogfx {

static PcoGfxChunkCompressor* chunk_compressor_build(const void* nums, size_t n, unsigned char dtype, const ResolvedConfig& cfg, const size_t* exact_pages = nullptr, size_t n_exact = 0) {
  const int bits = dtype_bits(dtype);
  if (!bits) throw HostError{PCO_GFX_INVALID_ARGUMENT, "invalid dtype"};
  const size_t esz = (size_t)bits / 8;
  require_device();
  Workspace& wsp = workspace();
  WorkspaceUse use(wsp, 0);
  std::vector<size_t> pn;
  if (exact_pages) {   // PagingSpec::Exact (chunk_config.rs:162-180)
    pn.assign(exact_pages, exact_pages + n_exact);
    size_t sum = 0; for (size_t x : pn) sum += x;
    if (sum != n) throw HostError{PCO_GFX_INVALID_ARGUMENT, "paging spec suggests " + std::to_string(sum) + " numbers but " + std::to_string(n) + " were given"};
    for (size_t x : pn) if (x == 0) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot write data page of 0 numbers"};
  } else n_per_page(cfg.max_page_n, n, pn);
  if (pn.empty()) throw HostError{PCO_GFX_INVALID_ARGUMENT, "cannot compress empty chunk"};
  uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(n * esz + 64);
  PCO_HIP_CHECK(hipMemcpyAsync(d_in, nums, n * esz, hipMemcpyHostToDevice, 0));
  PcoGfxEncodeTask task{d_in, n, nullptr, 0, dtype, 0};
  validate_task(task, cfg, false);
  std::vector<EncModePlan> plans(1);
  std::vector<PcoGfxEncodeTask> vt; ResolvedConfig ecfg = cfg; DictTask* d_dict = nullptr;
  if (cfg.mode_kind == PCO_MODE_TRY_DICT) { d_dict = build_dicts(1, &task, true, 0, vt, ecfg); task = vt[0]; }
  resolve_plans(1, &task, ecfg, plans, 0);
  ecfg.d_dict = d_dict;
  plans[0].n_pages = (uint32_t)pn.size(); plans[0].page_low = (uint32_t)(n / pn.size()); plans[0].page_r = (uint32_t)(n % pn.size()); plans[0].page_first = 1;
  plans[0].exact_paging = exact_pages ? 1u : 0u;
  const size_t meta_cap = chunk_meta_cap(cfg, bits, n);
  std::vector<size_t> offs(pn.size() + 1); size_t total = meta_cap;
  for (size_t i = 0; i < pn.size(); i++) { offs[i] = total; total += chunk_page_cap(cfg, bits, pn[i]); }
  offs[pn.size()] = total;
  uint8_t* d_out = (uint8_t*)wsp.io_out.ensure(total);
  std::vector<EncPage> pages(pn.size() + 1);
  { EncPage p{}; p.chunk = 0; p.n = 0; p.dst = d_out; p.dst_cap = meta_cap; p.flags = kPageFlagMetaOnly; pages[0] = p; }
  size_t start = 0;
  for (size_t i = 0; i < pn.size(); i++) {
    EncPage p{}; p.chunk = 0; p.page_idx = (uint32_t)i; p.start = start; p.n = pn[i]; p.dst = d_out + offs[i]; p.dst_cap = offs[i + 1] - offs[i]; p.flags = 0;
    pages[i + 1] = p; start += pn[i];
  }
  std::vector<PcoGfxTaskResult> res(pages.size());
  EncWorkspace ws{};
  run_encode(1, &task, plans, pages, ecfg, res.data(), nullptr, 0, &ws);
  for (auto& r : res) if (r.status != PCO_GFX_OK) throw HostError{(int)r.status, "chunk failed to compress"};
  std::unique_ptr<PcoGfxChunkCompressor> cc(new PcoGfxChunkCompressor());
  cc->meta.resize(res[0].n_out);
  PCO_HIP_CHECK(hipMemcpy(cc->meta.data(), d_out, res[0].n_out, hipMemcpyDeviceToHost));
  cc->page_n = pn;
  for (size_t i = 0; i < pn.size(); i++) {
    cc->pages.emplace_back(res[i + 1].n_out);
    PCO_HIP_CHECK(hipMemcpy(cc->pages.back().data(), d_out + offs[i], res[i + 1].n_out, hipMemcpyDeviceToHost));
  }
  // size hints (metadata/chunk.rs:105-125, metadata/bins.rs:23-32, wrapped/chunk_compressor.rs:556-621): host arithmetic on the trained plan
  EncChunk ch; PCO_HIP_CHECK(hipMemcpy(&ch, ws.chunks, sizeof(EncChunk), hipMemcpyDeviceToHost));
  // the three plan regions of the chunk (PlanRef layout): only the optimized bins' weights and offset bits are needed here
  const size_t pbytes = plan_bytes_for(ws.plan_cap);
  std::vector<uint8_t> pv_raw(3 * pbytes);
  PCO_HIP_CHECK(hipMemcpy(pv_raw.data(), ws.plans, 3 * pbytes, hipMemcpyDeviceToHost));
  struct HostPlan { const uint32_t* bweight; const uint8_t* bob; } pv[3];
  for (int v = 0; v < 3; v++) { const uint8_t* b = pv_raw.data() + v * pbytes; pv[v].bweight = (const uint32_t*)(b + 28ull * ws.plan_cap); pv[v].bob = b + 40ull * ws.plan_cap + (2ull << kMaxEncTableLog); }
  const bool fb = ch.fallback != 0;
  size_t meta_bits = kBitsModeVariant + (4 + 5 + 5 + 64 + 32 * 32);
  if (!fb) meta_bits += (ch.mode_kind == kIntMult || ch.mode_kind == kFloatMult) ? (size_t)bits : (ch.mode_kind == kFloatQuant ? kBitsQuantK : 0);
  if (!fb && ch.dict_dtype) meta_bits += kBitsDictLen + 7 + (size_t)ch.dict_k * bits;   // Mode::Dict (metadata/mode.rs:219-229)
  size_t page_meta_bits = 0; double avg[3] = {0, 0, 0}; uint32_t nlps[3] = {0, 0, 0};
  for (int v = 0; v < 3; v++) {
    const bool present = fb ? v == 1 : ch.v[v].present != 0;
    if (!present) continue;
    const uint32_t lb = fb ? (uint32_t)bits : ch.v[v].latent_bits, asl = fb ? 0 : ch.v[v].ans_size_log, nb = fb ? 1 : ch.v[v].n_bins;
    meta_bits += kBitsAnsSizeLog + kBitsNBins + (size_t)nb * (asl + lb + offset_bits_bits(lb));
    if (!fb && v == 1) nlps[v] = (ch.delta_kind == kDeltaConsecutive || ch.delta_kind == kDeltaConv1) ? ch.delta_order : (ch.delta_kind == kDeltaLookback ? (1u << ch.state_n_log) : 0u);
    page_meta_bits += (size_t)asl * 4 + (size_t)lb * nlps[v];
    if (fb) avg[v] = (double)bits;
    else {
      const double tw = (double)(1ull << asl);
      for (uint32_t b = 0; b < nb; b++) {
        const double w = (double)pv[v].bweight[b];
        avg[v] += ((double)asl - std::log2(w) + (double)pv[v].bob[b]) * w / tw;
      }
    }
  }
  cc->meta_size_hint = (meta_bits + 7) / 8;
  for (size_t i = 0; i < pn.size(); i++) {
    size_t body_bits = 0;
    for (int v = 0; v < 3; v++) {
      const bool present = fb ? v == 1 : ch.v[v].present != 0;
      if (!present) continue;
      const size_t stored = v == 2 ? pn[i] : (pn[i] > nlps[1] ? pn[i] - nlps[1] : 0);
      body_bits += (size_t)std::ceil((double)stored * avg[v] * 1.2);
    }
    cc->page_size_hints.push_back((page_meta_bits + 7) / 8 + (body_bits + 7) / 8);
  }
  return cc.release();
}

}  // namespace pcogfx

extern "C" {

enum PcoError pco_chunk_compressor_new(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config, PcoGfxChunkCompressor** out) {
  clear_error();
  if (!dtype_bits(dtype)) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try { *out = chunk_compressor_build(nums, n, dtype, resolve_config(config)); return PcoSuccess; }
  catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}
enum PcoError pco_chunk_compressor_new_exact(const void* nums, size_t n, unsigned char dtype, const PcoChunkConfigEx* config, const size_t* page_sizes,
                                             size_t n_pages, PcoGfxChunkCompressor** out) {
  clear_error();
  if (!dtype_bits(dtype)) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    if (!page_sizes) throw HostError{PCO_GFX_INVALID_ARGUMENT, "page_sizes is null"};
    static const size_t none = 0;
    *out = chunk_compressor_build(nums, n, dtype, resolve_config(config), n_pages ? page_sizes : &none, n_pages); return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoCompressionError); }
}
size_t pco_chunk_compressor_meta_size(const PcoGfxChunkCompressor* cc) { return cc->meta.size(); }
size_t pco_chunk_compressor_page_size(const PcoGfxChunkCompressor* cc, size_t i) { return i < cc->pages.size() ? cc->pages[i].size() : 0; }
size_t pco_chunk_compressor_n_pages(const PcoGfxChunkCompressor* cc) { return cc->pages.size(); }
size_t pco_chunk_compressor_page_n(const PcoGfxChunkCompressor* cc, size_t i) { return i < cc->page_n.size() ? cc->page_n[i] : 0; }
size_t pco_chunk_compressor_meta_size_hint(const PcoGfxChunkCompressor* cc) { return cc->meta_size_hint; }
size_t pco_chunk_compressor_page_size_hint(const PcoGfxChunkCompressor* cc, size_t i) { return i < cc->page_size_hints.size() ? cc->page_size_hints[i] : 0; }
enum PcoError pco_chunk_compressor_write_meta(const PcoGfxChunkCompressor* cc, void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  if (cc->meta.size() > dst_cap) { set_error(PCO_GFX_INVALID_ARGUMENT, "destination too small"); return PcoCompressionError; }
  std::memcpy(dst, cc->meta.data(), cc->meta.size()); if (n_written) *n_written = cc->meta.size();
  return PcoSuccess;
}
enum PcoError pco_chunk_compressor_write_page(const PcoGfxChunkCompressor* cc, size_t page_idx, void* dst, size_t dst_cap, size_t* n_written) {
  clear_error();
  if (page_idx >= cc->pages.size()) { set_error(PCO_GFX_INVALID_ARGUMENT, "page idx exceeds num pages"); return PcoCompressionError; }
  const auto& p = cc->pages[page_idx];
  if (p.size() > dst_cap) { set_error(PCO_GFX_INVALID_ARGUMENT, "destination too small"); return PcoCompressionError; }
  std::memcpy(dst, p.data(), p.size()); if (n_written) *n_written = p.size();
  return PcoSuccess;
}
void pco_chunk_compressor_free(PcoGfxChunkCompressor* cc) { delete cc; }

enum PcoError pco_chunk_decompressor_new(const void* src, size_t len, unsigned char dtype, uint8_t format_major,
                                         PcoGfxChunkDecompressor** out, size_t* consumed) {
  clear_error();
  const int bits = dtype_bits(dtype);
  if (!bits) { set_error(PCO_GFX_INVALID_ARGUMENT, "invalid dtype"); return PcoInvalidType; }
  try {
    require_device();
    Workspace& wsp = workspace();
    WorkspaceUse use(wsp, 0);
    uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(len + 64);
    PCO_HIP_CHECK(hipMemsetAsync(d_in + len, 0, 64, 0));
    if (len) PCO_HIP_CHECK(hipMemcpyAsync(d_in, src, len, hipMemcpyHostToDevice, 0));
    PcoGfxDecodeTask task{d_in, len, nullptr, 0, dtype, PCO_GFX_TASK_META_ONLY | ((uint32_t)format_major << 8)};
    PcoGfxTaskResult res{};
    launch_decode(1, &task, &res, nullptr, 0);
    if (res.status != PCO_GFX_OK) { set_error((int)res.status, "invalid chunk metadata"); return PcoDecompressionError; }
    auto* cd = new PcoGfxChunkDecompressor();
    cd->meta.assign((const uint8_t*)src, (const uint8_t*)src + res.consumed); cd->dtype = dtype; cd->format_major = format_major;
    *out = cd; if (consumed) *consumed = res.consumed;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}
static enum PcoError read_page_impl(PcoGfxChunkDecompressor* cd, const void* src, size_t len, size_t page_n, void* dst,
                                    size_t dst_cap, size_t* n_processed, size_t* consumed, int* partial_ok) {
  clear_error();
  try {
    if (dst_cap < page_n) throw HostError{PCO_GFX_INVALID_ARGUMENT, "dst must hold the whole page"};
    require_device();
    Workspace& wsp = workspace();
    WorkspaceUse use(wsp, 0);
    const int bits = dtype_bits(cd->dtype);
    const size_t ml = cd->meta.size();
    uint8_t* d_in = (uint8_t*)wsp.io_in.ensure(ml + len + 64);
    uint8_t* d_out = (uint8_t*)wsp.io_out.ensure(page_n * (size_t)(bits / 8) + 64);
    PCO_HIP_CHECK(hipMemsetAsync(d_in + ml + len, 0, 64, 0));
    PCO_HIP_CHECK(hipMemcpyAsync(d_in, cd->meta.data(), ml, hipMemcpyHostToDevice, 0));
    if (len) PCO_HIP_CHECK(hipMemcpyAsync(d_in + ml, src, len, hipMemcpyHostToDevice, 0));
    PcoGfxDecodeTask task{d_in, ml + len, d_out, page_n, cd->dtype, PCO_GFX_TASK_WRAPPED_PAGE | ((uint32_t)cd->format_major << 8)};
    PcoGfxTaskResult res{};
    launch_decode(1, &task, &res, nullptr, 0);
    if (res.status != PCO_GFX_OK) {
      // (internal use by pco_page_decompressor_new, which passes partial_ok: the batches in front of the failing one are copied out anyway)
      if (partial_ok && (res.aux & 1u)) {
        if (res.n_out) PCO_HIP_CHECK(hipMemcpy(dst, d_out, res.n_out * (size_t)(bits / 8), hipMemcpyDeviceToHost));
        *partial_ok = 1; if (n_processed) *n_processed = res.n_out;
      }
      set_error((int)res.status, "page failed to decompress"); return PcoDecompressionError;
    }
    PCO_HIP_CHECK(hipMemcpy(dst, d_out, page_n * (size_t)(bits / 8), hipMemcpyDeviceToHost));
    if (n_processed) *n_processed = res.n_out;
    if (consumed) *consumed = res.consumed - ml;
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}
enum PcoError pco_chunk_decompressor_read_page(PcoGfxChunkDecompressor* cd, const void* src, size_t len, size_t page_n, void* dst,
                                               size_t dst_cap, size_t* n_processed, size_t* consumed) {
  return read_page_impl(cd, src, len, page_n, dst, dst_cap, n_processed, consumed, nullptr);
}
void pco_chunk_decompressor_free(PcoGfxChunkDecompressor* cd) { delete cd; }

// PageDecompressor (wrapped/page_decompressor.rs:115-246): the page is decoded on the device when the handle is created (a page is
// one serial tANS stream; partial decodes would re-walk it) and `read` hands the numbers out at the reference's granularity -- with the
// reference's error timing: a page whose metadata is bad fails here, a page that goes wrong in batch k hands out the batches before k
// and fails on the call that reaches k (the last batch for the end-of-page checks).  (What differs: the footprint -- a page, not a batch.)
enum PcoError pco_page_decompressor_new(PcoGfxChunkDecompressor* cd, const void* src, size_t len, size_t page_n, PcoGfxPageDecompressor** out) {
  clear_error();
  try {
    const int bits = dtype_bits(cd->dtype);
    std::unique_ptr<PcoGfxPageDecompressor> pd(new PcoGfxPageDecompressor());
    pd->elem = (size_t)bits / 8; pd->n = page_n; pd->pos = 0;
    pd->nums.resize(std::max<size_t>(page_n, 1) * pd->elem);
    size_t n_done = 0, used = 0; int partial = 0;
    const PcoError code = read_page_impl(cd, src, len, page_n, pd->nums.data(), std::max<size_t>(page_n, 1), &n_done, &used, &partial);
    if (code != PcoSuccess && !partial) return code;
    pd->n_ok = code == PcoSuccess ? page_n : n_done;
    pd->bad_status = code == PcoSuccess ? 0 : pco_gfx_last_status();
    if (code != PcoSuccess) clear_error();
    pd->consumed = used;
    *out = pd.release();
    return PcoSuccess;
  } catch (const HostError& e) { return fail_with(e, PcoDecompressionError); }
}
enum PcoError pco_page_decompressor_read(PcoGfxPageDecompressor* pd, void* dst, size_t dst_len, size_t* n_processed, int* finished) {
  clear_error();
  const size_t remaining = pd->n - pd->pos;
  if (dst_len % kBatchN != 0 && dst_len < remaining) {   // page_decompressor.rs:199-206
    set_error(PCO_GFX_INVALID_ARGUMENT, "num_dst's length must either be a multiple of 256 or be at least the count of numbers remaining (" +
                                            std::to_string(dst_len) + " < " + std::to_string(remaining) + ")");
    return PcoDecompressionError;
  }
  const size_t k = std::min(dst_len, remaining);
  if (pd->pos + k > pd->n_ok) {   // the call reaches the batch the page failed in: what came before it is written, the call fails
    const size_t good = pd->n_ok > pd->pos ? pd->n_ok - pd->pos : 0;
    if (good) std::memcpy(dst, pd->nums.data() + pd->pos * pd->elem, good * pd->elem);
    pd->pos = pd->n_ok;
    if (n_processed) *n_processed = 0;
    set_error(pd->bad_status, "page failed to decompress");
    return PcoDecompressionError;
  }
  if (k) std::memcpy(dst, pd->nums.data() + pd->pos * pd->elem, k * pd->elem);
  pd->pos += k;
  if (n_processed) *n_processed = k;
  if (finished) *finished = pd->pos == pd->n ? 1 : 0;
  return PcoSuccess;
}
size_t pco_page_decompressor_consumed(const PcoGfxPageDecompressor* pd) { return pd->consumed; }   /* into_src: bytes of the page */
enum PcoError pco_chunk_compressor_meta_info(const PcoGfxChunkCompressor* cc, unsigned char dtype, PcoGfxChunkMetaInfo* out) {
  if (!cc) { clear_error(); set_error(PCO_GFX_INVALID_ARGUMENT, "null handle"); return PcoCompressionError; }
  return pco_gfx_chunk_meta_info(cc->meta.data(), cc->meta.size(), dtype, 4, out);
}
enum PcoError pco_chunk_decompressor_meta_info(const PcoGfxChunkDecompressor* cd, PcoGfxChunkMetaInfo* out) {
  if (!cd) { clear_error(); set_error(PCO_GFX_INVALID_ARGUMENT, "null handle"); return PcoDecompressionError; }
  return pco_gfx_chunk_meta_info(cd->meta.data(), cd->meta.size(), cd->dtype, cd->format_major, out);
}
void pco_page_decompressor_free(PcoGfxPageDecompressor* pd) { delete pd; }

}  // extern "C"
