// pco_meta_info.inc -- pco_gfx_chunk_meta_info, the host-side ChunkMeta parser (included by pco_gfx.hip).
extern "C" {

// ChunkMeta accessors: a host-side read of the metadata bytes (metadata/chunk.rs:127-174, mode.rs:138-195, delta_encoding.rs:120-200,
// chunk_latent_var.rs:30-71).  O(bytes of metadata); nothing touches the device.
enum PcoError pco_gfx_chunk_meta_info(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, PcoGfxChunkMetaInfo* out) {
  clear_error();
  const int LB = dtype_bits(dtype);
  if (!LB || !out || (!meta && len)) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_info: bad argument"); return PcoInvalidType; }
  std::memset(out, 0, sizeof(*out));
  const uint8_t* p = (const uint8_t*)meta;
  uint64_t bit = 0; bool short_read = false;
  auto rd = [&](uint32_t n) -> uint64_t {   // little-endian bit stream (bit_reader.rs)
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; i++, bit++) { const uint64_t byte = bit >> 3; if (byte >= len) { short_read = true; continue; } v |= (uint64_t)((p[byte] >> (bit & 7)) & 1u) << i; }
    return v;
  };
  auto fail = [&](int st, const char* msg) { set_error(st, msg); return PcoDecompressionError; };
  out->mode_kind = (uint32_t)rd(kBitsModeVariant);
  if (out->mode_kind == kIntMult || out->mode_kind == kFloatMult) out->mode_base_latent = rd((uint32_t)LB);
  else if (out->mode_kind == kFloatQuant) out->mode_k = (uint32_t)rd(kBitsQuantK);
  else if (out->mode_kind == kDict) { if (short_read) return fail(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoSuccess; }   // (the dictionary follows: kinds only)
  else if (out->mode_kind != kClassic) return fail(short_read ? PCO_GFX_INSUFFICIENT_DATA : PCO_GFX_CORRUPTION, "unknown mode");
  if (format_major < 3) { out->delta_order = (uint32_t)rd(kBitsDeltaOrder); out->delta_kind = out->delta_order ? kDeltaConsecutive : kDeltaNone; }
  else {
    out->delta_kind = (uint32_t)rd(kBitsDeltaVariant);
    // (the reference's own validation, metadata/delta_encoding.rs:143-176: a zero order, a window beyond the maximum and a state beyond the window are Corruption)
    if (out->delta_kind == kDeltaConsecutive) {
      out->delta_order = (uint32_t)rd(kBitsDeltaOrder);
      if (!short_read && out->delta_order == 0) return fail(PCO_GFX_CORRUPTION, "Consecutive delta encoding order must not be 0");
      out->secondary_uses_delta = (uint32_t)rd(1);
    } else if (out->delta_kind == kDeltaLookback) {
      out->window_n_log = 1 + (uint32_t)rd(kBitsLookbackWindowLog); out->state_n_log = (uint32_t)rd(kBitsLookbackStateLog);
      if (!short_read && out->window_n_log > kMaxLookbackWindowLog) return fail(PCO_GFX_CORRUPTION, "lookback delta encoding window size log exceeds the maximum");
      if (!short_read && out->state_n_log > out->window_n_log) return fail(PCO_GFX_CORRUPTION, "lookback delta encoding state size log exceeds the window size log");
      out->secondary_uses_delta = (uint32_t)rd(1);
    }
    else if (out->delta_kind == kDeltaConv1) { if (short_read) return fail(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoSuccess; }   // (weights follow: kinds only)
    else if (out->delta_kind != kDeltaNone) return fail(short_read ? PCO_GFX_INSUFFICIENT_DATA : PCO_GFX_CORRUPTION, "unknown delta encoding");
  }
  out->present[0] = out->delta_kind == kDeltaLookback; out->present[1] = 1;
  out->present[2] = out->mode_kind == kIntMult || out->mode_kind == kFloatMult || out->mode_kind == kFloatQuant;
  for (int v = 0; v < 3; v++) {
    if (out->present[v]) {
      const uint32_t lb = v == 0 ? 32u : (uint32_t)LB;
      out->ans_size_log[v] = (uint32_t)rd(kBitsAnsSizeLog); out->n_bins[v] = (uint32_t)rd(kBitsNBins);
      bit += (uint64_t)out->n_bins[v] * (out->ans_size_log[v] + lb + offset_bits_bits((int)lb));
    }
    if (short_read || (bit + 7) / 8 > len) return fail(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short");
    out->n_vars_parsed = (uint32_t)v + 1;
  }
  out->meta_bytes = (bit + 7) / 8;
  return PcoSuccess;
}
enum PcoError pco_gfx_chunk_meta_conv1(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, uint32_t* quantization,
                                       int64_t* bias, int32_t* weights, uint32_t* order) {
  clear_error();
  const int LB = dtype_bits(dtype);
  if (!LB || !quantization || !bias || !weights || !order || (!meta && len)) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_conv1: bad argument"); return PcoInvalidType; }
  *order = 0; *quantization = 0; *bias = 0;
  const uint8_t* p = (const uint8_t*)meta;
  uint64_t bit = 0; bool short_read = false;
  auto rd = [&](uint32_t n) -> uint64_t {   // little-endian bit stream (bit_reader.rs)
    uint64_t v = 0;
    for (uint32_t i = 0; i < n; i++, bit++) { const uint64_t byte = bit >> 3; if (byte >= len) { short_read = true; continue; } v |= (uint64_t)((p[byte] >> (bit & 7)) & 1u) << i; }
    return v;
  };
  const uint32_t mode_kind = (uint32_t)rd(kBitsModeVariant);
  if (mode_kind == kIntMult || mode_kind == kFloatMult) rd((uint32_t)LB);
  else if (mode_kind == kFloatQuant) rd(kBitsQuantK);
  else if (mode_kind != kClassic) { set_error(PCO_GFX_UNSUPPORTED, "chunk_meta_conv1: Dict or unknown mode"); return PcoDecompressionError; }
  if (format_major >= 3 && rd(kBitsDeltaVariant) == kDeltaConv1) {
    const uint32_t q = (uint32_t)rd(5);
    const uint64_t b = rd(64) ^ (1ull << 63);
    const uint32_t ord = (uint32_t)rd(5) + 1;
    for (uint32_t k = 0; k < ord; k++) weights[k] = (int32_t)((uint32_t)rd(32) ^ 0x80000000u);
    if (short_read) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
    *quantization = q; *bias = (int64_t)b; *order = ord;
  }
  if (short_read) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  return PcoSuccess;
}
enum PcoError pco_gfx_chunk_meta_dict(const void* meta, size_t len, unsigned char dtype, uint8_t format_major, uint32_t* n_unique, void* values,
                                      size_t cap) {
  clear_error();
  const int LB = dtype_bits(dtype);
  if (!LB || !n_unique || (!meta && len) || (!values && cap)) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_dict: bad argument"); return PcoInvalidType; }
  (void)format_major;   // (the mode section is the same in every format version)
  *n_unique = 0;
  const uint8_t* p = (const uint8_t*)meta;
  if (len == 0) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  if ((p[0] & 0xfu) != kDict) return PcoSuccess;
  // 4-bit variant, 25-bit length, zeros to the byte, then the dictionary as whole little-endian latents
  if (len < 4) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  const uint32_t hdr = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  const uint32_t k = (hdr >> 4) & ((1u << kBitsDictLen) - 1);
  const size_t vb = (size_t)LB / 8;
  *n_unique = k;
  if ((size_t)k * vb > len - 4) { set_error(PCO_GFX_INSUFFICIENT_DATA, "chunk metadata is cut short"); return PcoDecompressionError; }
  if (k > cap) { set_error(PCO_GFX_INVALID_ARGUMENT, "chunk_meta_dict: values holds fewer than n_unique entries"); return PcoInvalidType; }
  std::memcpy(values, p + 4, (size_t)k * vb);
  return PcoSuccess;
}

}  // extern "C"
