// verify.hip -- the device side of a verified encode (include/pco_gfx.h section 3b): PCO_GFX_CFG_VERIFY, pco_gfx_verify_chunks and
// pco_gfx_verify_wrapped_chunks decode the bytes an encode left through the library's own decode entry point into workspace scratch, and the
// kernels here do the rest.
//   verify_resolve_kernel      in front of the decode, on the DEVICE copy of its tasks: each task's source length from the encode's results (the
//                              host of an asynchronous call does not know them), and a task whose encode did not end OK -- or whose results name
//                              bytes outside its dst -- refused the way dir_resolve.hip refuses one: dtype 0 and no bytes, which the decoders
//                              answer with PCO_GFX_INVALID_ARGUMENT before they read anything.  Its stale dst is never decoded.
//   verify_compare_kernel      one pass over the source numbers and the decoded ones: two streams read, nothing written but one atomicMin per
//                              wave that saw a difference.  A comparison of BYTES: NaN payloads and the two zeros are distinct.
//   verify_finish_kernel       the verdict (pco_verify.h) per task, or per wrapped chunk over its pieces.
#pragma once
#include "pco_dev.h"
#include "pco_verify.h"
#include "decode_kernel.hip"   // MetaRef

namespace pcogfx {

// one stream pair of the compare kernel: a standalone chunk, or one page of a wrapped chunk
struct VerifyItem { const void* src; const void* dec; uint64_t n; uint32_t esz_log, pad; };   // src: naturally aligned; dec: 16-byte aligned scratch
static_assert(sizeof(VerifyItem) == 32, "VerifyItem");
// wrapped: where a page task's pieces are named (indices into the piece directory) and the chunk they lie in
struct VerifyPiece { const uint8_t* dst; uint64_t dst_cap; uint32_t meta_piece, page_piece; };
static_assert(sizeof(VerifyPiece) == 24, "VerifyPiece");
// wrapped: a chunk's pieces (the ChunkMeta's at piece0, its pages behind it) and its first page task
struct VerifyChunk { uint32_t piece0, n_pages, task0, pad; };
// what launch_decode takes as its optional verify argument: exactly one of d_encoded (standalone) and d_infos + pieces (wrapped; pieces is a HOST array)
struct VerifyPatch { const PcoGfxTaskResult* d_encoded; const PcoGfxPageInfo* d_infos; const VerifyPiece* pieces; };

// The host uploads src_len = dst_cap - 16 (what the task's dst can hold with the 16 readable bytes a decode source needs behind it).
__global__ __launch_bounds__(256) void verify_resolve_kernel(PcoGfxDecodeTask* tasks, const PcoGfxTaskResult* enc, uint32_t n_tasks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  PcoGfxDecodeTask PCO_GLOBAL* t = as_global(tasks) + i;
  const PcoGfxTaskResult PCO_GLOBAL* e = as_global(enc) + i;
  const uint64_t len = e->n_out;
  if (e->status == PCO_GFX_OK && len <= t->src_len) { t->src_len = len; return; }
  t->src_len = 0; t->dtype = 0;
}
__global__ __launch_bounds__(256) void verify_resolve_wrapped_kernel(PcoGfxDecodeTask* tasks, MetaRef* metas, const VerifyPiece* pieces, const PcoGfxPageInfo* infos, uint32_t n_tasks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  PcoGfxDecodeTask PCO_GLOBAL* t = as_global(tasks) + i;
  MetaRef PCO_GLOBAL* m = as_global(metas) + i;
  const VerifyPiece PCO_GLOBAL* pc = as_global(pieces) + i;
  const PcoGfxPageInfo PCO_GLOBAL* im = as_global(infos) + pc->meta_piece;
  const PcoGfxPageInfo PCO_GLOBAL* ip = as_global(infos) + pc->page_piece;
  const uint64_t cap = pc->dst_cap;   // (>= 16: checked by the host)
  const uint64_t m_off = im->offset, m_len = im->len, p_off = ip->offset, p_len = ip->len;
  const bool inside = m_off <= cap - 16 && m_len <= cap - 16 - m_off && p_off <= cap - 16 && p_len <= cap - 16 - p_off;
  if (im->status == PCO_GFX_OK && ip->status == PCO_GFX_OK && inside) {
    t->src = pc->dst + p_off; t->src_len = p_len;
    m->p = pc->dst + m_off; m->len = m_len;
    return;
  }
  t->src = pc->dst; t->src_len = 0; t->dtype = 0;
  m->p = pc->dst; m->len = 0;   // (never nullptr: that would mean "the ChunkMeta is in front of the page")
}

// Blocks map onto items in fixed pieces of 64 KiB, as compact_copy_kernel's do: block b takes piece b % pieces of item b / pieces.
constexpr uint32_t kVerifyPieceBytes = 64 * 1024;

// Bytes [s0, s1) of one item, s0 a multiple of the piece size: whole 16-byte vectors four in flight per lane -- the decoded side aligned, the source
// side through an under-aligned vector type (a source is aligned to its number type only) -- and the numbers behind the last whole vector one per lane.
// kFind false: non-zero iff the lane saw a difference.  kFind true: the lowest index of a differing NUMBER the lane saw, or ~0.
template <bool kFind>
__device__ __forceinline__ uint32_t verify_scan_piece(gcptr_u8 src, gcptr_u8 dec, uint64_t s0, uint64_t s1, uint32_t esz_log, uint32_t tid) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef u32x4 __attribute__((aligned(1))) u32x4_unaligned;
  uint32_t acc = kFind ? 0xffffffffu : 0u;
  auto fold = [&](u32x4 d, uint64_t byte0) {
    const uint32_t any = d.x | d.y | d.z | d.w;
    if constexpr (!kFind) acc |= any;
    else if (any) {
      const uint32_t w = d.x ? 0u : (d.y ? 1u : (d.z ? 2u : 3u)), dw = d.x ? d.x : (d.y ? d.y : (d.z ? d.z : d.w));
      const uint32_t idx = (uint32_t)((byte0 + 4 * w + ((uint32_t)__builtin_ctz(dw) >> 3)) >> esz_log);   // (< 2^24)
      acc = idx < acc ? idx : acc;
    }
  };
  const uint32_t nq = (uint32_t)((s1 - s0) >> 4);
  uint32_t q = tid;
  for (; q + 3 * 256 < nq; q += 4 * 256) {
    u32x4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; u++) a[u] = *(const u32x4_unaligned PCO_GLOBAL*)(src + s0 + ((uint64_t)(q + u * 256) << 4));
#pragma unroll
    for (int u = 0; u < 4; u++) b[u] = *(const u32x4 PCO_GLOBAL*)(dec + s0 + ((uint64_t)(q + u * 256) << 4));
#pragma unroll
    for (int u = 0; u < 4; u++) fold(a[u] ^ b[u], s0 + ((uint64_t)(q + u * 256) << 4));
  }
  for (; q < nq; q += 256) {
    const uint64_t at = s0 + ((uint64_t)q << 4);
    fold(*(const u32x4_unaligned PCO_GLOBAL*)(src + at) ^ *(const u32x4 PCO_GLOBAL*)(dec + at), at);
  }
  const uint64_t t0 = s0 + ((uint64_t)nq << 4);
  if (tid < (uint32_t)((s1 - t0) >> esz_log)) {   // fewer than 16 bytes: the tail of an item's last piece
    const uint64_t at = t0 + ((uint64_t)tid << esz_log);
    uint64_t x;
    if (esz_log == 3) x = *(const uint64_t PCO_GLOBAL*)(src + at) ^ *(const uint64_t PCO_GLOBAL*)(dec + at);
    else if (esz_log == 2) x = *(const uint32_t PCO_GLOBAL*)(src + at) ^ *(const uint32_t PCO_GLOBAL*)(dec + at);
    else if (esz_log == 1) x = (uint64_t)(*(const uint16_t PCO_GLOBAL*)(src + at) ^ *(const uint16_t PCO_GLOBAL*)(dec + at));
    else x = (uint64_t)(src[at] ^ dec[at]);
    if constexpr (!kFind) acc |= x != 0 ? 1u : 0u;
    else if (x != 0) { const uint32_t idx = (uint32_t)(at >> esz_log); acc = idx < acc ? idx : acc; }
  }
  return acc;
}

// dec_res[i]: the decode's result for item i.  An item whose decode did not end OK has nothing to compare (verify_verdict does not look at its
// first-difference word); one that decoded fewer numbers than n is compared over those.  first[i] was set to ~0 by the host.
__global__ __launch_bounds__(256) void verify_compare_kernel(const VerifyItem* items, const PcoGfxTaskResult* dec_res, unsigned long long* first, uint32_t n_items, uint32_t pieces) {
  const uint32_t i = blockIdx.x / pieces, pc = blockIdx.x - i * pieces;
  if (i >= n_items) return;
  const PcoGfxTaskResult PCO_GLOBAL* r = as_global(dec_res) + i;
  if (r->status != PCO_GFX_OK) return;
  const VerifyItem PCO_GLOBAL* it = as_global(items) + i;
  const uint64_t n = it->n, got = r->n_out, m = got < n ? got : n;
  const uint32_t esz_log = it->esz_log;
  const uint64_t bytes = m << esz_log, s0 = (uint64_t)pc * kVerifyPieceBytes;
  if (s0 >= bytes) return;
  const uint64_t s1 = s0 + kVerifyPieceBytes < bytes ? s0 + kVerifyPieceBytes : bytes;
  gcptr_u8 src = (gcptr_u8)it->src, dec = (gcptr_u8)it->dec;
  const uint32_t tid = threadIdx.x;
  if (wave_or_u32(verify_scan_piece<false>(src, dec, s0, s1, esz_log, tid)) == 0) return;   // (every return above is the whole block's)
  // a wave that saw a difference goes over its lanes' bytes once more for the lowest differing number
  const uint32_t low = wave_reduce_u32(verify_scan_piece<true>(src, dec, s0, s1, esz_log, tid), [](uint32_t a, uint32_t b) { return a < b ? a : b; });
  if (lane_id() == 0 && low != 0xffffffffu) atomicMin(first + i, (unsigned long long)low);
}

__device__ __forceinline__ VerifyResult verify_item_verdict(VerifyResult enc, const VerifyItem* items, const PcoGfxTaskResult* dec_res, const unsigned long long* first, uint32_t i) {
  const PcoGfxTaskResult PCO_GLOBAL* d = as_global(dec_res) + i;
  return verify_verdict(enc, d->status, d->n_out, as_global(items)[i].n, as_global(first)[i]);
}
// standalone: one thread per task.  `out` may be `enc`: a thread reads its entry before it writes it.
__global__ __launch_bounds__(256) void verify_finish_kernel(const VerifyItem* items, const PcoGfxTaskResult* enc, const PcoGfxTaskResult* dec_res, const unsigned long long* first,
                                                            PcoGfxTaskResult* out, uint32_t n_tasks) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  const PcoGfxTaskResult PCO_GLOBAL* e = as_global(enc) + i;
  const VerifyResult v = verify_item_verdict(VerifyResult{e->n_out, e->consumed, e->status, e->aux}, items, dec_res, first, i);
  PcoGfxTaskResult PCO_GLOBAL* o = as_global(out) + i;
  o->n_out = v.n_out; o->consumed = v.consumed; o->status = v.status; o->aux = v.aux;
}
// wrapped: one thread per chunk over its pieces, which report status and aux only (PcoGfxPageInfo has no field for an index).  A chunk whose
// ChunkMeta piece is not OK keeps all its pieces as they are.  The ChunkMeta piece is verified iff every page is; it is Corruption when a page is.
__global__ __launch_bounds__(256) void verify_finish_wrapped_kernel(const VerifyChunk* chunks, const VerifyItem* items, const PcoGfxPageInfo* enc, const PcoGfxTaskResult* dec_res,
                                                                    const unsigned long long* first, PcoGfxPageInfo* out, uint32_t n_chunks) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_chunks) return;
  const VerifyChunk ch = chunks[c];   // (plain pointers: a handful of records per thread)
  const PcoGfxPageInfo meta = enc[ch.piece0];
  bool all = meta.status == PCO_GFX_OK, bad = false;
  for (uint32_t p = 0; p < ch.n_pages; p++) {
    PcoGfxPageInfo info = enc[ch.piece0 + 1 + p];
    if (meta.status == PCO_GFX_OK) {
      const VerifyResult v = verify_item_verdict(VerifyResult{info.len, 0, info.status, info.aux}, items, dec_res, first, ch.task0 + p);
      all = all && v.status == PCO_GFX_OK && (v.aux & kVerifyAuxVerified) != 0;
      bad = bad || (info.status == PCO_GFX_OK && v.status != PCO_GFX_OK);
      info.status = v.status; info.aux = v.aux;
    }
    out[ch.piece0 + 1 + p] = info;
  }
  PcoGfxPageInfo m = meta;
  if (all) m.aux |= kVerifyAuxVerified;
  else if (bad) { m.status = PCO_GFX_CORRUPTION; m.aux &= ~kVerifyAuxVerified; }
  out[ch.piece0] = m;
}

}  // namespace pcogfx
