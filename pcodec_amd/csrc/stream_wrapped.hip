// stream_wrapped.hip -- the wrapped batched encoder's piece directory on the device, and the assembly of its pieces into one stream.
//
// pco_gfx_compress_wrapped_chunks_ex leaves every piece of a chunk (its ChunkMeta, then its pages) in a worst-case-sized slot inside the
// chunk's dst; on compressible data the slots are several times the bytes written.  pco_gfx_compact_wrapped_chunks moves the pieces into one
// contiguous stream, `gap` untouched bytes in front of each for the caller's own framing, without a host round trip:
//   wcompact_valid_kernel   a chunk with any failed piece is dropped whole (a wave per chunk; also the piece -> chunk map)
//   wcompact_scan_kernel    two exclusive scans over the pieces: bytes (len + gap) and 16 KiB work slices (one block, four pieces per thread)
//   wcompact_copy_kernel    a persistent grid; every WAVE takes a contiguous run of slices, finds its first piece by binary search in the
//                           slice prefix and walks on from there.  A small piece (a ChunkMeta of a few dozen bytes) is one slice: one wave's
//                           work, not a block's.  Destination-aligned 16-byte stores from unaligned 16-byte loads, eight loads in flight per
//                           lane; the bytes before the first / after the last aligned quad go one by one.
// Pieces range from a few dozen bytes to megabytes, a call can hold a million of them, and an asynchronous caller does not know their
// lengths on the host: a grid sized from capacities (compact_copy_kernel) does not carry over.  HBM-bound: 2 x compressed size.
#pragma once
#include "pco_dev.h"

namespace pcogfx {

// PcoGfxPageInfo entries of a wrapped encode, from the per-page results: the offsets are the slots' (known before launch: EncPage::dst)
__global__ __launch_bounds__(256) void wrapped_infos_kernel(const EncPage* pages, const PcoGfxEncodeTask* tasks, const PcoGfxTaskResult* res, PcoGfxPageInfo* infos, uint32_t n_pieces) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_pieces) return;
  const EncPage PCO_GLOBAL* p = as_global(pages) + k;
  PcoGfxPageInfo PCO_GLOBAL* e = as_global(infos) + k;
  e->offset = (uint64_t)((const uint8_t*)p->dst - (const uint8_t*)as_global(tasks)[p->chunk].dst);
  e->len = as_global(res)[k].n_out; e->n = p->n; e->status = as_global(res)[k].status; e->aux = as_global(res)[k].aux;
}

struct WcChunk { const uint8_t* dst; uint64_t dst_cap; uint32_t piece_first, n_pieces; };
static_assert(sizeof(WcChunk) == 24, "WcChunk");
constexpr uint32_t kWcSliceLog = 14;          // 16 KiB of a piece per work slice
constexpr uint32_t kWcDropped = 0xffffffffu;  // piece_chunk[] of a piece whose chunk contributes nothing

// grid = ceil(n_chunks / 4) blocks of four waves, a wave per chunk: piece_chunk[k] = the piece's chunk, or kWcDropped when ANY piece of the chunk
// failed (a chunk without one of its pages is of no use to a reader) or claims bytes beyond its chunk's dst
__global__ __launch_bounds__(256) void wcompact_valid_kernel(const WcChunk* chunks, const PcoGfxPageInfo* infos, uint32_t* piece_chunk, uint32_t n_chunks) {
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= n_chunks) return;
  const WcChunk PCO_GLOBAL* chp = as_global(chunks) + c;
  const struct { uint64_t dst_cap; uint32_t piece_first, n_pieces; } ch = {uni(chp->dst_cap), uni(chp->piece_first), uni(chp->n_pieces)};
  bool bad = false;
  for (uint32_t p = lane; p < ch.n_pieces; p += 64) {
    const PcoGfxPageInfo PCO_GLOBAL* e = as_global(infos) + ch.piece_first + p;
    const uint64_t off = e->offset, len = e->len;
    bad |= e->status != PCO_GFX_OK || off > ch.dst_cap || len > ch.dst_cap - off;
  }
  const uint32_t v = __any(bad) ? kWcDropped : c;
  for (uint32_t p = lane; p < ch.n_pieces; p += 64) as_global(piece_chunk)[ch.piece_first + p] = v;
}

// offsets[k] = base + the bytes (len + gap) of the kept pieces before k, offsets[n] = the end (~0 when it exceeds dst_cap); slice_pfx[k] = the work
// slices before piece k, slice_pfx[n] = all of them (0 on overflow: nothing is copied)
__global__ __launch_bounds__(1024) void wcompact_scan_kernel(const PcoGfxPageInfo* infos, const uint32_t* piece_chunk, uint32_t n, uint32_t gap, uint64_t base, uint64_t dst_cap,
                                                             uint64_t* offsets, uint32_t* slice_pfx, uint32_t* overflow) {
  __shared__ uint64_t part_b[16], part_s[16];
  __shared__ uint64_t carry_b, carry_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { carry_b = base; carry_s = 0; }
  __syncthreads();
  for (uint64_t i0 = 0; i0 < n; i0 += 4096) {
    const uint64_t k0 = i0 + (uint64_t)tid * 4;
    uint64_t b[4], s[4], tot_b = 0, tot_s = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t k = k0 + u;
      const bool keep = k < n && as_global(piece_chunk)[k] != kWcDropped;
      const uint64_t len = keep ? as_global(infos)[k].len : 0ull;
      b[u] = keep ? len + gap : 0ull; s[u] = (len + ((1ull << kWcSliceLog) - 1)) >> kWcSliceLog;
      tot_b += b[u]; tot_s += s[u];
    }
    const uint64_t incl_b = wave_incl_scan(tot_b), incl_s = wave_incl_scan(tot_s);
    if (lane == 63) { part_b[wave] = incl_b; part_s[wave] = incl_s; }
    __syncthreads();
    uint64_t before_b = carry_b, before_s = carry_s;
    for (uint32_t w = 0; w < wave; w++) { before_b += part_b[w]; before_s += part_s[w]; }
    uint64_t run_b = before_b + incl_b - tot_b, run_s = before_s + incl_s - tot_s;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t k = k0 + u;
      if (k < n) { as_global(offsets)[k] = run_b; as_global(slice_pfx)[k] = (uint32_t)run_s; }
      run_b += b[u]; run_s += s[u];
    }
    __syncthreads();
    if (tid == 1023) { carry_b = before_b + incl_b; carry_s = before_s + incl_s; }
    __syncthreads();
  }
  // (an asynchronous caller never sees `overflow`: the end offset it is handed reads ~0 when the destination is too small)
  if (tid == 0) {
    const bool over = carry_b > dst_cap || carry_b < base || carry_s > 0xffffffffull;
    as_global(offsets)[n] = over ? ~0ull : carry_b; as_global(slice_pfx)[n] = over ? 0u : (uint32_t)carry_s; *as_global(overflow) = over ? 1u : 0u;
  }
}

// persistent: gridDim.x blocks of four waves; wave w copies slices [w * per, (w + 1) * per) of the work list
__global__ __launch_bounds__(256) void wcompact_copy_kernel(const WcChunk* chunks, const PcoGfxPageInfo* infos, const uint32_t* piece_chunk, const uint64_t* offsets,
                                                            const uint32_t* slice_pfx, uint8_t* dst, uint32_t n_pieces, uint32_t gap) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef u32x4 __attribute__((aligned(1))) u32x4_unaligned;
  const uint32_t PCO_GLOBAL* pfx = as_global(slice_pfx);
  const uint64_t total = uni(pfx[n_pieces]);
  const uint64_t n_waves = (uint64_t)gridDim.x * 4, w = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t per = (total + n_waves - 1) / n_waves;
  const uint64_t first = w * per, last = first + per < total ? first + per : total;
  if (first >= last) return;
  // the piece of slice `first`: the first k with slice_pfx[k + 1] > first (pieces without slices -- dropped, or empty -- are stepped over)
  uint32_t lo = 0, hi = n_pieces;
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (uni(pfx[mid + 1]) > first) hi = mid; else lo = mid + 1; }
  uint32_t k = lo;
  for (uint64_t sl = first; sl < last; sl++) {
    while (k < n_pieces && uni(pfx[k + 1]) <= sl) k++;
    if (k >= n_pieces) return;   // (cannot happen: sl < slice_pfx[n_pieces])
    const uint32_t c = uni(as_global(piece_chunk)[k]);
    if (c == kWcDropped) return;   // (cannot happen: a dropped piece has no slices)
    const uint64_t len = uni(as_global(infos)[k].len);
    const uint64_t s0 = (sl - uni(pfx[k])) << kWcSliceLog;
    if (s0 >= len) continue;
    const uint64_t s1 = s0 + (1ull << kWcSliceLog) < len ? s0 + (1ull << kWcSliceLog) : len;
    gcptr_u8 src = (gcptr_u8)as_global(chunks)[c].dst + uni(as_global(infos)[k].offset);
    gptr_u8 out = (gptr_u8)dst + uni(as_global(offsets)[k]) + gap;
    // destination-aligned 16-byte quads inside [s0, s1); the bytes before the first / after the last quad go one by one
    const uint64_t a0 = (uint64_t)(uintptr_t)(out + s0);
    uint64_t head = (16 - (a0 & 15)) & 15;
    if (head > s1 - s0) head = s1 - s0;
    const uint64_t q0 = s0 + head, nq = (s1 - q0) >> 4, tail0 = q0 + (nq << 4);
    if (lane < head) out[s0 + lane] = src[s0 + lane];
    if (lane < s1 - tail0) out[tail0 + lane] = src[tail0 + lane];
    for (uint64_t qb = 0; qb < nq; qb += 8 * 64) {   // eight loads in flight per lane
      u32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) { const uint64_t q = qb + u * 64 + lane; if (q < nq) v[u] = *(const u32x4_unaligned PCO_GLOBAL*)(src + q0 + (q << 4)); }
#pragma unroll
      for (int u = 0; u < 8; u++) { const uint64_t q = qb + u * 64 + lane; if (q < nq) *(u32x4 PCO_GLOBAL*)(out + q0 + (q << 4)) = v[u]; }
    }
  }
}

}  // namespace pcogfx
