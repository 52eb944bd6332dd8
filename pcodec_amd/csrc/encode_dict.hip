// encode_dict.hip -- Dict mode encode (mode/dict.rs:10-66), opt-in behind PCO_GFX_CFG_DICT.
//
// Per chunk, before the rest of the pipeline: the distinct ordered latents and their counts, the dictionary sorted by (count descending,
// ordered latent ascending), and every number's u32 dictionary index.  The chunk is then encoded as a Classic u32 chunk of those indices
// (the pipeline's variable 1 is 32 bits wide, like the reference's primary latent type for Dict); the meta writers put Mode::Dict in
// front, and enc_dict_place_kernel copies the dictionary bytes into the hole they leave behind the Dict header.
//
// The reference breaks ties between equal counts in HashMap iteration order, which is not defined; this encoder takes ascending ordered
// latent, which is one of the orders the reference may write, and makes the bytes independent of insertion races and task order.
//
// Two table homes, one 1024-thread block per chunk:
//  - enc_dict_lds_kernel: an open-addressing table of kDictLdsSlots in LDS while the chunk has at most kDictLdsMaxK distinct latents;
//    a bitonic sort of the occupied slots' indices in LDS orders them.
//  - enc_dict_hbm_kernel: the chunks that outgrew it, with a table of 2^ceil(log2(2n)) slots in their own HBM slot, and a bitonic sort
//    of the compacted entries there.
// Free slots hold kDictEmpty; the latent with that bit pattern (only 64-bit types have it) is counted in an extra slot behind the table.
// Memory model: a table belongs to one workgroup.  Its slots are claimed and counted with atomics; everything that reads them after a
// __syncthreads (compaction, ordering, the index pass) is in the same workgroup, whose waves share one L1 and see each other's writes at
// workgroup scope, HBM tables included.  The probe during counting loads a slot atomically (relaxed): a stale kDictEmpty only sends it to
// the CAS, which decides.
namespace pcogfx {

// (DictTask, the per-chunk record: encode_kernels.hip)
constexpr uint32_t kNoDictSlot = 0xffffffffu;
constexpr uint32_t kDictThreads = 1024;
constexpr uint32_t kDictLdsSlots = 8192, kDictLdsMaxK = 4096;
constexpr uint32_t kDictNoSlot = 0xffffu;   // padding of the LDS sort (slot indices are at most kDictLdsSlots)
constexpr uint64_t kDictEmpty = ~0ull;
// LDS: keys u64[slots + 1] | counts (ranks, once ordered) u32[slots + 1] | occupied slot list u16[max k] | counters u32[4]
constexpr uint32_t kDictLdsKeys = 0, kDictLdsCnt = (kDictLdsSlots + 1) * 8, kDictLdsList = kDictLdsCnt + (((kDictLdsSlots + 1) * 4 + 15) & ~15u);
constexpr uint32_t kDictLdsCtr = kDictLdsList + kDictLdsMaxK * 2, kDictLdsBytes = kDictLdsCtr + 16;
// HBM slot of a chunk of up to n_max numbers: keys u64[2P + 1] | counts u32[2P + 1] | entries DictEntry[P], P = next power of two >= n_max
struct DictEntry { uint64_t key; uint32_t cnt, slot; };
__host__ __device__ inline uint64_t dict_pow2(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }
__host__ __device__ inline uint64_t dict_hbm_slot_bytes(uint64_t n_max) {
  const uint64_t p = dict_pow2(n_max < 32 ? 32 : n_max);
  return ((2 * p + 1) * 8 + 255) / 256 * 256 + ((2 * p + 1) * 4 + 255) / 256 * 256 + p * sizeof(DictEntry);
}

__device__ __forceinline__ uint32_t dict_hash(uint64_t x, uint32_t mask) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x & mask;
}
__device__ __forceinline__ uint64_t dict_latent(const void* src, uint64_t i, uint32_t dtype) {
  const uint32_t kind = dtype_kind(dtype);
  switch (dtype_bits(dtype)) {
    case 64: return to_latent_ordered<uint64_t>(((const uint64_t*)src)[i], kind);
    case 32: return to_latent_ordered<uint32_t>(((const uint32_t*)src)[i], kind);
    case 16: return to_latent_ordered<uint16_t>(((const uint16_t*)src)[i], kind);
    default: return to_latent_ordered<uint8_t>(((const uint8_t*)src)[i], kind);
  }
}
__device__ __forceinline__ void dict_put_value(uint8_t* values, uint32_t rank, uint64_t key, uint32_t bytes) {
  if (bytes == 8) ((uint64_t*)values)[rank] = key;
  else if (bytes == 4) ((uint32_t*)values)[rank] = (uint32_t)key;
  else if (bytes == 2) ((uint16_t*)values)[rank] = (uint16_t)key;
  else values[rank] = (uint8_t)key;
}
// count one latent; `mask` + 1 slots, the extra slot at mask + 1.  Returns whether x took a new slot.
__device__ __forceinline__ bool dict_insert(uint64_t* keys, uint32_t* cnt, uint32_t mask, uint64_t x) {
  if (x == kDictEmpty) return atomicAdd(&cnt[mask + 1], 1u) == 0;
  uint32_t h = dict_hash(x, mask);
  for (uint32_t probe = 0; probe <= mask; probe++) {
    uint64_t old = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == kDictEmpty) old = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)kDictEmpty, (unsigned long long)x);
    if (old == kDictEmpty || old == x) { atomicAdd(&cnt[h], 1u); return old == kDictEmpty; }
    h = (h + 1) & mask;
  }
  return false;   // (unreachable: the tables never fill)
}
__device__ __forceinline__ uint32_t dict_find(const uint64_t* keys, uint32_t mask, uint64_t x) {
  if (x == kDictEmpty) return mask + 1;
  uint32_t h = dict_hash(x, mask);
  for (uint32_t probe = 0; probe <= mask && keys[h] != x; probe++) h = (h + 1) & mask;
  return h;
}
// every number's index: the rank its slot holds
__device__ __forceinline__ void dict_map(const DictTask& d, const uint64_t* keys, const uint32_t* rank, uint32_t mask) {
  for (uint64_t i = threadIdx.x; i < d.n; i += kDictThreads) d.idx[i] = rank[dict_find(keys, mask, dict_latent(d.src, i, d.dtype))];
}

// grid = tasks, 1024 threads, kDictLdsBytes of LDS
__global__ __launch_bounds__(kDictThreads) void enc_dict_lds_kernel(DictTask* tasks, uint32_t n_tasks, uint32_t* n_over) {
  const uint32_t t = blockIdx.x, tid = threadIdx.x;
  if (t >= n_tasks) return;
  const DictTask d = tasks[t];
  uint8_t PCO_LDS* smem = enc_lds_base();
  uint64_t* keys = (uint64_t*)(smem + kDictLdsKeys);
  uint32_t* cnt = (uint32_t*)(smem + kDictLdsCnt);
  uint16_t* list = (uint16_t*)(smem + kDictLdsList);
  uint32_t* ctr = (uint32_t*)(smem + kDictLdsCtr);   // [0] slots taken, [1] compacted entries
  constexpr uint32_t mask = kDictLdsSlots - 1;
  for (uint32_t s = tid; s <= kDictLdsSlots; s += kDictThreads) { keys[s] = kDictEmpty; cnt[s] = 0; }
  if (tid < 4) ctr[tid] = 0;
  __syncthreads();
  for (uint64_t i = tid; i < d.n; i += kDictThreads) {
    if (*(volatile uint32_t*)&ctr[0] > kDictLdsMaxK) break;   // (at most 1024 inserts in flight past the limit: the table keeps free slots)
    if (dict_insert(keys, cnt, mask, dict_latent(d.src, i, d.dtype))) atomicAdd(&ctr[0], 1u);
  }
  __syncthreads();
  if (ctr[0] > kDictLdsMaxK) {   // too many distinct latents: enc_dict_hbm_kernel takes the chunk
    if (tid == 0) tasks[t].hslot = atomicAdd(n_over, 1u);
    return;
  }
  for (uint32_t s = tid; s <= kDictLdsSlots; s += kDictThreads)
    if (s < kDictLdsSlots ? keys[s] != kDictEmpty : cnt[s] != 0) list[atomicAdd(&ctr[1], 1u)] = (uint16_t)s;
  __syncthreads();
  const uint32_t k = ctr[1];
  // order the occupied slots by (count descending, ordered latent ascending): a bitonic sort of their indices, padded with kDictNoSlot
  // (after every real entry) to a power of two; an entry's rank is then its position
  const uint32_t p = (uint32_t)dict_pow2(k);
  for (uint32_t e = k + tid; e < p; e += kDictThreads) list[e] = kDictNoSlot;
  __syncthreads();
  auto before = [&](uint32_t a, uint32_t b) {
    if (a == kDictNoSlot) return false;
    if (b == kDictNoSlot) return true;
    const uint32_t ca = cnt[a], cb = cnt[b];
    const uint64_t xa = a < kDictLdsSlots ? keys[a] : kDictEmpty, xb = b < kDictLdsSlots ? keys[b] : kDictEmpty;
    return ca > cb || (ca == cb && xa < xb);
  };
  for (uint32_t size = 2; size <= p; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = tid; i < p / 2; i += kDictThreads) {
        const uint32_t lo = (i / stride) * stride * 2 + (i % stride), hi = lo + stride;
        const uint32_t a = list[lo], b = list[hi];
        if (before(b, a) == ((lo & size) == 0)) { list[lo] = (uint16_t)b; list[hi] = (uint16_t)a; }
      }
      __syncthreads();
    }
  }
  const uint32_t vbytes = (uint32_t)dtype_bits(d.dtype) / 8;
  for (uint32_t r = tid; r < k; r += kDictThreads) {
    const uint32_t s = list[r];
    cnt[s] = r;
    dict_put_value(d.values, r, s < kDictLdsSlots ? keys[s] : kDictEmpty, vbytes);
  }
  if (tid == 0) tasks[t].k = k;
  __syncthreads();
  dict_map(d, keys, cnt, mask);
}

__device__ __forceinline__ bool dict_before(const DictEntry& a, const DictEntry& b) { return a.cnt > b.cnt || (a.cnt == b.cnt && a.key < b.key); }

// grid = tasks, 1024 threads: the chunks enc_dict_lds_kernel handed over, each in its HBM slot of `slot_bytes`
__global__ __launch_bounds__(kDictThreads) void enc_dict_hbm_kernel(DictTask* tasks, uint32_t n_tasks, uint8_t* slots, uint64_t slot_bytes, uint64_t n_max) {
  const uint32_t t = blockIdx.x, tid = threadIdx.x;
  if (t >= n_tasks) return;
  const DictTask d = tasks[t];
  if (d.hslot == kNoDictSlot) return;
  __shared__ uint32_t ctr[2];
  const uint64_t pmax = dict_pow2(n_max < 32 ? 32 : n_max);
  uint8_t* base = slots + (uint64_t)d.hslot * slot_bytes;
  uint64_t* keys = (uint64_t*)base;
  uint32_t* cnt = (uint32_t*)(base + ((2 * pmax + 1) * 8 + 255) / 256 * 256);
  DictEntry* ent = (DictEntry*)((uint8_t*)cnt + ((2 * pmax + 1) * 4 + 255) / 256 * 256);
  const uint32_t mask = (uint32_t)(2 * dict_pow2(d.n < 32 ? 32 : d.n) - 1);
  for (uint32_t s = tid; s <= mask + 1; s += kDictThreads) { keys[s] = kDictEmpty; cnt[s] = 0; }
  if (tid < 2) ctr[tid] = 0;
  __syncthreads();
  for (uint64_t i = tid; i < d.n; i += kDictThreads) dict_insert(keys, cnt, mask, dict_latent(d.src, i, d.dtype));
  __syncthreads();
  for (uint32_t s = tid; s <= mask + 1; s += kDictThreads) {
    const bool used = s <= mask ? keys[s] != kDictEmpty : cnt[s] != 0;
    if (used) ent[atomicAdd(&ctr[0], 1u)] = DictEntry{s <= mask ? keys[s] : kDictEmpty, cnt[s], s};
  }
  __syncthreads();
  const uint32_t k = ctr[0];
  const uint32_t p = (uint32_t)dict_pow2(k);
  for (uint32_t e = k + tid; e < p; e += kDictThreads) ent[e] = DictEntry{kDictEmpty, 0u, 0xffffffffu};   // (count 0: after every real entry)
  __syncthreads();
  // bitonic sort of the p entries (an order with unique keys: the result does not depend on the compaction order)
  for (uint32_t size = 2; size <= p; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t i = tid; i < p / 2; i += kDictThreads) {
        const uint32_t lo = (i / stride) * stride * 2 + (i % stride), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const DictEntry a = ent[lo], b = ent[hi];
        if (dict_before(b, a) == up) { ent[lo] = b; ent[hi] = a; }
      }
      __syncthreads();
    }
  }
  const uint32_t vbytes = (uint32_t)dtype_bits(d.dtype) / 8;
  for (uint32_t r = tid; r < k; r += kDictThreads) {
    const DictEntry e = ent[r];
    cnt[e.slot] = r;
    dict_put_value(d.values, r, e.key, vbytes);
  }
  if (tid == 0) tasks[t].k = k;
  __syncthreads();
  dict_map(d, keys, cnt, mask);
}

// The dictionary bytes into the hole the meta writers left behind the Dict header (BitSink / PackSink::skip): 8 bytes into a standalone
// chunk (preamble 32 bits, header 29 bits padded to the byte), 4 into a ChunkMeta of its own.  Runs after every kernel that writes the
// page, which leave the hole's bytes zero.  grid = pages x blocks_per_page, 256 threads
__global__ __launch_bounds__(256) void enc_dict_place_kernel(EncWorkspace ws, uint32_t n_pages, uint32_t blocks_per_page) {
  const uint32_t p = blockIdx.x / blocks_per_page, b = blockIdx.x % blocks_per_page;
  if (p >= n_pages) return;
  const EncPage pg = ws.pages[p];
  if (!(pg.flags & (kPageFlagPreamble | kPageFlagMetaOnly))) return;
  const EncChunk* ch = ws.chunks + pg.chunk;
  if (ch->status != PCO_GFX_OK || ch->fallback || ch->dict_dtype == 0) return;
  const DictTask d = ws.dict[pg.chunk];
  const uint64_t off = (pg.flags & kPageFlagPreamble) ? 8 : 4, bytes = (uint64_t)d.k * (dtype_bits(d.dtype) / 8);
  if (off + bytes + 8 > pg.dst_cap) return;   // (the page's sink reported the overflow)
  uint8_t* dst = (uint8_t*)pg.dst + off;      // (4-byte aligned: dst is 8-byte aligned)
  const uint64_t nd = bytes / 4;
  for (uint64_t i = (uint64_t)b * 256 + threadIdx.x; i < nd; i += (uint64_t)blocks_per_page * 256) ((uint32_t*)dst)[i] = ((const uint32_t*)d.values)[i];
  if (b == 0 && threadIdx.x < (bytes & 3)) dst[nd * 4 + threadIdx.x] = d.values[nd * 4 + threadIdx.x];
}

}  // namespace pcogfx
