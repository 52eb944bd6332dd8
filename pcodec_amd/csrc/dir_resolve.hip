// dir_resolve.hip -- pco_gfx_decompress_pages_dir / pco_gfx_decompress_page_ranges_dir (include/pco_gfx.h section 4e): the page directory of a
// decode call lives in DEVICE memory (the d_offsets pco_gfx_compact_wrapped_chunks wrote), so the host uploads its decode tasks with null
// sources plus each task's pair of piece indices, and ONE small kernel, queued on the caller's stream between the task upload and the first
// decode kernel, turns the indices into the pointers and lengths every decode kernel reads from the workspace's task array anyway.
//
// How a refused task (pco_dir.h) stays away from the blob and from dst, without a change to any decode kernel:
//   PCO_GFX_INVALID_ARGUMENT   the DEVICE copy of the task gets dtype 0: the walkers' front hands it to the single-kernel decoder, which answers
//                              {PCO_GFX_INVALID_ARGUMENT, n_out 0, consumed 0, aux 0} before it reads anything (the host grouped the task by its
//                              real dtype before the upload; the second pass of a synchronous call never sees it);
//   PCO_GFX_INSUFFICIENT_DATA  a ChunkMeta of 0 bytes: the first metadata read is out of bounds, and MetaReader reads nothing beyond its length.
// Either way the source lengths are 0 and the pointers are the blob's first byte.
//
// pco_gfx_decompress_chunks_dir / pco_gfx_decompress_chunk_reads_dir / pco_gfx_index_chunks_dir (section 4l): the pieces are the STANDALONE chunks behind
// pco_gfx_compact_chunks' offsets.  dir_resolve_chunks_kernel / dir_resolve_chunks_reads_kernel split each task's chunk into its ChunkMeta and its one
// page (pco_chunk_dir.h), and everything behind them sees a wrapped page.  A chunk verdict has one more refusal:
//   PCO_GFX_CORRUPTION         a ChunkMeta of ONE byte in the call's task buffer that holds the unknown mode nibble 15: the first metadata read is in
//                              bounds and names no mode, which every decoder answers with Corruption before it reads anything else.
#pragma once
#include "pco_host.h"
#include "pco_dev.h"
#include "pco_dir.h"
#include "pco_chunk_dir.h"
#include "decode_kernel.hip"   // PcoGfxDecodeTask's device readers: MetaRef, RangeRef

#include <string>

namespace pcogfx {

struct DirPieces { uint32_t meta_piece, page_piece; };
static_assert(sizeof(DirPieces) == 8, "DirPieces");
struct DirArgs { const uint8_t* blob; uint64_t blob_len; const uint64_t* offsets; uint64_t n_pieces; uint32_t gap; };
// what launch_decode / launch_partial take as their optional directory argument: the directory, and the HOST array of piece pairs
// chunks: the pieces are standalone chunks (section 4l), and the chunk kernels below resolve them
struct DirLaunch { DirArgs args; const DirPieces* pieces; bool chunks = false; };

// one thread per task.  kRange: a task with count == 0 reads nothing and is PCO_GFX_OK whatever its pieces look like (the range kernels
// answer it before they look at the task), so it takes no verdict.
template <bool kRange>
__global__ __launch_bounds__(256) void dir_resolve_kernel(PcoGfxDecodeTask* tasks, MetaRef* metas, const DirPieces* pieces, const RangeRef* ranges, uint32_t n_tasks, DirArgs dir) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  DirVerdict v{dir.blob, 0, dir.blob, 0, kDirOk};
  bool empty = false;
  if constexpr (kRange) empty = as_global(ranges)[i].count == 0;
  if (!empty) {
    const uint64_t PCO_GLOBAL* off = as_global(dir.offsets);
    const DirPieces pc{as_global(pieces)[i].meta_piece, as_global(pieces)[i].page_piece};   // (both indices < n_pieces: checked by the host, so every read below is inside the n_pieces + 1 entries)
    v = dir_verdict(dir.blob, dir.blob_len, dir.gap, off[dir.n_pieces], off[pc.meta_piece], off[(uint64_t)pc.meta_piece + 1], off[pc.page_piece], off[(uint64_t)pc.page_piece + 1]);
  }
  PcoGfxDecodeTask PCO_GLOBAL* t = as_global(tasks) + i;
  t->src = v.page; t->src_len = v.page_len;
  if (v.status == kDirInvalidArgument) t->dtype = 0;
  MetaRef PCO_GLOBAL* m = as_global(metas) + i;
  m->p = v.meta; m->len = v.meta_len;   // (never nullptr: that would mean "the ChunkMeta is in front of the page")
}

// dir_resolve_kernel<true> for the READ tasks of pco_gfx_decompress_page_reads_dir (section 4k).  A read call has one more thing on the device that a
// refused task must not reach: its cursor references.  The resume expander judges the `from` cursor of every task the walkers hand back -- which is
// where both refusals above send a task -- and would read it, and answer with ITS verdict; so a refused task's DEVICE copy of the pair becomes
// {nullptr, nullptr}: a read from the page's start that leaves no cursor, which then fails as above, with nothing of `from` read and nothing of `to`
// written.  (Its history reference needs no such care: a history's header is read after the ChunkMeta and the page header are parsed, and a refused
// task gets to neither.  Nor does an index task: its cursor slots and histories are written under PCO_GFX_OK alone, and it runs dir_resolve_kernel.)
// This kernel runs in front of reads_shadow_kernel / reads_rows_kernel, which read the device copy too.
struct DirCursorPair { uint64_t* from; uint64_t* to; };   // (ReadRef's layout, decode_fast.hip: checked where the kernel is launched)
template <bool kRange>
__global__ __launch_bounds__(256) void dir_resolve_reads_kernel(PcoGfxDecodeTask* tasks, MetaRef* metas, const DirPieces* pieces, const RangeRef* ranges, uint32_t n_tasks, DirArgs dir,
                                                                DirCursorPair* cursors) {
  static_assert(kRange, "a read task is a range task");
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  DirVerdict v{dir.blob, 0, dir.blob, 0, kDirOk};
  if (as_global(ranges)[i].count != 0) {
    const uint64_t PCO_GLOBAL* off = as_global(dir.offsets);
    const DirPieces pc{as_global(pieces)[i].meta_piece, as_global(pieces)[i].page_piece};   // (both indices < n_pieces: checked by the host)
    v = dir_verdict(dir.blob, dir.blob_len, dir.gap, off[dir.n_pieces], off[pc.meta_piece], off[(uint64_t)pc.meta_piece + 1], off[pc.page_piece], off[(uint64_t)pc.page_piece + 1]);
  }
  PcoGfxDecodeTask PCO_GLOBAL* t = as_global(tasks) + i;
  t->src = v.page; t->src_len = v.page_len;
  if (v.status == kDirInvalidArgument) t->dtype = 0;
  MetaRef PCO_GLOBAL* m = as_global(metas) + i;
  m->p = v.meta; m->len = v.meta_len;
  if (v.status != kDirOk) { DirCursorPair PCO_GLOBAL* c = as_global(cursors) + i; c->from = nullptr; c->to = nullptr; }
}

// The same two kernels for the tasks of section 4l: a task's one piece (DirPieces::page_piece; the host saw that meta_piece equals it) is a standalone
// chunk, and chunk_verdict says where its ChunkMeta and its page are.  The task's dtype, n and format version are read from its device copy.
// bad_meta: 16 bytes of the call's task buffer for the refusal by Corruption (above); every thread that refuses so writes the same byte.
constexpr uint8_t kUnknownModeNibble = 0x0f;
__device__ inline uint32_t dir_resolve_chunk_task(PcoGfxDecodeTask* tasks, MetaRef* metas, const DirPieces* pieces, uint32_t i, bool empty, const DirArgs& dir, uint8_t* bad_meta) {
  DirVerdict v{dir.blob, 0, dir.blob, 0, kDirOk};
  PcoGfxDecodeTask PCO_GLOBAL* t = as_global(tasks) + i;
  if (!empty) {
    const uint64_t PCO_GLOBAL* off = as_global(dir.offsets);
    const uint32_t k = as_global(pieces)[i].page_piece;   // (< n_pieces: checked by the host, so every read below is inside the n_pieces + 1 entries)
    v = chunk_verdict(dir.blob, dir.blob_len, dir.gap, off[dir.n_pieces], off[k], off[(uint64_t)k + 1], t->dtype, t->dst_cap, (t->flags >> 8) & 0xffu);
  }
  if (v.status == kDirCorruption) { as_global(bad_meta)[0] = kUnknownModeNibble; v.meta = bad_meta; v.meta_len = 1; }
  t->src = v.page; t->src_len = v.page_len;
  if (v.status == kDirInvalidArgument) t->dtype = 0;
  MetaRef PCO_GLOBAL* m = as_global(metas) + i;
  m->p = v.meta; m->len = v.meta_len;
  return v.status;
}
template <bool kRange>
__global__ __launch_bounds__(256) void dir_resolve_chunks_kernel(PcoGfxDecodeTask* tasks, MetaRef* metas, const DirPieces* pieces, const RangeRef* ranges, uint32_t n_tasks, DirArgs dir,
                                                                 uint8_t* bad_meta) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  bool empty = false;
  if constexpr (kRange) empty = as_global(ranges)[i].count == 0;
  dir_resolve_chunk_task(tasks, metas, pieces, i, empty, dir, bad_meta);
}
template <bool kRange>
__global__ __launch_bounds__(256) void dir_resolve_chunks_reads_kernel(PcoGfxDecodeTask* tasks, MetaRef* metas, const DirPieces* pieces, const RangeRef* ranges, uint32_t n_tasks, DirArgs dir,
                                                                       uint8_t* bad_meta, DirCursorPair* cursors) {
  static_assert(kRange, "a read task is a range task");
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tasks) return;
  const uint32_t status = dir_resolve_chunk_task(tasks, metas, pieces, i, as_global(ranges)[i].count == 0, dir, bad_meta);
  if (status != kDirOk) { DirCursorPair PCO_GLOBAL* c = as_global(cursors) + i; c->from = nullptr; c->to = nullptr; }   // (as dir_resolve_reads_kernel)
}

// the host checks both entry points share; `who`: "page" / "page range"
inline DirArgs checked_directory(const PcoGfxDirectory* dir, const char* who) {
  if (!dir || !dir->d_blob || !dir->d_offsets) throw HostError{PCO_GFX_INVALID_ARGUMENT, std::string(who) + " directory: null directory, blob or offsets"};
  if (dir->n_pieces >= (1ull << 31)) throw HostError{PCO_GFX_INVALID_ARGUMENT, std::string(who) + " directory: fewer than 2^31 pieces"};
  return DirArgs{(const uint8_t*)dir->d_blob, dir->blob_len, dir->d_offsets, dir->n_pieces, dir->gap};
}
inline void check_piece_pair(uint32_t meta_piece, uint32_t page_piece, uint64_t n_pieces, const std::string& who) {
  if (meta_piece >= n_pieces || page_piece >= n_pieces) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": piece index beyond the directory"};
  if (meta_piece == page_piece) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": the ChunkMeta and the page are one piece"};
}
// ... and of a chunk task: one piece, named twice
inline void check_chunk_piece(uint32_t meta_piece, uint32_t page_piece, uint64_t n_pieces, const std::string& who) {
  if (meta_piece >= n_pieces || page_piece >= n_pieces) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": piece index beyond the directory"};
  if (meta_piece != page_piece) throw HostError{PCO_GFX_INVALID_ARGUMENT, who + ": a standalone chunk is one piece; meta_piece must equal page_piece"};
}

}  // namespace pcogfx
