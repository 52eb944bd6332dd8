// scan.hip -- the kernel of pco_gfx_scan_chunks (include/pco_gfx.h section 4m): where the chunks of a standalone stream start, found on the device
// from ONE walk of it that stores no rows.  A .pco file stores no chunk lengths: chunk k + 1 starts where chunk k's bit stream ends, and that end
// follows from the symbols alone -- the bits each tANS state takes and the offset width of each symbol's bin.  So the walk keeps the four chain
// states and the SUM of the offset widths of a batch; it unpacks no offset, adds no lower, runs no delta decode, joins and stores nothing.  (One exception: the lookback variable of a Lookback page, whose values
// the chain judges against the window, is unpacked for that verdict.)
//
// One 64-lane wave per stream, many streams per launch; a wave loops over its stream's chunks.  The ChunkMeta is parsed, validated and turned into
// decoder tables by decode_chunk (decode_kernel.hip) compiled with kScan = true -- a new instantiation: the kernels the other entry points launch
// are what they were -- which hands the page to scan_page_body below in place of a decode body.  The chain is latency-bound (a dependent LDS
// lookup per four symbols), so what a launch gains over a loop of one-chunk decodes is the streams a CU holds side by side and the host round
// trips it does not make.
#pragma once
#include "decode_kernel.hip"
#include "pco_scan.h"

namespace pcogfx {

// A scan node: walk_ans' node with the offset bits of its symbol's bin where the symbol was -- bits 0..13 next_state_idx_base, 14..17 bits_to_read,
// 18..24 the bin's offset bits.  The scan needs no symbol, and one table lookup a step is one LDS round trip less on the chain.
template <bool kLds>
__device__ __forceinline__ void scan_fold_offset_bits(tptr<kLds, uint32_t> nodes, tptr<kLds, uint8_t> obs, uint32_t table_size) {
  for (uint32_t t = lane_id(); t < table_size; t += 64) { const uint32_t node = nodes[t]; nodes[t] = (node & 0x3ffffu) | ((uint32_t)obs[node >> 18] << 18); }
  wave_sync_lds();
}

// walk_ans (decode_kernel.hip) over scan nodes, without the symbol stage: lanes 0..3 walk the four chains and add up the offset bits their nodes
// carry.  A step's window words depend on the bit position alone, so they are asked for TOGETHER with the node, in front of everything that
// waits for either: one LDS round trip a step on the chain.  Returns the new bit position; ob_sum: the batch's offset bits, wave-uniform.
template <bool kLds>
__device__ __forceinline__ uint64_t scan_walk_ans(gcptr_u8 src, uint64_t src_len, uint64_t bitpos, uint32_t cnt, tptr<kLds, uint32_t> nodes, uint32_t& st, uint32_t& ob_sum) {
  const uint32_t lane = lane_id();
  uint32_t PCO_LDS* win = (uint32_t PCO_LDS*)(lds_base() + kLdsWinOff);
  // stage the ANS section: 136 dwords from the dword containing bitpos
  const uint64_t dw0 = bitpos >> 5;
  {
    const uint64_t w = load_u64_le_safe(src, dw0 * 4 + (uint64_t)lane * 8, src_len + 16);
    win[2 * lane] = (uint32_t)w; win[2 * lane + 1] = (uint32_t)(w >> 32);
    if (lane < 4) {
      const uint64_t w2 = load_u64_le_safe(src, dw0 * 4 + 512 + (uint64_t)lane * 8, src_len + 16);
      win[128 + 2 * lane] = (uint32_t)w2; win[128 + 2 * lane + 1] = (uint32_t)(w2 >> 32);
    }
  }
  wave_sync_lds();
  uint32_t rel = (uint32_t)(bitpos & 31);  // bit offset relative to win[0]
  uint32_t acc = 0;
  if (lane < 4) {
    const uint32_t steps = (cnt + 3) >> 2;
    for (uint32_t g = 0; g < steps; g++) {
      const bool act = 4 * g + lane < cnt;
      const uint32_t d = rel >> 5;
      const uint32_t w0 = win[d], w1 = win[d + 1], w2 = win[d + 2], w3 = win[d + 3];
      const uint32_t node = nodes[st];
      __builtin_amdgcn_sched_barrier(0);   // (the five loads stay in front of their first use)
      const uint32_t btr = act ? ((node >> 14) & 15u) : 0u;
      // inclusive prefix of btr over the quad: lanes 0..3 open a DPP row, whose shifts fill with zeros
      uint32_t incl = btr + dpp0<0x111, 0xf>(btr);
      incl += dpp0<0x112, 0xf>(incl);
      const uint32_t excl = incl - btr;
      const uint32_t tot = (uint32_t)__builtin_amdgcn_mov_dpp((int)incl, 0xff /*[3,3,3,3]*/, 0xf, 0xf, false);
      const uint32_t sh = (rel & 31) + excl;  // <= 31 + 42
      const uint32_t sel = sh >> 5;
      const uint32_t lo = sel == 0 ? w0 : (sel == 1 ? w1 : w2);
      const uint32_t hi = sel == 0 ? w1 : (sel == 1 ? w2 : w3);
      const uint32_t bits = __builtin_amdgcn_alignbit(hi, lo, sh & 31);
      const uint32_t val = bits & ((1u << btr) - 1u);
      acc += act ? (node >> 18) : 0u;
      st = act ? (node & 0x3fffu) + val : st;
      rel += tot;
    }
  }
  const uint32_t rel_end = uni(rel);  // lane 0
  ob_sum = (uint32_t)__builtin_amdgcn_readlane((int)acc, 0) + (uint32_t)__builtin_amdgcn_readlane((int)acc, 1) +
           (uint32_t)__builtin_amdgcn_readlane((int)acc, 2) + (uint32_t)__builtin_amdgcn_readlane((int)acc, 3);
  wave_sync_lds();
  return (dw0 << 5) + rel_end;
}

// One page of n numbers walked for its end: the framing of decode_page_body / decode_page_body_dict (decode_kernel.hip), whose two layouts are one
// here -- the variables' latent widths are in their VarInfo -- with every check of theirs that the framing decides, in their order, and the one on the lookback
// variable's values.  The check they make on a row's VALUE -- a Dict index beyond the dictionary -- needs the rows and is not made.
template <bool kLds>
__device__ __noinline__ void scan_page_body(gcptr_u8 src, uint64_t src_len, MetaReader& mr, tptr<kLds, uint8_t> tbl, uint32_t n, uint32_t& status) {
  const uint32_t lane = lane_id();
  VarInfo PCO_LDS* vinfo = (VarInfo PCO_LDS*)(lds_base() + kLdsVarOff);
  uint32_t present[3], n_bins[3], max_ob[3], asl[3], nlps[3], off_nodes[3], off_ob[3];
#pragma unroll
  for (int vi = 0; vi < 3; vi++) {
    present[vi] = uni(vinfo[vi].present); n_bins[vi] = uni(vinfo[vi].n_bins); max_ob[vi] = uni(vinfo[vi].max_ob); asl[vi] = uni(vinfo[vi].ans_size_log);
    off_nodes[vi] = uni(vinfo[vi].off_nodes); off_ob[vi] = uni(vinfo[vi].off_ob);
    const uint32_t dk = uni(vinfo[vi].delta_kind), dord = uni(vinfo[vi].delta_order);
    nlps[vi] = (dk == kDeltaConsecutive || dk == kDeltaConv1) ? dord : (dk == kDeltaLookback ? (1u << uni(vinfo[vi].state_n_log)) : 0u);
  }
  // ---- page meta (metadata/page.rs:36-57): per variable its delta state, skipped by its length, then the four tANS states ----
  uint32_t st[3] = {0, 0, 0};
#pragma unroll
  for (int vi = 0; vi < 3; vi++) {
    if (!present[vi]) continue;
    mr.bit += (uint64_t)nlps[vi] * uni(vinfo[vi].latent_bits);
    uint32_t mine = 0;
    for (uint32_t j = 0; j < 4; j++) { const uint32_t s = (uint32_t)mr.read(asl[vi]); if (lane == j) mine = s; }
    st[vi] = mine;
  }
  if (!mr.drain_empty_byte()) { if (mr.in_bounds()) status = PCO_GFX_CORRUPTION; }
  if (!mr.in_bounds()) { status = PCO_GFX_INSUFFICIENT_DATA; return; }
  if (status) return;
  if (n > nlps[1]) {
#pragma unroll
    for (int vi = 0; vi < 3; vi++) if (present[vi] && n_bins[vi] == 0) { status = PCO_GFX_CORRUPTION; return; }
  }
  wave_sync_lds();
  // the walked variables' tables become scan tables (the lookback variable keeps its symbols: its values are unpacked below)
#pragma unroll
  for (int vi = 1; vi < 3; vi++) if (present[vi] && n_bins[vi] > 1) scan_fold_offset_bits<kLds>((tptr<kLds, uint32_t>)(tbl + off_nodes[vi]), tbl + off_ob[vi], 1u << asl[vi]);
  uint64_t bitpos = mr.bit;
  uint32_t n_remaining = n, lb_oob = 0;
  const uint32_t off_lower0 = uni(vinfo[0].off_lower), window_n = 1u << uni(vinfo[1].window_n_log);
  for (uint32_t j0 = 0; j0 < n; j0 += kBatchN) {
    const uint32_t batch_n = n_remaining < kBatchN ? n_remaining : kBatchN;
#pragma unroll
    for (int vi = 0; vi < 3; vi++) {
      if (!present[vi]) continue;
      uint32_t cnt;
      if (vi == 0) { const uint32_t lim = n_remaining > nlps[1] ? n_remaining - nlps[1] : 0; cnt = lim < batch_n ? lim : batch_n; }
      else { const uint32_t rem = n_remaining > nlps[vi] ? n_remaining - nlps[vi] : 0; cnt = rem < kBatchN ? rem : kBatchN; }
      if (cnt == 0) continue;
      if (vi == 0) {
        // the lookback variable is the one whose VALUES the framing of the page's rows does not need and a verdict does: a lookback beyond the
        // window is corruption (decode_page_body).  Its latents are no rows -- no delta, no join -- so they are unpacked and judged here.
        const bool single_bin = n_bins[0] <= 1;
        if (!single_bin) bitpos = walk_ans<kLds>(src, src_len, bitpos, cnt, (tptr<kLds, uint32_t>)(tbl + off_nodes[0]), st[0]);
        if (max_ob[0] != 0 || !single_bin) {
          uint32_t lb[4];
          bitpos = unpack_offsets<uint32_t, kLds>(src, src_len, bitpos, cnt, (tptr<kLds, uint32_t>)(tbl + off_lower0), tbl + off_ob[0], single_bin, lb);
#pragma unroll
          for (int k = 0; k < 4; k++) if (4 * lane + k < cnt && lb[k] > window_n) lb_oob = 1;
        }
      } else if (n_bins[vi] > 1) {
        uint32_t ob_sum = 0;
        bitpos = scan_walk_ans<kLds>(src, src_len, bitpos, cnt, (tptr<kLds, uint32_t>)(tbl + off_nodes[vi]), st[vi], ob_sum);
        bitpos += ob_sum;
      } else bitpos += (uint64_t)cnt * max_ob[vi];   // one bin: no tANS bits, its offset width for every number
      if (bitpos > src_len * 8) { status = PCO_GFX_INSUFFICIENT_DATA; return; }
    }
    n_remaining -= batch_n;
  }
  if (uni(wave_or_u32(lb_oob))) { status = PCO_GFX_CORRUPTION; return; }
  // trailing bits of the page must be zero (page_decompressor.rs:184-188)
  mr.bit = bitpos;
  if (!mr.drain_empty_byte()) status = PCO_GFX_CORRUPTION;
  if (!mr.in_bounds()) status = PCO_GFX_INSUFFICIENT_DATA;
}

// One wave per task; a task is a standalone stream, with or without its file header and terminator.
__global__ __launch_bounds__(64, kDecMinWaves) void pco_scan_kernel(const PcoGfxScanTask* tasks, PcoGfxTaskResult* results, uint32_t n_tasks, uint32_t lds_table_budget,
                                                                    uint8_t* tbl_ws_base) {
  const uint32_t lane = lane_id();
  gptr_u8 tbl_ws = (gptr_u8)tbl_ws_base + (uint64_t)blockIdx.x * kTblWsBytes;
  for (uint32_t ti = blockIdx.x; ti < n_tasks; ti += gridDim.x) {
    const PcoGfxScanTask task = tasks[ti];
    gcptr_u8 src = (gcptr_u8)task.src;
    const uint64_t src_len = uni((uint64_t)task.src_len);
    const uint32_t dtype = uni(task.dtype), flags = uni(task.flags), max_chunks = uni(task.max_chunks);
    uint64_t PCO_GLOBAL* offsets = (uint64_t PCO_GLOBAL*)task.d_offsets;
    uint32_t PCO_GLOBAL* counts = (uint32_t PCO_GLOBAL*)task.d_counts;
    const ScanBytes bytes{(const uint8_t*)task.src, src_len};
    const bool in_file = (flags & PCO_GFX_TASK_HAS_FILE_HEADER) != 0;
    uint32_t status = PCO_GFX_OK, format_major = 4, uniform_type = 0, k = 0, aux = 0;
    uint64_t pos = 0;   // where the next chunk's preamble stands: the end of the last chunk found
    if (in_file) {
      const ScanHeader h = scan_file_header(bytes);
      status = uni(h.status); format_major = uni(h.format_major); uniform_type = uni(h.uniform_type);
      if (!status) pos = uni(h.len);
    } else if (((flags >> 8) & 0xffu) != 0) format_major = (flags >> 8) & 0xffu;
    while (!status) {
      const bool first = in_file && k == 0;   // the step of the chain that carries the header flag
      const ScanPreamble pre = scan_chunk_preamble(bytes, pos, dtype, first ? uniform_type : 0u, !first);
      status = uni(pre.status);
      const uint32_t kind = uni(pre.kind), n = uni(pre.n);
      if (status || kind == kScanEnd) break;
      if (kind == kScanTerminator) { aux = 2; break; }   // a stream without (further) chunks
      MetaReader mr{src, src_len, (pos + 4) * 8};
      switch (scan_type_bits(dtype)) {
        case 64: decode_chunk<uint64_t, false, false, false, false, true>(src, src_len, mr, lds_table_budget, tbl_ws, format_major, dtype, n, (uint64_t PCO_GLOBAL*)nullptr, status, false); break;
        case 32: decode_chunk<uint32_t, false, false, false, false, true>(src, src_len, mr, lds_table_budget, tbl_ws, format_major, dtype, n, (uint32_t PCO_GLOBAL*)nullptr, status, false); break;
        case 16: decode_chunk<uint16_t, false, false, false, false, true>(src, src_len, mr, lds_table_budget, tbl_ws, format_major, dtype, n, (uint16_t PCO_GLOBAL*)nullptr, status, false); break;
        default: decode_chunk<uint8_t, false, false, false, false, true>(src, src_len, mr, lds_table_budget, tbl_ws, format_major, dtype, n, (uint8_t PCO_GLOBAL*)nullptr, status, false); break;
      }
      status = uni(status);
      wave_sync_lds();
      if (status) break;
      const uint64_t end = uni(mr.bit >> 3);
      const ScanBehind behind = scan_behind_chunk(bytes, end, first);
      status = uni(behind.status);
      if (status) break;   // (a file that ends behind its first chunk: the chain's step fails, and the chunk with it)
      if (lane == 0) { offsets[k] = pos; counts[k] = n; }
      k++; pos = end; aux = uni(behind.aux);
      if (aux != 1u || k == max_chunks) break;
    }
    if (status) aux = 0;
    if (lane == 0) {
      offsets[k] = pos;
      PcoGfxTaskResult r; r.n_out = k; r.consumed = pos + ((aux & 2u) ? 1u : 0u); r.status = status; r.aux = aux | (format_major << 8);
      results[ti] = r;
    }
  }
}

}  // namespace pcogfx
