// =============================================================================
// pco_oracle_testenc.hpp -- ORACLE (test infrastructure): a TEST-ONLY stream generator.
//
// NOT a restatement of the reference's encoder.  The reference can write chunks the restated
// encoder (pco_oracle_encode.hpp) does not: Dict mode (mode/dict.rs:12-33), Conv1 delta
// (delta/conv1.rs:424-461), and the format allows more than any encoder writes (a secondary
// variable that is delta'd too, lookback state_n_log > 0: metadata/delta_encoding.rs:86-99).
// Decoding is deterministic, so ANY valid stream exercises the decoders; this file writes such
// streams from a caller-chosen spec (dictionary order, lookbacks, Conv1 weights) with the format
// writers of pco_oracle.hpp and the restated bin training / tANS machinery -- and, on request, with
// the trained table reshaped into a FOREIGN one (test_reshape_table: any ans_size_log up to 14, weights
// no quantize_weights produces, split / duplicated / shuffled bins, widened offsets, wrapped lowers),
// or with one named invalid table header (TblFault).  The decode side
// they are checked against (pco_oracle_decode.hpp) IS a restatement and is pinned by the
// reference's own v1_0_0_dict.pco / v1_0_0_conv1.pco assets.
// Only tests/ may reach this (through pco_oracle_capi.cpp); the product never does.
// =============================================================================
#pragma once
#include "pco_oracle_encode.hpp"
#include <memory>

namespace pco_oracle {

struct TestEncSpec {
  uint32_t mode_kind;           // ModeSpecKind numbering: 1 classic, 2 float mult (mode_f64), 3 float quant (mode_u64), 4 int mult (mode_u64), 5 dict
  uint32_t delta_kind;          // DeltaKind: 0 none, 1 consecutive, 2 lookback, 3 conv1
  double mode_f64;
  uint64_t mode_u64;
  uint32_t order;               // consecutive order / number of Conv1 weights
  uint32_t secondary_uses_delta;
  uint32_t window_n_log, state_n_log;
  uint32_t lookback_seed;       // 0: choose_lookbacks (the reference's search); else random valid lookbacks from this seed
  uint32_t quantization;
  int64_t bias;
  int32_t weights[32];
  uint32_t level;
  uint32_t dict_first_appearance;  // dictionary in first-appearance order instead of sorted
  // ---- foreign tables: reshape the TRAINED table of the selected variables into one that is legal but that no training produces.
  //      All zero = the trained table, byte for byte.  What cannot be written validly is refused (InvalidArgument).
  uint32_t tbl_vars;          // which variables: bit 0 delta, bit 1 primary (Dict's u32 primary too), bit 2 secondary; absent ones are skipped
  uint32_t tbl_ans_size_log;  // 0: the trained value, raised to what the bins need; 1..14: exactly this; kTblAnsMin (255): the smallest that fits n_bins
  uint32_t tbl_n_bins;        // 0: the trained bins; 1: ONE bin over all latents (ans_size_log 0); else raise the count to this (<= 2^14) by
                              //    splitting bins at data values and by duplicating bins over the same range
  uint32_t tbl_weight_style;  // TblWeights: 0 proportional to the counts, 1 flat, 2 inverse (every bin 1, the RAREST bin the rest), 3 all 1 (needs
                              //    n_bins == 2^ans_size_log), 4 seeded random.  Always positive, always summing to 2^ans_size_log
  uint32_t tbl_ob_mode;       // TblOffsets: 0 tight, 1 every bin max(needed, tbl_ob_value), 2 seeded random in [needed, BITS], 3 every other bin
                              //    BITS wide and the rest tight, 4 ONE seeded bin max(needed, tbl_ob_value) and the rest tight
  uint32_t tbl_ob_value;      // <= the latent's BITS
  uint32_t tbl_lower_wrap;    // 1: move the lower of every widened bin down (mod 2^BITS) as far as its offset bits allow, seeded, so that
                              //    lower.wrapping_add(offset) wraps where lower was small (never on the lookback variable: its lowers are bounded)
  uint32_t tbl_shuffle;       // 1: the bins in seeded random order in the metadata
  uint32_t tbl_seed;
  uint32_t tbl_fault;         // TblFault: ONE invalid table header on tbl_fault_var (0 delta, 1 primary, 2 secondary); the body is not meant to be read
  uint32_t tbl_fault_var;
  uint32_t tbl_reserved;
};
constexpr uint32_t kTblAnsMin = 255;
enum TblFault { kTblFaultNone = 0, kTblFaultWeightsBelow = 1, kTblFaultWeightsAbove = 2, kTblFaultOneBinWithAns = 3, kTblFaultAnsTooSmall = 4,
                kTblFaultAns15 = 5, kTblFaultOffsetBits = 6, kTblFaultNoBins = 7 };

// The bins of a reshaped table may overlap, repeat and come in any order, so the trained table's search (compression_table.rs:51-74, sorted
// disjoint bins) cannot assign them: `forced` names the bin (its index in the metadata) of every latent, and dissect_page follows it.
template <class V> struct TestVar : LatentCompressor<V> {
  std::vector<uint32_t> forced;   // per position of `latents`; empty = the trained table and its search
  DissectedVar dissect_page(size_t start, size_t end) const {
    if (forced.empty()) return LatentCompressor<V>::dissect_page(start, end);
    DissectedVar d; for (int j = 0; j < 4; j++) d.ans_final_states[j] = this->encoder.default_state();
    if (this->is_trivial) return d;
    const size_t page_n = end - start;
    d.ans_vals.assign(page_n, 0); d.ans_bits.assign(page_n, 0); d.offset_bits.assign(page_n, 0); d.offsets.assign(page_n, 0);
    for (size_t b = (page_n + FULL_BATCH_N - 1) / FULL_BATCH_N; b-- > 0;) {
      const size_t rs = b * FULL_BATCH_N, re = std::min(rs + FULL_BATCH_N, page_n);
      for (size_t i = re; i-- > rs;) {   // encode_ans_in_reverse (chunk_latent_compressor.rs:96-132): chain i mod 4 within the batch, i descending
        const uint32_t sym = forced[start + i]; const DynBin& bin = this->meta.bins[sym];
        d.offset_bits[i] = bin.offset_bits; d.offsets[i] = (uint64_t)(V)(this->latents[start + i] - (V)bin.lower);
        if (this->encoder.size_log == 0) continue;
        const size_t j = (i - rs) % ANS_INTERLEAVING; uint32_t ns; Bitlen bits;
        this->encoder.encode(d.ans_final_states[j], sym, ns, bits);
        d.ans_vals[i] = d.ans_final_states[j] & ((1u << bits) - 1); d.ans_bits[i] = bits; d.ans_final_states[j] = ns;
      }
    }
    return d;
  }
};

// Reshape the trained table `t` of one variable by `spec` (see TestEncSpec) and assign every body latent (the positions in `ranges` of `lat`)
// to a bin that covers it.  Returns the bin of every position (empty when the variable has no latents: its table stays empty).
template <class V> std::vector<uint32_t> test_reshape_table(TrainedBins<V>& t, const std::vector<V>& lat, const std::vector<std::pair<size_t, size_t>>& ranges,
                                                            const TestEncSpec& spec, bool is_delta_var) {
  constexpr Bitlen BITS = LT<V>::BITS;
  std::vector<V> S; for (auto& r : ranges) S.insert(S.end(), lat.begin() + r.first, lat.begin() + r.second);
  if (S.empty() || t.infos.empty()) return {};
  std::sort(S.begin(), S.end());
  std::vector<V> D(S); D.erase(std::unique(D.begin(), D.end()), D.end());
  Xoroshiro128PlusPlus rng(0x7ab1e5ull + spec.tbl_seed);
  struct Piece { V lo, hi; size_t a, b; uint32_t dups; size_t count; };   // D[a..b) are its distinct values
  auto piece = [&](V lo, V hi) {
    Piece p{lo, hi, (size_t)(std::lower_bound(D.begin(), D.end(), lo) - D.begin()), (size_t)(std::upper_bound(D.begin(), D.end(), hi) - D.begin()), 1, 0};
    p.count = (size_t)(std::upper_bound(S.begin(), S.end(), hi) - std::lower_bound(S.begin(), S.end(), lo));
    return p;
  };
  std::vector<Piece> pieces;
  const size_t trained_n = t.infos.size();
  if (spec.tbl_n_bins == 1) pieces.push_back(piece(S.front(), S.back()));
  else {
    std::vector<BinCompressionInfo<V>> sorted(t.infos);
    std::sort(sorted.begin(), sorted.end(), [](const BinCompressionInfo<V>& x, const BinCompressionInfo<V>& y) { return x.lower < y.lower; });
    for (auto& i : sorted) pieces.push_back(piece(i.lower, i.upper));
    for (size_t k = 0; k + 1 < pieces.size(); k++) if (pieces[k].hi >= pieces[k + 1].lo) fail(kInvalidArgument, "trained bins overlap");
    if (S.front() < pieces.front().lo || S.back() > pieces.back().hi) fail(kInvalidArgument, "trained bins do not cover the latents");
  }
  if (spec.tbl_n_bins > 1) {
    if (spec.tbl_n_bins > (1u << MAX_ANS_BITS)) fail(kInvalidArgument, "tbl_n_bins beyond 2^14");
    if (spec.tbl_n_bins < pieces.size()) fail(kInvalidArgument, "tbl_n_bins below the trained bin count (the count is forced upward only)");
    size_t extra = spec.tbl_n_bins - pieces.size();
    // splits first (a seeded share of the extra bins, as far as the distinct values go), always at a data value, so both halves hold latents
    size_t n_splits = std::min(extra, D.size() - pieces.size()) * (1 + rng.next_u64() % 4) / 4;
    auto less = [&](size_t x, size_t y) { return pieces[x].b - pieces[x].a < pieces[y].b - pieces[y].a; };
    std::vector<size_t> heap(pieces.size()); for (size_t k = 0; k < heap.size(); k++) heap[k] = k;
    std::make_heap(heap.begin(), heap.end(), less);
    for (; n_splits > 0; n_splits--, extra--) {
      std::pop_heap(heap.begin(), heap.end(), less); const size_t k = heap.back();
      Piece p = pieces[k];
      if (p.b - p.a < 2) break;
      const size_t m = p.a + 1 + rng.next_u64() % (p.b - p.a - 1);   // D[m] opens the upper half
      pieces[k] = piece(p.lo, D[m - 1]); pieces.push_back(piece(D[m], p.hi));
      std::push_heap(heap.begin(), heap.end(), less);
      heap.push_back(pieces.size() - 1); std::push_heap(heap.begin(), heap.end(), less);
    }
    // duplicates: round after round one more copy of every piece that still has more latents than copies
    while (extra > 0) {
      bool any = false;
      for (size_t k = 0; k < pieces.size() && extra > 0; k++) if (pieces[k].count > pieces[k].dups) { pieces[k].dups++; extra--; any = true; }
      if (!any) { pieces[0].dups += (uint32_t)extra; extra = 0; }   // more bins than latents: the rest cannot be used
    }
  }
  std::sort(pieces.begin(), pieces.end(), [](const Piece& x, const Piece& y) { return x.lo < y.lo; });
  // the bins, in sorted order for now: piece k owns first[k] .. first[k + 1]
  std::vector<size_t> first(pieces.size() + 1, 0);
  for (size_t k = 0; k < pieces.size(); k++) first[k + 1] = first[k] + pieces[k].dups;
  const size_t N = first.back();
  const bool reshaped = N != trained_n || spec.tbl_n_bins == 1;
  const Bitlen min_log = N <= 1 ? 0 : ilog2_u64(N - 1) + 1;
  Bitlen asl;
  if (spec.tbl_ans_size_log == 0) asl = N == 1 ? 0 : std::max(min_log, t.ans_size_log);
  else if (spec.tbl_ans_size_log == kTblAnsMin) asl = min_log;
  else {
    if (N == 1) fail(kInvalidArgument, "one bin takes ans_size_log 0");
    if (spec.tbl_ans_size_log < min_log || spec.tbl_ans_size_log > MAX_ANS_BITS) fail(kInvalidArgument, "tbl_ans_size_log does not fit n_bins or exceeds 14");
    asl = spec.tbl_ans_size_log;
  }
  std::vector<BinCompressionInfo<V>> bins(N); std::vector<uint32_t> counts(N);
  for (size_t k = 0; k < pieces.size(); k++) for (size_t j = first[k]; j < first[k + 1]; j++) {
    bins[j] = BinCompressionInfo<V>{1, pieces[k].lo, pieces[k].hi, bits_to_encode_offset<V>((V)(pieces[k].hi - pieces[k].lo)), 0};
    counts[j] = (uint32_t)((pieces[k].count + (j - first[k])) / pieces[k].dups);   // the piece's latents shared out among its copies
  }
  // weights: positive, summing to 2^asl
  const uint32_t T = 1u << asl;
  std::vector<uint32_t> w(N, 1);
  if (N == 1) w[0] = 1;
  else switch (spec.tbl_weight_style) {
    case 0:
      if (!reshaped && asl == t.ans_size_log) { std::sort(t.infos.begin(), t.infos.end(), [](const BinCompressionInfo<V>& x, const BinCompressionInfo<V>& y) { return x.lower < y.lower; });
        for (size_t j = 0; j < N; j++) w[j] = t.infos[j].weight; }
      else w = quantize_weights_to(counts, S.size(), asl);
      break;
    case 1: for (size_t j = 0; j < N; j++) w[j] = T / (uint32_t)N + (j < T % N ? 1 : 0); break;
    case 2: { size_t rare = 0; for (size_t j = 1; j < N; j++) if (counts[j] < counts[rare]) rare = j; w[rare] = T - (uint32_t)(N - 1); break; }
    case 3: if (N != T) fail(kInvalidArgument, "all-ones weights need n_bins == 2^ans_size_log"); break;
    case 4: { uint32_t rem = T - (uint32_t)N;
      while (rem > 0) { const uint64_t r = rng.next_u64(); const uint32_t part = (r & 7) == 0 ? rem : 1 + (uint32_t)((r >> 8) % rem) / (1 + (uint32_t)((r >> 3) & 31)); w[(r >> 40) % N] += part; rem -= part; }
      break; }
    default: fail(kInvalidArgument, "tbl_weight_style");
  }
  uint64_t sum = 0; for (size_t j = 0; j < N; j++) { if (w[j] == 0) fail(kInvalidArgument, "a weight of zero"); sum += w[j]; }
  if (sum != T) fail(kInvalidArgument, "weights do not sum to 2^ans_size_log");
  // offset bits, then lowers
  if (spec.tbl_ob_value > BITS) fail(kInvalidArgument, "tbl_ob_value beyond the latent's bits");
  if (spec.tbl_lower_wrap && is_delta_var) fail(kInvalidArgument, "the lookback variable's lowers are bounded by the window: no wrapped lower there");
  const size_t one = (size_t)(rng.next_u64() % N);
  for (size_t j = 0; j < N; j++) {
    Bitlen& ob = bins[j].offset_bits; const Bitlen needed = ob;
    switch (spec.tbl_ob_mode) {
      case 0: break;
      case 1: ob = std::max(needed, (Bitlen)spec.tbl_ob_value); break;
      case 2: ob = needed + (Bitlen)(rng.next_u64() % (BITS - needed + 1)); break;
      case 3: if (j % 2 == 0) ob = BITS; break;
      case 4: if (j == one) ob = std::max(needed, (Bitlen)spec.tbl_ob_value); break;
      default: fail(kInvalidArgument, "tbl_ob_mode");
    }
    if (spec.tbl_lower_wrap && ob > needed) {   // the highest offset must still fit ob bits: lower may go down by up to 2^ob - 1 - (hi - lo)
      const uint64_t span = (uint64_t)(V)(bins[j].upper - bins[j].lower);
      const uint64_t room = (ob >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << ob) - 1)) - span;
      const uint64_t r = rng.next_u64();
      const uint64_t down = (r & 1) ? room : (room == ~(uint64_t)0 ? (r >> 1) : (r >> 1) % (room + 1));
      bins[j].lower = (V)(bins[j].lower - (V)down);   // `upper` keeps the real range (only `lower` and `offset_bits` are written)
    }
  }
  // order in the metadata
  std::vector<uint32_t> where(N); for (size_t j = 0; j < N; j++) where[j] = (uint32_t)j;   // sorted index -> metadata index
  if (spec.tbl_shuffle) for (size_t j = N; j-- > 1;) std::swap(where[j], where[(size_t)(rng.next_u64() % (j + 1))]);
  t.infos.assign(N, BinCompressionInfo<V>{}); t.counts.assign(N, 0);
  for (size_t j = 0; j < N; j++) { bins[j].weight = w[j]; bins[j].symbol = where[j]; t.infos[where[j]] = bins[j]; t.counts[where[j]] = counts[j]; }
  t.ans_size_log = asl;
  // assignment: a latent of a multiply covered range goes to a copy nobody has used yet, else to a seeded one
  std::vector<uint32_t> forced(lat.size(), 0); std::vector<uint32_t> used(pieces.size(), 0);
  for (auto& r : ranges) for (size_t i = r.first; i < r.second; i++) {
    const V x = lat[i];
    size_t k = (size_t)(std::upper_bound(pieces.begin(), pieces.end(), x, [](V v, const Piece& p) { return v < p.lo; }) - pieces.begin());
    if (k == 0 || x > pieces[k - 1].hi) fail(kInvalidArgument, "a latent that no bin covers");
    k--;
    const uint32_t c = used[k] < pieces[k].dups ? used[k]++ : (uint32_t)(rng.next_u64() % pieces[k].dups);
    forced[i] = where[first[k] + c];
  }
  return forced;
}

// Conv1 residuals in place (delta/conv1.rs:424-461 semantics, :148-161 predict_one): latents[i] -= prediction(latents[i-order..i]), + MID;
// returns the state (the first `order` latents, zero-padded when the page is shorter).  The prediction arithmetic is the decoder's.
template <class P> std::vector<P> test_conv1_encode_in_place(const LatentVarDelta& d, P* latents, size_t len) {
  if (LT<P>::BITS > 32) fail(kInvalidArgument, "Conv1 needs a latent type of at most 32 bits");
  const int conv_bits = LT<P>::BITS == 32 ? 64 : 2 * LT<P>::BITS;
  auto wrap = [&](uint64_t x) -> int64_t { return conv_bits == 64 ? (int64_t)x : (int64_t)(x << ((64 - conv_bits) & 63)) >> ((64 - conv_bits) & 63); };
  const size_t order = d.weights.size();
  std::vector<P> state(order, 0);
  for (size_t i = 0; i < std::min(order, len); i++) state[i] = latents[i];
  for (size_t i = len; i-- > order;) {
    uint64_t sum = (uint64_t)wrap((uint64_t)d.bias);
    for (size_t k = 0; k < order; k++) sum += (uint64_t)wrap((uint64_t)d.weights[k]) * (uint64_t)latents[i - order + k];
    int64_t s = wrap(sum); if (s < 0) s = 0;
    latents[i] = (P)(latents[i] - (P)(uint64_t)(s >> d.quantization) + MID<P>());
  }
  return state;
}

template <class L, class P> struct TestChunk {
  ChunkMeta meta; uint8_t dtype = 0;
  TestVar<uint32_t> dvar; TestVar<P> pvar; TestVar<L> svar;
  struct PageInfo { size_t page_n; PageVarInfo v[3]; };
  std::vector<PageInfo> page_infos;
  int fault_var = -1; LatentVarMeta fault_meta;   // tbl_fault: what the metadata says of that variable instead of its real table
  void write_var_metas(BitWriter& w) const { for (int v = 0; v < 3; v++) if (meta.vars[v].present) write_latent_var_meta(v == fault_var ? fault_meta : meta.vars[v], w); }

  void write_page(size_t page_idx, BitWriter& w) const {   // (the layout of wrapped/chunk_compressor.rs:659-705)
    const PageInfo& pi = page_infos[page_idx];
    DissectedVar dd, dp, ds;
    if (dvar.present) dd = dvar.dissect_page(pi.v[0].start, pi.v[0].end);
    dp = pvar.dissect_page(pi.v[1].start, pi.v[1].end);
    if (svar.present) ds = svar.dissect_page(pi.v[2].start, pi.v[2].end);
    auto write_var_meta = [&](const PageVarInfo& v, const DissectedVar& d, int latent_bits, Bitlen ans_size_log, uint32_t default_state) {
      for (uint64_t x : v.delta_state) w.write_uint(x, (Bitlen)latent_bits);
      for (int j = 0; j < 4; j++) w.write_uint(d.ans_final_states[j] - default_state, ans_size_log);
    };
    if (dvar.present) write_var_meta(pi.v[0], dd, 32, dvar.encoder.size_log, dvar.encoder.default_state());
    write_var_meta(pi.v[1], dp, LT<P>::BITS, pvar.encoder.size_log, pvar.encoder.default_state());
    if (svar.present) write_var_meta(pi.v[2], ds, LT<L>::BITS, svar.encoder.size_log, svar.encoder.default_state());
    w.finish_byte();
    for (size_t batch_start = 0; batch_start < pi.page_n; batch_start += FULL_BATCH_N) {
      if (dvar.present) dvar.write_dissected_batch(dd, batch_start, w);
      pvar.write_dissected_batch(dp, batch_start, w);
      if (svar.present) svar.write_dissected_batch(ds, batch_start, w);
    }
    w.finish_byte();
  }
};

// Conv1 delta encoding in the ChunkMeta (metadata/delta_encoding.rs:239-252); write_delta_encoding refuses it (no restated encoder).
inline void test_write_delta_encoding(const DeltaEncoding& d, BitWriter& w) {
  if (d.kind != kDeltaConv1) { write_delta_encoding(d, w); return; }
  w.write_uint(3, BITS_TO_ENCODE_DELTA_ENCODING_VARIANT);
  w.write_uint(d.quantization, BITS_TO_ENCODE_DELTA_CONV_QUANTIZATION);
  w.write_uint((uint64_t)d.bias ^ ((uint64_t)1 << 63), 64);
  w.write_uint(d.weights.size() - 1, BITS_TO_ENCODE_DELTA_CONV_N_WEIGHTS);
  for (int64_t x : d.weights) w.write_uint((uint64_t)((uint32_t)(int32_t)x ^ 0x80000000u), 32);
}

template <class L, class P> void test_build_chunk(TestChunk<L, P>& tc, std::vector<P> primary, std::vector<L> secondary, bool has_secondary,
                                                  const std::vector<size_t>& pages, const Mode& mode, const DeltaEncoding& de, const TestEncSpec& spec, uint8_t dtype) {
  tc = TestChunk<L, P>(); tc.dtype = dtype;
  const size_t n = primary.size();
  const Bitlen ubl = choose_unoptimized_bins_log(spec.level, n);
  std::vector<uint32_t> delta_latents;
  const LatentVarDelta dprim = delta_for_latent_var(de, kVarPrimary), dsec = delta_for_latent_var(de, kVarSecondary);
  Xoroshiro128PlusPlus rng(spec.lookback_seed);
  size_t start_idx = 0;
  for (size_t page_n : pages) {
    const size_t end_idx = start_idx + page_n;
    typename TestChunk<L, P>::PageInfo pi; pi.page_n = page_n;
    std::vector<uint32_t> lbs;
    if (de.kind == kDeltaLookback) {
      const size_t state_n = (size_t)1 << de.state_n_log, window_n = (size_t)1 << de.window_n_log;
      // (lookback.rs:166-185 pads a short page's state at the front and the decoder returns the first n state slots: unwritable)
      if (page_n < state_n) fail(kInvalidArgument, "a page shorter than the lookback state cannot be represented");
      if (spec.lookback_seed == 0) lbs = choose_lookbacks<P>(de.window_n_log, de.state_n_log, primary.data() + start_idx, page_n);
      else if (page_n > state_n) {   // any lookback in [1, min(window_n, i)] is valid for element i (lookback.rs:166-185 reads latents[i - lookback])
        lbs.resize(page_n - state_n);
        for (size_t i = state_n; i < page_n; i++) {
          const uint64_t r = rng.next_u64(); const size_t lim = std::min(window_n, i);
          // a mix of short, repeated and far lookbacks, the window's far end included
          size_t lb = (r & 3) == 0 ? 1 + (r >> 8) % lim : ((r & 3) == 1 ? lim : 1 + (r >> 8) % std::min<size_t>(lim, 7));
          lbs[i - state_n] = (uint32_t)lb;
        }
      }
    }
    auto encode_var = [&](auto& v, const LatentVarDelta& d, PageVarInfo& out) {
      typedef typename std::remove_reference<decltype(v)>::type::value_type V;
      std::vector<V> st;
      if (d.kind == kDeltaConsecutive) st = consecutive_encode_in_place<V>(d.order, v.data() + start_idx, page_n);
      else if (d.kind == kDeltaLookback) st = lookback_encode_in_place<V>(d.state_n_log, lbs.data(), v.data() + start_idx, page_n);
      else if (d.kind == kDeltaConv1) { if constexpr (sizeof(V) <= 4) st = test_conv1_encode_in_place<V>(d, v.data() + start_idx, page_n); else fail(kInvalidArgument, "Conv1 on a 64-bit latent"); }
      for (V x : st) out.delta_state.push_back((uint64_t)x);
      out.start = std::min(start_idx + d.n_latents_per_state(), end_idx); out.end = end_idx;
    };
    encode_var(primary, dprim, pi.v[1]);
    if (has_secondary) encode_var(secondary, dsec, pi.v[2]);
    if (de.kind == kDeltaLookback) { pi.v[0].start = delta_latents.size(); pi.v[0].end = delta_latents.size() + lbs.size(); delta_latents.insert(delta_latents.end(), lbs.begin(), lbs.end()); }
    tc.page_infos.push_back(pi);
    start_idx = end_idx;
  }
  auto contiguous = [&](auto& v, int key) {
    typename std::remove_reference<decltype(v)>::type res;
    for (auto& pi : tc.page_infos) res.insert(res.end(), v.begin() + pi.v[key].start, v.begin() + pi.v[key].end);
    return res;
  };
  tc.meta.mode = mode; tc.meta.delta = de;
  auto reshape = [&](auto& t, const auto& v, int key, auto& var) {   // between train_infos and LatentCompressor::init
    if (!((spec.tbl_vars >> key) & 1)) return;
    std::vector<std::pair<size_t, size_t>> ranges; for (auto& pi : tc.page_infos) ranges.push_back({pi.v[key].start, pi.v[key].end});
    var.forced = test_reshape_table(t, v, ranges, spec, key == kVarDelta);
  };
  if (de.kind == kDeltaLookback) {
    auto t = train_infos<uint32_t>(contiguous(delta_latents, 0), ubl);
    reshape(t, delta_latents, kVarDelta, tc.dvar);
    tc.meta.vars[kVarDelta] = var_meta_from_trained(t);
    tc.dvar.init(t, tc.meta.vars[kVarDelta], std::move(delta_latents));
  }
  {
    auto t = train_infos<P>(contiguous(primary, 1), ubl);
    reshape(t, primary, kVarPrimary, tc.pvar);
    tc.meta.vars[kVarPrimary] = var_meta_from_trained(t);
    tc.pvar.init(t, tc.meta.vars[kVarPrimary], std::move(primary));
  }
  if (has_secondary) {
    auto t = train_infos<L>(contiguous(secondary, 2), std::min(ubl, LIMITED_UNOPTIMIZED_BINS_LOG));
    reshape(t, secondary, kVarSecondary, tc.svar);
    tc.meta.vars[kVarSecondary] = var_meta_from_trained(t);
    tc.svar.init(t, tc.meta.vars[kVarSecondary], std::move(secondary));
  }
  validate_chunk_meta(tc.meta);
  if (spec.tbl_fault != kTblFaultNone) {   // one invalid table header; both decoders reject it before any walk
    if (spec.tbl_fault_var > 2 || !tc.meta.vars[spec.tbl_fault_var].present) fail(kInvalidArgument, "tbl_fault_var names a variable the chunk does not have");
    tc.fault_var = (int)spec.tbl_fault_var;
    LatentVarMeta& f = tc.fault_meta; f = tc.meta.vars[tc.fault_var];
    const size_t nb = f.bins.size();
    size_t body = 0; for (auto& pi : tc.page_infos) body += pi.v[tc.fault_var].end - pi.v[tc.fault_var].start;
    switch (spec.tbl_fault) {
      case kTblFaultWeightsBelow: { size_t j = 0; while (j < nb && f.bins[j].weight < 2) j++;
        if (j == nb) fail(kInvalidArgument, "no weight above 1 to lower"); f.bins[j].weight--; break; }
      case kTblFaultWeightsAbove: if (nb < 2) fail(kInvalidArgument, "one bin's weight cannot be raised"); f.bins[0].weight++; break;
      case kTblFaultOneBinWithAns: if (nb == 0) fail(kInvalidArgument, "no bin to keep");
        f.bins.resize(1); f.ans_size_log = std::max<Bitlen>(f.ans_size_log, 1); f.bins[0].weight = 1u << f.ans_size_log; break;
      case kTblFaultAnsTooSmall: if (nb < 2) fail(kInvalidArgument, "fewer than two bins always fit");
        f.ans_size_log = ilog2_u64(nb - 1); for (auto& b : f.bins) b.weight = 1; break;   // 2^ans_size_log < n_bins
      case kTblFaultAns15: f.ans_size_log = MAX_ANS_BITS + 1; break;
      case kTblFaultOffsetBits: if (nb == 0) fail(kInvalidArgument, "no bin to widen"); f.bins[nb / 2].offset_bits = (Bitlen)f.latent_bits + 1; break;
      case kTblFaultNoBins: if (body == 0) fail(kInvalidArgument, "no latents in the body: an empty table is valid there");
        f.bins.clear(); f.ans_size_log = 0; break;
      default: fail(kInvalidArgument, "tbl_fault");
    }
  }
}

inline DeltaEncoding test_delta_from_spec(const TestEncSpec& spec) {
  DeltaEncoding de;
  de.kind = (DeltaKind)spec.delta_kind; de.secondary_uses_delta = spec.secondary_uses_delta != 0;
  if (de.kind == kDeltaConsecutive) { de.order = spec.order; if (de.order == 0 || de.order > MAX_CONSECUTIVE_DELTA_ORDER) fail(kInvalidArgument, "consecutive order"); }
  else if (de.kind == kDeltaLookback) {
    de.window_n_log = spec.window_n_log; de.state_n_log = spec.state_n_log;
    if (de.window_n_log < 1 || de.window_n_log > MAX_DELTA_LOOKBACK_WINDOW_N_LOG || de.state_n_log > de.window_n_log) fail(kInvalidArgument, "lookback window / state");
  } else if (de.kind == kDeltaConv1) {
    if (spec.order < 1 || spec.order > 32) fail(kInvalidArgument, "conv1 order");
    de.quantization = spec.quantization; de.bias = spec.bias; de.weights.assign(spec.weights, spec.weights + spec.order); de.secondary_uses_delta = false;
  } else if (de.kind != kDeltaNone) fail(kInvalidArgument, "delta kind");
  return de;
}

// One chunk of `cn` numbers in the pages `pages`: emit(chunk) is called with the built TestChunk (its meta, write_var_metas, write_page).
template <class L, class F> void test_with_chunk(const L* src, size_t cn, uint8_t dtype, const TestEncSpec& spec, const DeltaEncoding& de,
                                                 const std::vector<size_t>& pages, F&& emit) {
  const NumKind kind = dtype_kind(dtype);
  if (spec.mode_kind == kModeTryDict) {   // mode/dict.rs:12-33: u32 indices into the dictionary of distinct latents
    std::vector<L> lat(cn);
    for (size_t i = 0; i < cn; i++) lat[i] = to_latent_ordered<L>(src[i], kind);
    std::vector<L> uniq;
    if (spec.dict_first_appearance) { std::vector<L> sorted(lat); std::sort(sorted.begin(), sorted.end()); sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
      std::vector<uint8_t> seen(sorted.size(), 0);
      for (L x : lat) { size_t k = std::lower_bound(sorted.begin(), sorted.end(), x) - sorted.begin(); if (!seen[k]) { seen[k] = 1; uniq.push_back(x); } }
    } else { uniq = lat; std::sort(uniq.begin(), uniq.end()); uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end()); }
    std::vector<std::pair<L, uint32_t>> index; for (size_t k = 0; k < uniq.size(); k++) index.push_back({uniq[k], (uint32_t)k});
    std::sort(index.begin(), index.end());
    std::vector<uint32_t> idx(cn);
    for (size_t i = 0; i < cn; i++) idx[i] = std::lower_bound(index.begin(), index.end(), std::make_pair(lat[i], (uint32_t)0))->second;
    Mode mode; mode.kind = kDict; for (L x : uniq) mode.dict.push_back((uint64_t)x);
    std::unique_ptr<TestChunk<L, uint32_t>> tc(new TestChunk<L, uint32_t>());
    test_build_chunk<L, uint32_t>(*tc, std::move(idx), {}, false, pages, mode, de, spec, dtype);
    emit(*tc);
  } else {
    ChunkConfig cfg; cfg.mode_kind = (ModeSpecKind)spec.mode_kind; cfg.mode_f64 = spec.mode_f64; cfg.mode_u64 = spec.mode_u64; cfg.enable_8_bit = true;
    if (cfg.mode_kind == kModeAuto) fail(kInvalidArgument, "the test encoder takes explicit modes");
    Mode mode;
    SplitLatents<L> lat = choose_mode_and_split<L>(src, cn, dtype, cfg, mode);
    std::unique_ptr<TestChunk<L, L>> tc(new TestChunk<L, L>());
    test_build_chunk<L, L>(*tc, std::move(lat.primary), std::move(lat.secondary), lat.has_secondary, pages, mode, de, spec, dtype);
    emit(*tc);
  }
}

// One standalone file: header | one chunk (one page) per entry of `chunks` | terminator.
template <class L> std::vector<uint8_t> test_encode_file(const L* bits, size_t n, uint8_t dtype, const TestEncSpec& spec, const std::vector<size_t>& chunks) {
  const DeltaEncoding de = test_delta_from_spec(spec);
  BitWriter w;
  write_standalone_header(w, n, 0);
  size_t sum = 0; for (size_t c : chunks) { if (c == 0) fail(kInvalidArgument, "empty chunk"); sum += c; }
  if (sum != n) fail(kInvalidArgument, "chunk sizes do not sum to n");
  size_t start = 0;
  for (size_t cn : chunks) {
    const uint32_t n_m1 = (uint32_t)cn - 1;
    w.write_aligned_bytes(&dtype, 1);
    w.write_uint(n_m1, BITS_TO_ENCODE_N_ENTRIES);
    test_with_chunk<L>(bits + start, cn, dtype, spec, de, {cn}, [&](auto& tc) {
      write_mode(tc.meta.mode, LT<L>::BITS, w); test_write_delta_encoding(tc.meta.delta, w);
      tc.write_var_metas(w);
      w.finish_byte();
      tc.write_page(0, w);
    });
    start += cn;
  }
  const uint8_t term = MAGIC_TERMINATION_BYTE;
  w.write_aligned_bytes(&term, 1);
  w.buf.resize(w.byte_len());
  return w.buf;
}

// One WRAPPED chunk in the pages `pages` (wrapped/chunk_compressor.rs:659-705): [ChunkMeta bytes, page 0, page 1, ...].
template <class L> std::vector<std::vector<uint8_t>> test_encode_wrapped(const L* bits, size_t n, uint8_t dtype, const TestEncSpec& spec, const std::vector<size_t>& pages) {
  const DeltaEncoding de = test_delta_from_spec(spec);
  size_t sum = 0; for (size_t c : pages) { if (c == 0) fail(kInvalidArgument, "empty page"); sum += c; }
  if (sum != n) fail(kInvalidArgument, "page sizes do not sum to n");
  std::vector<std::vector<uint8_t>> out;
  test_with_chunk<L>(bits, n, dtype, spec, de, pages, [&](auto& tc) {
    { BitWriter w; write_mode(tc.meta.mode, LT<L>::BITS, w); test_write_delta_encoding(tc.meta.delta, w); tc.write_var_metas(w); w.finish_byte(); w.buf.resize(w.byte_len()); out.push_back(w.buf); }
    for (size_t p = 0; p < pages.size(); p++) { BitWriter w; tc.write_page(p, w); w.buf.resize(w.byte_len()); out.push_back(w.buf); }
  });
  return out;
}

}  // namespace pco_oracle
