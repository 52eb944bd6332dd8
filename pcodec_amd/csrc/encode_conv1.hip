// encode_conv1.hip -- Conv1 delta encode (delta/conv1.rs, reference 1.0.3) on gfx950.
//
//   conv1.rs:256-286 build_initial_autocov_dots, the integer part of :288-343   -> enc_conv1_stats_kernel   (one block per chunk)
//   conv1.rs:288-421 build_autocov_mats, Cholesky, choose_config                -> enc_conv1_solve_kernel   (one wave per chunk)
//   conv1.rs:424-461 encode_in_place (per page, delta/mod.rs:121)               -> enc_conv1_resid_kernel   (one block per 2048 numbers)
//
// The split (enc_split_kernel) stages a Conv1 chunk's un-delta'd primary latents in sort buffer A, as it does for lookback.  The fit runs
// over the whole chunk (wrapped/chunk_compressor.rs:387-391); the residuals are taken page by page, each page keeping its first `order`
// latents as state.  Everything in f64 follows the reference operation by operation: the library is compiled with -ffp-contract=off, so a
// product and a sum stay two roundings, and fma appears exactly where conv1.rs writes mul_add.  Division and sqrt of doubles are correctly
// rounded on gfx950 (the compiler's f64 division and sqrt sequences), as Rust's are.
namespace pcogfx {

constexpr uint32_t kConv1Batch = 512;                 // ENCODE_BATCH_SIZE
constexpr uint32_t kConv1Group = 8;                   // batches per round of enc_conv1_stats_kernel
constexpr uint32_t kConv1Threads = 256;

// sort_utils.rs:5-56 (choose_pivot): a median of three (of medians of three from 50 numbers on)
template <class L> __device__ __forceinline__ L conv1_choose_pivot(const L PCO_GLOBAL* v, uint64_t len) {
  uint64_t a = len / 4, b = len / 2, c = (len * 3) / 4;
  if (len >= 8) {
    auto sort2 = [&](uint64_t& x, uint64_t& y) { if (v[y] < v[x]) { const uint64_t tmp = x; x = y; y = tmp; } };
    auto sort3 = [&](uint64_t& x, uint64_t& y, uint64_t& z) { sort2(x, y); sort2(y, z); sort2(x, y); };
    if (len >= 50) {
      auto sort_adjacent = [&](uint64_t& x) { uint64_t lo = x - 1, hi = x + 1; sort3(lo, x, hi); };
      sort_adjacent(a); sort_adjacent(b); sort_adjacent(c);
    }
    sort3(a, b, c);
  }
  return v[b];
}
// the centred value (conv1.rs:368-377); exact in f64 for latents of at most 32 bits
template <class L> __device__ __forceinline__ double conv1_v(L x, L center) {
  return x < center ? -(double)(uint64_t)(L)(center - x) : (double)(uint64_t)(L)(x - center);
}

// Per chunk: center, the (order + 1) autocovariance dots in the reference's order, and the exact integer sum / max |v| of v[..n - order].
// Rounds of kConv1Group batches: the block stages the round's v (plus the `order` that follow) in LDS, one thread per (batch, sep, lane of
// four) runs the 128-step strided partial sum, and thread `sep` then adds (dot0 + dot1) + (dot2 + dot3) of each batch to its accumulator
// in batch order -- the reference's sequence of roundings exactly.  Bounded by the f64 multiply-adds: (order + 1) per number.
template <class L> __device__ void conv1_stats_body(const EncWorkspace& ws, uint32_t t, uint64_t n, uint32_t order) {
  struct Lds { double v[kConv1Group * kConv1Batch + kConv1MaxOrder]; double part[kConv1Group][kConv1MaxOrder + 1][4]; int64_t isum[kConv1Threads / 64]; uint64_t vmax[kConv1Threads / 64]; };
  __shared__ Lds lds;
  const uint32_t tid = threadIdx.x;
  const L PCO_GLOBAL* lat = sort_ptr<L>(ws, t, 0);
  const L center = conv1_choose_pivot<L>(lat, n);
  const uint64_t m = n - order, almost_n = m / kConv1Batch * kConv1Batch;
  double acc = 0.0;
  int64_t isum = 0; uint64_t vmax = 0;
  // a round's numbers are loaded into registers while the round before runs its chains (the loads' latency under the f64 work)
  constexpr uint32_t kPer = (kConv1Group * kConv1Batch + kConv1MaxOrder + kConv1Threads - 1) / kConv1Threads;
  L r[kPer];
  auto round_cnt = [&](uint64_t b0, uint32_t& nb) {
    const uint64_t left = (almost_n - b0) / kConv1Batch;
    nb = left < kConv1Group ? (uint32_t)left : kConv1Group;
    return nb * kConv1Batch + order;   // b0 + cnt <= almost_n + order <= n
  };
  auto load_round = [&](uint64_t b0) {
    uint32_t nb; const uint32_t cnt = round_cnt(b0, nb);
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) { const uint32_t i = tid + k * kConv1Threads; r[k] = i < cnt ? lat[b0 + i] : (L)0; }
  };
  if (almost_n) load_round(0);
  for (uint64_t b0 = 0; b0 < almost_n; b0 += (uint64_t)kConv1Group * kConv1Batch) {
    uint32_t nb; const uint32_t cnt = round_cnt(b0, nb);
#pragma unroll
    for (uint32_t k = 0; k < kPer; k++) {
      const uint32_t i = tid + k * kConv1Threads;
      if (i < cnt) {
        const double x = conv1_v<L>(r[k], center);
        lds.v[i] = x;
        if (i < nb * kConv1Batch) { const int64_t xi = (int64_t)x; isum += xi; const uint64_t ax = (uint64_t)(xi < 0 ? -xi : xi); vmax = ax > vmax ? ax : vmax; }
      }
    }
    __syncthreads();
    const uint64_t b1 = b0 + (uint64_t)kConv1Group * kConv1Batch;
    if (b1 < almost_n) load_round(b1);
    const uint32_t n_chains = nb * (order + 1) * 4;
    for (uint32_t c = tid; c < n_chains; c += kConv1Threads) {
      const uint32_t q = c & 3u, rest = c >> 2, sep = rest % (order + 1), b = rest / (order + 1);
      const double* p = lds.v + b * kConv1Batch + q;
      double d = 0.0;
      for (uint32_t s = 0; s < kConv1Batch; s += 4) d += p[s] * p[s + sep];
      lds.part[b][sep][q] = d;
    }
    __syncthreads();
    if (tid <= order)
      for (uint32_t b = 0; b < nb; b++) acc += (lds.part[b][tid][0] + lds.part[b][tid][1]) + (lds.part[b][tid][2] + lds.part[b][tid][3]);
    __syncthreads();
  }
  for (uint64_t i = almost_n + tid; i < m; i += kConv1Threads) {
    const int64_t xi = (int64_t)conv1_v<L>(lat[i], center); isum += xi; const uint64_t ax = (uint64_t)(xi < 0 ? -xi : xi); vmax = ax > vmax ? ax : vmax;
  }
  if (tid <= order)   // the tail, one number after the other (conv1.rs:280-284)
    for (uint64_t i = almost_n; i < m; i++) acc += conv1_v<L>(lat[i], center) * conv1_v<L>(lat[i + tid], center);
  // block totals of the integer sum and the max
  for (int dl = 32; dl >= 1; dl >>= 1) {
    const int64_t o = shfl_idx(isum, (int)(lane_id() ^ dl)); isum += o;
    const uint64_t om = shfl_idx(vmax, (int)(lane_id() ^ dl)); vmax = om > vmax ? om : vmax;
  }
  if (lane_id() == 0) { lds.isum[tid >> 6] = isum; lds.vmax[tid >> 6] = vmax; }
  __syncthreads();
  EncConv PCO_GLOBAL* cv = (EncConv PCO_GLOBAL*)ws.conv + t;
  if (tid <= order) cv->dots[tid] = acc;
  if (tid == 0) {
    int64_t s = 0; uint64_t mx = 0;
    for (uint32_t w = 0; w < kConv1Threads / 64; w++) { s += lds.isum[w]; mx = lds.vmax[w] > mx ? lds.vmax[w] : mx; }
    cv->isum = s; cv->vmax = mx; cv->center = (uint64_t)center;
  }
}
__device__ __forceinline__ bool conv1_chunk_fits(const EncChunk PCO_GLOBAL* ch) {
  return uni(ch->status) == PCO_GFX_OK && uni(ch->delta_kind) == kDeltaConv1 && uni((uint64_t)ch->n) >= (uint64_t)uni(ch->delta_order) + 1;
}
// grid = tasks, kConv1Threads threads
__global__ __launch_bounds__(kConv1Threads) void enc_conv1_stats_kernel(EncWorkspace ws, uint32_t n_tasks) {
  const uint32_t t = blockIdx.x;
  if (t >= n_tasks) return;
  const EncChunk PCO_GLOBAL* ch = (const EncChunk PCO_GLOBAL*)ws.chunks + t;
  if (!conv1_chunk_fits(ch)) return;
  const uint64_t n = uni((uint64_t)ch->n); const uint32_t order = uni(ch->delta_order);
  const int bits = dtype_bits(uni(ch->dtype));
  if (bits == 32) conv1_stats_body<uint32_t>(ws, t, n, order);
  else if (bits == 16) conv1_stats_body<uint16_t>(ws, t, n, order);
  else if (bits == 8) conv1_stats_body<uint8_t>(ws, t, n, order);
}

// floor(log2(x)) as Rust's `x.log2().floor()` gives it, for a finite x >= 1.  log2 of a double is taken to be rounded to nearest: it is the
// exponent e of x, except in the band just below 2^(e+1) where log2(x) = e + 1 - delta / ln 2 (delta = 1 - x / 2^(e+1)) lies within half an
// ulp of the integer e + 1 and rounds up to it.  The band is a few ulps of x wide; tests/test_conv1_model.py checks the rule against the
// host's math.log2 around every power of two the quantization can meet.
__host__ __device__ inline int conv1_floor_log2(double x) {
  int e = 0;
  const double m = frexp(x, &e);                       // x = m * 2^e, m in [0.5, 1): floor(log2 x) = e - 1 away from the band
  const double delta = 1.0 - m;                        // exact (Sterbenz)
  const int k = e;                                     // the integer log2(x) may round up to
  if (k <= 0) return e - 1;
  const int kexp = 31 - __builtin_clz((uint32_t)k);    // ulp(k) = 2^(kexp - 52); just below a power of two k the spacing is half that
  const double half_ulp = ldexp(1.0, (k & (k - 1)) == 0 ? kexp - 54 : kexp - 53);
  return delta * 1.4426950408889634 <= half_ulp ? k : e - 1;   // (delta / ln 2 against half an ulp of k)
}
// Rust `f64 as i64`: truncation, saturating, NaN -> 0
__host__ __device__ inline int64_t conv1_as_i64(double x) {
  if (x != x) return 0;
  if (x >= 9223372036854775807.0) return INT64_MAX;
  if (x <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)x;
}

// One wave per chunk, lane 0 solving: build_autocov_mats (conv1.rs:288-343), into_cholesky (:59-96), forward_sub_into (:122-144),
// transposed_backward_sub_into (:98-120), choose_config (:358-421).  O(order^3) flops on a 33 x 33 matrix in LDS; the one part that can be
// long is initial_sum when the integer shortcut does not hold (n * max|v| >= 2^53: the f64 partial sums may round, so they are formed one
// number after the other, 64 at a time through LDS).  A chunk whose fit returns no config becomes a NoOp-delta chunk here; a chunk with a
// page shorter than its order (the reference panics in encode_in_place) fails with INVALID_ARGUMENT.
template <class L> __device__ void conv1_solve_body(const EncWorkspace& ws, uint32_t t, EncChunk PCO_GLOBAL* ch, double* xtx, double* xty, double* seq) {
  const uint32_t lane = lane_id();
  EncConv PCO_GLOBAL* cv = (EncConv PCO_GLOBAL*)ws.conv + t;
  const L PCO_GLOBAL* lat = sort_ptr<L>(ws, t, 0);
  const uint64_t n = uni((uint64_t)ch->n);
  const uint32_t order = uni(ch->delta_order), h = order + 1;
  const L center = (L)uni((uint64_t)cv->center);
  const uint64_t m = n - order;
  // initial_sum = v[..n - order].iter().sum()
  double initial_sum;
  const uint64_t vmax = uni((uint64_t)cv->vmax);
  if (vmax == 0 || m <= ((1ull << 53) - 1) / vmax) initial_sum = (double)(int64_t)uni((uint64_t)cv->isum);   // every partial sum is an integer below 2^53: exact in any order
  else {
    double s = 0.0;
    for (uint64_t i0 = 0; i0 < m; i0 += 64) {
      const uint64_t i = i0 + lane;
      seq[lane] = i < m ? conv1_v<L>(lat[i], center) : 0.0;
      enc_wave_sync();
      if (lane == 0) { const uint32_t c = m - i0 < 64 ? (uint32_t)(m - i0) : 64u; for (uint32_t k = 0; k < c; k++) s += seq[k]; }
      enc_wave_sync();
    }
    initial_sum = s;
  }
  if (lane != 0) return;
  auto V = [&](uint64_t i) { return conv1_v<L>(lat[i], center); };
  auto X = [&](uint32_t i, uint32_t j) -> double& { return xtx[i + j * h]; };   // column-major (conv1.rs:38-41)
  for (uint32_t i = 0; i < h * h; i++) xtx[i] = 0.0;
  for (uint32_t i = 0; i < h; i++) xty[i] = 0.0;
  for (uint32_t i = 0; i < order; i++) { const double d = cv->dots[i]; X(i, 0) = d; X(0, i) = d; }
  X(order, 0) = initial_sum; X(0, order) = initial_sum;
  xty[0] = cv->dots[order];
  for (uint32_t i = 1; i < order; i++) {
    for (uint32_t j = 1; j <= i; j++) {
      const double last = X(i - 1, j - 1);
      const double dot = last + (V(n - order + i - 1) * V(n - order + j - 1) - V(i - 1) * V(j - 1));
      X(i, j) = dot; X(j, i) = dot;
    }
    const double last_sum = X(order, i - 1);
    const double sum = last_sum + (V(n - order + i - 1) - V(i - 1));
    X(order, i) = sum; X(i, order) = sum;
  }
  for (uint32_t i = 1; i < order; i++) {
    const double last = X(order - 1, i - 1);
    xty[i] = last + (V(n - order + i - 1) * V(n - 1) - V(i - 1) * V(order - 1));
  }
  X(order, order) = (double)m;
  xty[order] = X(order, order - 1) + (V(n - 1) - V(order - 1));
  for (uint32_t i = 0; i < h; i++) X(i, i) = X(i, i) + 0.1;   // L2_REGULARIZATION
  // Cholesky-Crout
  for (uint32_t j = 0; j < h; j++) {
    for (uint32_t i = 0; i < j; i++) X(i, j) = 0.0;
    double s = 0.0;
    for (uint32_t k = 0; k < j; k++) { const double val = X(j, k); s = fma(val, val, s); }
    const double diag = sqrt(fmax(X(j, j) - s, 0.0));
    X(j, j) = diag;
    const double scale = diag == 0.0 ? 0.0 : 1.0 / diag;
    for (uint32_t i = j + 1; i < h; i++) {
      double s2 = 0.0;
      for (uint32_t k = 0; k < j; k++) s2 = fma(X(i, k), X(j, k), s2);
      X(i, j) = scale * (X(i, j) - s2);
    }
  }
  for (uint32_t j = 0; j < h; j++) {   // forward substitution
    const double dv = xty[j] / X(j, j);
    xty[j] = dv;
    for (uint32_t i = j + 1; i < h; i++) xty[i] = xty[i] - dv * X(i, j);
  }
  for (uint32_t j = h; j-- > 0;) {     // backward substitution with the transpose
    const double dv = xty[j] / X(j, j);
    xty[j] = dv;
    for (uint32_t i = 0; i < j; i++) xty[i] = xty[i] - dv * X(j, i);
  }
  double total = 0.0, total_abs = 0.0;
  for (uint32_t k = 0; k < order; k++) { total_abs += fabs(xty[k]); total += xty[k]; }
  bool ok = isfinite(total) && isfinite(total_abs);
  int q = -1;
  double float_bias = 0.0;
  if (ok) {
    float_bias = ((1.0 - total) * (double)(uint64_t)center) + xty[order];
    constexpr double kConvMax = sizeof(L) == 1 ? 32767.0 : (sizeof(L) == 2 ? 2147483647.0 : 9223372036854775807.0);
    constexpr int kConvBits = sizeof(L) == 1 ? 16 : (sizeof(L) == 2 ? 32 : 64);
    const double x = kConvMax / (total_abs * (double)(L)~(L)0 + fabs(float_bias) + 1.0);
    if (x >= 1.0) {   // (below 1 -- or NaN -- the quantization is negative: no config)
      q = conv1_floor_log2(x) - 1;
      q = q < 31 ? q : 31;
      q = q < kConvBits - 1 ? q : kConvBits - 1;
    }
    ok = q >= 0;
  }
  if (ok) {
    const double f = ldexp(1.0, q);
    for (uint32_t k = 0; k < order; k++) cv->w[k] = conv1_as_i64(round(xty[k] * f));
    cv->bias = conv1_as_i64(float_bias * f);
    cv->quant = (uint32_t)q; cv->order = order;
    // pages shorter than the order: the reference panics (conv1.rs:428 slices latents[..order]); refused here
    const uint32_t np = ch->n_pages;
    for (uint32_t p = 0; p < np; p++) {
      const uint64_t pn = ch->exact_paging ? ws.pages[ch->page_first + p].n : (uint64_t)(ch->page_low + (p < ch->page_r ? 1u : 0u));
      if (pn < order) { ch->status = PCO_GFX_INVALID_ARGUMENT; break; }
    }
  }
  if (!ok) {   // NoOp delta (wrapped/chunk_compressor.rs:387-391): every latent stored
    ch->delta_kind = kDeltaNone; ch->delta_order = 0;
    ch->v[1].lat_start = 0; ch->v[1].n_lat = (uint32_t)n;
    cv->order = 0;
  }
}
// grid = tasks, 64 threads
__global__ __launch_bounds__(64) void enc_conv1_solve_kernel(EncWorkspace ws, uint32_t n_tasks) {
  __shared__ double xtx[(kConv1MaxOrder + 1) * (kConv1MaxOrder + 1)], xty[kConv1MaxOrder + 1], seq[64];
  const uint32_t t = blockIdx.x;
  if (t >= n_tasks) return;
  EncChunk PCO_GLOBAL* ch = (EncChunk PCO_GLOBAL*)ws.chunks + t;
  EncConv PCO_GLOBAL* cv = (EncConv PCO_GLOBAL*)ws.conv + t;
  const bool planned = uni(ch->status) == PCO_GFX_OK && uni(ch->delta_kind) == kDeltaConv1;
  if (threadIdx.x == 0) cv->planned = planned ? 1u : 0u;
  if (!planned) return;
  if (!conv1_chunk_fits(ch)) {   // n < order + 1: no config (conv1.rs:359-361)
    if (threadIdx.x == 0) { const uint64_t n = ch->n; ch->delta_kind = kDeltaNone; ch->delta_order = 0; ch->v[1].lat_start = 0; ch->v[1].n_lat = (uint32_t)n; cv->order = 0; }
    return;
  }
  const int bits = dtype_bits(uni(ch->dtype));
  if (bits == 32) conv1_solve_body<uint32_t>(ws, t, ch, xtx, xty, seq);
  else if (bits == 16) conv1_solve_body<uint16_t>(ws, t, ch, xtx, xty, seq);
  else if (bits == 8) conv1_solve_body<uint8_t>(ws, t, ch, xtx, xty, seq);
}

// The residuals of one tile of a page (conv1.rs:424-461, predict_one :148-161): latent - predict(previous `order` latents) + MID, in the
// Conv type (i16 for u8, i32 for u16, i64 for u32); the page's first `order` latents are its state.  A chunk whose fit gave no config
// copies its primary through.  The tile and the `order` numbers before it are staged in LDS; the primary's range is reduced per block.
template <class L> struct ConvOf { typedef int64_t T; };
template <> struct ConvOf<uint8_t> { typedef int16_t T; };
template <> struct ConvOf<uint16_t> { typedef int32_t T; };
template <class L> __device__ void conv1_resid_body(const EncWorkspace& ws, uint32_t t, EncPage PCO_GLOBAL* pg, uint32_t page, uint32_t tile) {
  typedef typename ConvOf<L>::T C;
  __shared__ L win[kConv1MaxOrder + kSplitTile];
  __shared__ C wts[kConv1MaxOrder];
  __shared__ uint64_t red[2][kConv1Threads / 64];
  EncChunk PCO_GLOBAL* ch = (EncChunk PCO_GLOBAL*)ws.chunks + t;
  const EncConv PCO_GLOBAL* cv = (const EncConv PCO_GLOBAL*)ws.conv + t;
  const uint32_t tid = threadIdx.x;
  const uint64_t n = uni((uint64_t)pg->n), pstart = uni((uint64_t)pg->start);
  const uint32_t order = uni(cv->order), quant = uni(cv->quant);   // order 0: NoOp
  const C bias = (C)uni((uint64_t)cv->bias);
  const L PCO_GLOBAL* src = sort_ptr<L>(ws, t, 0) + pstart;
  L PCO_GLOBAL* dst = lat_ptr<L>(ws, t, 1) + pstart;
  const uint64_t tile0 = (uint64_t)tile * kSplitTile;
  const uint64_t lo = tile0 >= order ? tile0 - order : 0, hi = tile0 + kSplitTile < n ? tile0 + kSplitTile : n;
  for (uint64_t i = lo + tid; i < hi; i += kConv1Threads) win[i - tile0 + kConv1MaxOrder] = src[i];
  if (tid < order) wts[tid] = (C)cv->w[tid];
  __syncthreads();
  L mn = (L)~(L)0, mx = 0;
  for (uint64_t i = tile0 + tid; i < hi; i += kConv1Threads) {
    const L x = win[i - tile0 + kConv1MaxOrder];
    if (i < order) { ws.conv_state[(uint64_t)page * kConv1MaxOrder + i] = (uint32_t)x; continue; }
    L r = x;
    if (order) {
      // (the Conv type's wrapping arithmetic, formed in 32 bits for i16 / i32 and in 64 for i64, then cut to the type: the quantization keeps
      //  the sum in range, conv1.rs:388-400)
      typedef typename std::conditional<sizeof(C) == 8, uint64_t, uint32_t>::type A;
      A s = (A)(int64_t)bias;
      const L* w0 = win + (i - tile0 + kConv1MaxOrder - order);
      for (uint32_t k = 0; k < order; k++) s += (A)(int64_t)wts[k] * (A)w0[k];
      const C sc = (C)s;
      r = (L)(x - (L)((sc < 0 ? (C)0 : sc) >> quant) + lmid<L>());
    }
    dst[i] = r;
    mn = r < mn ? r : mn; mx = r > mx ? r : mx;
  }
  uint64_t m1 = mn, x1 = mx;
  for (int dl = 32; dl >= 1; dl >>= 1) {
    const uint64_t o1 = shfl_idx(m1, (int)(lane_id() ^ dl)); m1 = o1 < m1 ? o1 : m1;
    const uint64_t o2 = shfl_idx(x1, (int)(lane_id() ^ dl)); x1 = o2 > x1 ? o2 : x1;
  }
  if (lane_id() == 0) { red[0][tid >> 6] = m1; red[1][tid >> 6] = x1; }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < kConv1Threads / 64; w++) { m1 = red[0][w] < m1 ? red[0][w] : m1; x1 = red[1][w] > x1 ? red[1][w] : x1; }
    if (red[0][0] < m1) m1 = red[0][0];
    if (red[1][0] > x1) x1 = red[1][0];
    if (m1 <= x1) { atomicMin((unsigned long long*)&ch->v[1].minv, (unsigned long long)m1); atomicMax((unsigned long long*)&ch->v[1].maxv, (unsigned long long)x1); }
  }
}
// grid = pages * tiles_per_page, kConv1Threads threads
__global__ __launch_bounds__(kConv1Threads) void enc_conv1_resid_kernel(EncWorkspace ws, uint32_t tiles_per_page) {
  const uint32_t page = blockIdx.x / tiles_per_page, tile = blockIdx.x % tiles_per_page;
  EncPage PCO_GLOBAL* pg = (EncPage PCO_GLOBAL*)ws.pages + page;
  if (uni(pg->flags) & kPageFlagMetaOnly) return;
  const uint32_t t = uni(pg->chunk);
  if (uni(ws.chunks[t].status) != PCO_GFX_OK || uni(ws.conv[t].planned) == 0) return;
  if ((uint64_t)tile * kSplitTile >= uni((uint64_t)pg->n)) return;
  const int bits = dtype_bits(uni(ws.chunks[t].dtype));
  if (bits == 32) conv1_resid_body<uint32_t>(ws, t, pg, page, tile);
  else if (bits == 16) conv1_resid_body<uint16_t>(ws, t, pg, page, tile);
  else if (bits == 8) conv1_resid_body<uint8_t>(ws, t, pg, page, tile);
}

}  // namespace pcogfx
