// Pixel-wise losses (K10), FGSM tail (K11), flat Adam (K12) and Dice counts.  All HBM-bound:
// one pass over [pixels][C] fp32 logits with C <= 8 channels held in registers; reductions are
// wave shuffle -> LDS -> per-block partial -> single-block fixed-order finalize (deterministic,
// no atomics on floats, no host synchronisation).
#include "dct_common.h"

namespace {

constexpr int kMaxBlocks = 1024;
constexpr float kEntEps = 1e-16f;  // loss.py:80

template <int C> __device__ __forceinline__ void load_px(const float* p, long long pix, float v[C]) {
  if constexpr (C == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + pix * 4);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if constexpr (C == 2) {
    const f32x2 t = *reinterpret_cast<const f32x2*>(p + pix * 2);
    v[0] = t[0]; v[1] = t[1];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[pix * C + c];
  }
}
template <int C> __device__ __forceinline__ void store_px_plain(float* p, long long pix, const float v[C]) {
  if constexpr (C == 4) *reinterpret_cast<f32x4*>(p + pix * 4) = f32x4{v[0], v[1], v[2], v[3]};
  else if constexpr (C == 2) *reinterpret_cast<f32x2*>(p + pix * 2) = f32x2{v[0], v[1]};
  else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[pix * C + c] = v[c];
  }
}
// (not written as a call of itself with acc = false: a recursive function is not inlined, and every caller then passed its pixel through scratch
// memory to a real call -- round 5, seen in the ISA of every kernel of this file that stores through it)
template <int C> __device__ __forceinline__ void store_px(float* p, long long pix, const float v[C], bool acc) {
  if (acc) {
#pragma clang fp contract(off)    // the value is rounded before it is added, whatever expression the caller formed it from (as when this was a call)
    float o[C];
    load_px<C>(p, pix, o);
    float t[C];
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = v[c] + o[c];
    store_px_plain<C>(p, pix, t);
    return;
  }
  store_px_plain<C>(p, pix, v);
}
template <int C> __device__ __forceinline__ float softmax_px(const float x[C], float p[C]) {
  float m = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { p[c] = expf(x[c] - m); s += p[c]; }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] *= inv;
  return m + logf(s);  // logsumexp
}

__device__ __forceinline__ void block_partial2(float a, float b, float* partial) {
  __shared__ float sm[8];
  a = wave_sum(a); b = wave_sum(b);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sm[w] = a; sm[4 + w] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 2 + 0] = sm[0] + sm[1] + sm[2] + sm[3];
    partial[blockIdx.x * 2 + 1] = sm[4] + sm[5] + sm[6] + sm[7];
  }
}
// The fold of the block partial pairs, by a whole block of 256 threads and in one fixed order: thread i takes pairs i, i + 256, ... in
// order, then the LDS tree.  Every thread gets both sums.  The one copy: whichever kernel folds, the sums come out bit for bit.
__device__ __forceinline__ void fold_partials(const float* partial, int blocks, float& sum_a, float& sum_b) {
  __shared__ float sa[256], sb[256];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < blocks; i += 256) { a += partial[2 * i]; b += partial[2 * i + 1]; }
  sa[threadIdx.x] = a; sb[threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
    __syncthreads();
  }
  sum_a = sa[0]; sum_b = sb[0];
}
// out[0] = sum_a / (use_count ? sum_b : denom); out[1] = sum_b
__global__ __launch_bounds__(256) void finalize_kernel(const float* partial, int blocks, float* out, int use_count, float denom, int write_b) {
  float a, b;
  fold_partials(partial, blocks, a, b);
  if (threadIdx.x == 0) {
    out[0] = a / (use_count ? b : denom);
    if (write_b) out[1] = b;
  }
}

// ---- plain, class-weighted and focal cross entropy: one kernel family over the rule of one pixel (the rules: include/dct.h) ------------
// The C class weights are read once per wave (a uniform address: they sit in scalar registers) and w_t is picked by the select that picks
// x_t -- never weight[t].
template <int C> __device__ __forceinline__ void load_weights(const float* weight, float wr[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) wr[c] = weight ? weight[c] : 1.f;
}
template <int C> __device__ __forceinline__ bool counted(long long t, int ignore) { return t != ignore && t >= 0 && t < C; }
template <int C> __device__ __forceinline__ float weight_of(long long t, const float wr[C]) {
  float w = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) w = (t == c) ? wr[c] : w;
  return w;
}
// l = logsumexp(x) - x_t of one pixel (x_t = 0 for a target outside [0, C))
template <int C> __device__ __forceinline__ float ce_px(const float* logits, long long pix, long long t) {
  float x[C], p[C];
  load_px<C>(logits, pix, x);
  const float lse = softmax_px<C>(x, p);
  float xt = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) xt = (t == c) ? x[c] : xt;
  return lse - xt;
}
// One focal pixel: p = softmax(x); q = the mass off the target, summed from the exponentials (never 1 - p_t: at a confident pixel that is a
// rounding error); l = -log p_t = -log1p(-q) while q < 1/2 (relative error ~ that of q) and (max - x_t) + log(sum) above it (two terms
// >= 0, l >= log 2: nothing cancels); m = q^gamma = exp2(gamma log2 q); k = m (1 + gamma p_t l / q), the sum of two terms >= 0.
// gamma == 0 (the same in every lane) is m = k = 1 whatever q is; q == 0 under gamma > 0 is m = k = 0 (then l = -log1p(-0) = 0 too).
// The selects keep every operand finite: log2 and the division see 1 in place of a zero q, and p_t == 0 (the only case in which l may
// have overflowed) drops its term.  A target outside [0, C) selects nothing and leaves finite numbers that the callers discard.
template <int C>
__device__ __forceinline__ void focal_px(const float x[C], long long t, float gamma, float p[C], float& q, float& l, float& m, float& k) {
  float mx = x[0];
#pragma unroll
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
  float s = 0.f, off = 0.f, xt = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = expf(x[c] - mx);
    s += p[c];
    off += (t == c) ? 0.f : p[c];
    xt = (t == c) ? x[c] : xt;
  }
  const float inv = 1.f / s;
  float pt = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { p[c] *= inv; pt = (t == c) ? p[c] : pt; }
  q = off * inv;
  l = q < 0.5f ? -log1pf(-q) : (mx - xt) + logf(s);
  if (gamma == 0.f) { m = 1.f; k = 1.f; return; }
  const bool some = q > 0.f;
  const float qs = some ? q : 1.f;
  const float pw = exp2f(gamma * log2f(qs));
  const float tl = pt > 0.f ? pt * (l / qs) : 0.f;
  m = some ? pw : 0.f;
  k = some ? pw * (1.f + gamma * tl) : 0.f;
}

// A rule is what the three criteria differ in.  It is built from (ignore, weight, gamma), once per thread, and offers
//   counted(t)                      whether the pixel enters the sums (and the map);
//   value(logits, pix, t, den)      the value of one counted pixel, with its term of the denominator in den;
//   grad(logits, pix, t, g, d)      the gradient row of one pixel (counted or not) under the scalar factor g;
//   kChecksC                        whether the host refuses an unsupported C ahead of the workspace (else: at dispatch).
// Plain: every t != ignore counts, also one outside [0, C) (its x_t is 0, its gradient g p); value l, denominator 1.
template <int C> struct PlainRule {
  static constexpr bool kChecksC = false;
  int ignore;
  __device__ __forceinline__ PlainRule(int ignore_, const float*, float) : ignore(ignore_) {}
  __device__ __forceinline__ bool counted(long long t) const { return t != ignore; }
  __device__ __forceinline__ float value(const float* logits, long long pix, long long t, float& den) const {
    den = 1.f;
    return ce_px<C>(logits, pix, t);
  }
  __device__ __forceinline__ void grad(const float* logits, long long pix, long long t, float g, float d[C]) const {
    float x[C], p[C];
    load_px<C>(logits, pix, x);
    softmax_px<C>(x, p);
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = (t == ignore) ? 0.f : g * (p[c] - (t == c ? 1.f : 0.f));
  }
};
// Weighted: a target outside [0, C) is ignored like ignore_index (w = 0, no logit read for the value, gradient exactly 0); value w_t l,
// denominator w_t, gradient (g w_t) (p - onehot).
template <int C> struct WeightedRule {
  static constexpr bool kChecksC = true;
  int ignore;
  float wr[C];
  __device__ __forceinline__ WeightedRule(int ignore_, const float* weight, float) : ignore(ignore_) { load_weights<C>(weight, wr); }
  __device__ __forceinline__ bool counted(long long t) const { return ::counted<C>(t, ignore); }
  __device__ __forceinline__ float value(const float* logits, long long pix, long long t, float& den) const {
    const float l = ce_px<C>(logits, pix, t);
    den = weight_of<C>(t, wr);
    return den * l;
  }
  __device__ __forceinline__ void grad(const float* logits, long long pix, long long t, float g, float d[C]) const {
    const bool on = counted(t);
    float x[C], p[C];
    load_px<C>(logits, pix, x);
    softmax_px<C>(x, p);
    const float gw = g * weight_of<C>(t, wr);
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = on ? gw * (p[c] - (t == c ? 1.f : 0.f)) : 0.f;
  }
};
// Focal: the weighted rule's pixels; value w_t m l, denominator w_t, gradient (g w_t k) (p - onehot) with the target's own entry as -q.
template <int C> struct FocalRule {
  static constexpr bool kChecksC = true;
  int ignore;
  float gamma, wr[C];
  __device__ __forceinline__ FocalRule(int ignore_, const float* weight, float gamma_) : ignore(ignore_), gamma(gamma_) { load_weights<C>(weight, wr); }
  __device__ __forceinline__ bool counted(long long t) const { return ::counted<C>(t, ignore); }
  __device__ __forceinline__ float value(const float* logits, long long pix, long long t, float& den) const {
    float x[C], p[C], q, l, m, k;
    load_px<C>(logits, pix, x);
    focal_px<C>(x, t, gamma, p, q, l, m, k);
    den = weight_of<C>(t, wr);
    return den * (m * l);
  }
  __device__ __forceinline__ void grad(const float* logits, long long pix, long long t, float g, float d[C]) const {
    const bool on = counted(t);
    float x[C], p[C], q, l, m, k;
    load_px<C>(logits, pix, x);
    focal_px<C>(x, t, gamma, p, q, l, m, k);
    const float gw = g * weight_of<C>(t, wr) * k;
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = on ? gw * (t == c ? -q : p[c]) : 0.f;
  }
};

// dl (=|+=) the rule's gradient rows over the grid's pixels; g_px (nullable): a per-pixel factor times g (the map's dmap)
template <int C, template <int> class Rule>
__device__ __forceinline__ void grad_pixels(const Rule<C>& rule, const float* logits, const long long* tgt, long long P, float g, const float* g_px,
                                            float* dl, int acc) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float d[C];
    rule.grad(logits, pix, tgt[pix], g_px ? g * g_px[pix] : g, d);
    store_px<C>(dl, pix, d, acc);
  }
}
// partial[2b] = the block's sum of the values, partial[2b + 1] = its sum of the denominator terms
template <int C, template <int> class Rule>
__global__ __launch_bounds__(256) void loss_fwd_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                        float gamma, float* partial) {
  const Rule<C> rule(ignore, weight, gamma);
  float sum = 0.f, den = 0.f;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const long long t = tgt[pix];
    if (!rule.counted(t)) continue;
    float w;
    sum += rule.value(logits, pix, t, w);
    den += w;
  }
  block_partial2(sum, den, partial);
}
// the logit gradient from a finished denominator (denom nullable: the sum reduction passes none, its denominator is 1)
template <int C, template <int> class Rule>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                        float gamma, const float* denom, const float* gscale, float gmul, float* dl, int acc) {
  const Rule<C> rule(ignore, weight, gamma);
  float g = (gscale ? gscale[0] : 1.f) * gmul;
  if (denom) g = g / denom[0];
  grad_pixels<C, Rule>(rule, logits, tgt, P, g, nullptr, dl, acc);
}
// A step's forward and backward in two launches instead of three (every small launch on a model's chain costs the step ~3 us): this
// kernel folds the forward kernel's block partials itself -- every block, through finalize_kernel's fold_partials, so the denominator
// (and the loss block 0 writes) come out bit for bit -- before it writes the logit gradients.
template <int C, template <int> class Rule>
__global__ __launch_bounds__(256) void loss_bwd_fin_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                            float gamma, int mean, const float* partial, int blocks, float* out2,
                                                            const float* gscale, float gmul, float* dl, int acc) {
  float sum, den;
  fold_partials(partial, blocks, sum, den);
  if (blockIdx.x == 0 && threadIdx.x == 0) { out2[0] = mean ? sum / den : sum; out2[1] = den; }
  const Rule<C> rule(ignore, weight, gamma);
  float g = (gscale ? gscale[0] : 1.f) * gmul;
  if (mean) g = g / den;
  grad_pixels<C, Rule>(rule, logits, tgt, P, g, nullptr, dl, acc);
}
// the per-pixel map: the value of a counted pixel, 0 elsewhere
template <int C, template <int> class Rule>
__global__ __launch_bounds__(256) void loss_map_fwd_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                            float gamma, float* map) {
  const Rule<C> rule(ignore, weight, gamma);
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const long long t = tgt[pix];
    float v = 0.f;
    if (rule.counted(t)) {
      float w;
      v = rule.value(logits, pix, t, w);
    }
    map[pix] = v;
  }
}
template <int C, template <int> class Rule>
__global__ __launch_bounds__(256) void loss_map_bwd_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                            float gamma, const float* dmap, float gmul, float* dl, int acc) {
  const Rule<C> rule(ignore, weight, gamma);
  grad_pixels<C, Rule>(rule, logits, tgt, P, gmul, dmap, dl, acc);
}

// ---- top-k cross entropy: the mean of the K largest entries of the weighted rule's map (the rule: include/dct.h, dct_topk_ce_*) ---------
// tau, the K-th largest entry, is found by a radix select over the map's order-preserving 32-bit keys, most significant digit first:
// three histograms (11 + 11 + 10 bits; LDS integer atomics per block, then one global integer add per non-empty bin), and every block
// of the next launch picks the digit from the finished histogram for itself (the way the fused backward kernels fold the forward
// partials in every block: no ticket, no last block).  Only integers are added atomically, so nothing depends on arrival order.
// Workspace, in 32-bit words: the three histograms (zeroed by the entry point), the select's state, then kMaxBlocks partial pairs.
constexpr int kTopkBins1 = 2048, kTopkBins2 = 2048, kTopkBins3 = 1024;
constexpr int kTopkHistWords = kTopkBins1 + kTopkBins2 + kTopkBins3;
constexpr int kTopkSelWords = 16;        // {N, K, digit 1, entries above it, digit 2, entries above digits 1:2}, written by block 0
constexpr size_t kTopkWsBytes = (size_t)(kTopkHistWords + kTopkSelWords + kMaxBlocks * 2) * 4;

// The key: unsigned order of the keys = float order of the values, -0 on +0's key, every NaN on the largest key (above +inf).
__device__ __forceinline__ unsigned topk_key(float v) {
  unsigned b = __float_as_uint(v);
  if (b == 0x80000000u) b = 0u;
  const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return v != v ? 0xffffffffu : k;
}
__device__ __forceinline__ float topk_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
// K = min(N, max(1, floor(N k / 100))) in IEEE double, in this order
__device__ __forceinline__ unsigned topk_k(unsigned N, double k_percent) {
  long long k = (long long)floor((double)N * k_percent / 100.0);
  k = k < 1 ? 1 : k;
  return (unsigned)(k > (long long)N ? (long long)N : k);
}
__device__ __forceinline__ float topk_value(float sum, long long K, long long n_gt, float tau) {
#pragma clang fp contract(off)    // one rounding per operation in both kernels that form it
  const float rest = (float)(K - n_gt) * tau;
  return (sum + rest) / (float)K;
}
// Thread i holds bins [i PER, (i + 1) PER) of a histogram of NB = 256 PER bins in h; above = the entries in the bins above its own
// (a suffix sum: shuffles inside the wave, then the four wave totals), total = all entries.  Every thread of the block calls it.
template <int NB>
__device__ __forceinline__ void hist_suffix(const unsigned* hist, unsigned h[NB / 256], unsigned& above, unsigned& total) {
  constexpr int PER = NB / 256;
  __shared__ unsigned wsum[4];
  unsigned mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) { h[j] = hist[threadIdx.x * PER + j]; mine += h[j]; }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_down(incl, off, 64);
    incl += (lane + off < 64) ? o : 0u;
  }
  if (lane == 0) wsum[w] = incl;
  __syncthreads();
  above = incl - mine;
#pragma unroll
  for (int k = 1; k < 4; ++k) above += (k > w) ? wsum[k] : 0u;
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// The bin that holds the rank-th largest entry (1 <= rank <= total), in every thread: bin, gt = the entries in the bins above it,
// cnt = its own.  Exactly one thread's bins straddle the rank; a rank of 0 (nothing counted) leaves {0, 0, 0}.
template <int NB>
__device__ __forceinline__ void pick_bin(const unsigned h[NB / 256], unsigned above, unsigned rank, unsigned& bin, unsigned& gt, unsigned& cnt) {
  constexpr int PER = NB / 256;
  __shared__ unsigned res[3];
  if (threadIdx.x == 0) { res[0] = 0u; res[1] = 0u; res[2] = 0u; }
  __syncthreads();
  unsigned a = above;
#pragma unroll
  for (int j = PER - 1; j >= 0; --j) {
    if (a < rank && rank <= a + h[j]) { res[0] = threadIdx.x * PER + j; res[1] = a; res[2] = h[j]; }
    a += h[j];
  }
  __syncthreads();
  bin = res[0]; gt = res[1]; cnt = res[2];
}
__device__ __forceinline__ void lds_hist_clear(unsigned* lh, int bins) {
  for (int i = threadIdx.x; i < bins; i += 256) lh[i] = 0u;
  __syncthreads();
}
__device__ __forceinline__ void lds_hist_flush(const unsigned* lh, int bins, unsigned* hist) {
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 256) {
    const unsigned c = lh[i];
    if (c) atomicAdd(hist + i, c);
  }
}
// Launch 1: loss_map_fwd_kernel<C, WeightedRule> (the same expressions: the map comes out bit for bit) + the histogram of the top 11
// key bits of the counted pixels.  Its total is N.
template <int C>
__global__ __launch_bounds__(256) void topk_map_hist_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                             float* map, unsigned* h1) {
  __shared__ unsigned lh[kTopkBins1];
  lds_hist_clear(lh, kTopkBins1);
  const WeightedRule<C> rule(ignore, weight, 0.f);
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const long long t = tgt[pix];
    float v = 0.f;
    if (rule.counted(t)) {
      float w;
      v = rule.value(logits, pix, t, w);
      atomicAdd(&lh[topk_key(v) >> 21], 1u);
    }
    map[pix] = v;
  }
  lds_hist_flush(lh, kTopkBins1, h1);
}
// Launch 2: N and K from the first histogram, the first digit, then the histogram of the next 11 bits of the counted pixels under it.
// The stored map is read (here and from here on), never a recomputed value; the target only where the key matches.
__global__ __launch_bounds__(256) void topk_hist2_kernel(const float* map, const long long* tgt, long long P, int ignore, int C, double k_percent,
                                                          const unsigned* h1, unsigned* h2, unsigned* sel) {
  __shared__ unsigned lh[kTopkBins2];
  lds_hist_clear(lh, kTopkBins2);
  unsigned h[kTopkBins1 / 256], above, N, b1, gt1, cnt;
  hist_suffix<kTopkBins1>(h1, h, above, N);
  const unsigned K = N ? topk_k(N, k_percent) : 0u;
  pick_bin<kTopkBins1>(h, above, K, b1, gt1, cnt);
  if (blockIdx.x == 0 && threadIdx.x == 0) { sel[0] = N; sel[1] = K; sel[2] = b1; sel[3] = gt1; }
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const unsigned key = topk_key(map[pix]);
    if ((key >> 21) != b1) continue;
    const long long t = tgt[pix];
    if (t != ignore && t >= 0 && t < C) atomicAdd(&lh[(key >> 10) & (kTopkBins2 - 1)], 1u);
  }
  lds_hist_flush(lh, kTopkBins2, h2);
}
// Launch 3: the second digit, then the histogram of the last 10 bits under the 22-bit prefix.
__global__ __launch_bounds__(256) void topk_hist3_kernel(const float* map, const long long* tgt, long long P, int ignore, int C,
                                                          const unsigned* h2, unsigned* h3, unsigned* sel) {
  __shared__ unsigned lh[kTopkBins3];
  lds_hist_clear(lh, kTopkBins3);
  const unsigned K = sel[1], b1 = sel[2], gt1 = sel[3];
  unsigned h[kTopkBins2 / 256], above, total, b2, gt2, cnt;
  hist_suffix<kTopkBins2>(h2, h, above, total);
  pick_bin<kTopkBins2>(h, above, K - gt1, b2, gt2, cnt);
  const unsigned prefix = (b1 << 11) | b2;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const unsigned key = topk_key(map[pix]);
    if ((key >> 10) != prefix) continue;
    const long long t = tgt[pix];
    if (t != ignore && t >= 0 && t < C) atomicAdd(&lh[key & (kTopkBins3 - 1)], 1u);
  }
  lds_hist_flush(lh, kTopkBins3, h3);
  if (blockIdx.x == 0 && threadIdx.x == 0) { sel[4] = b2; sel[5] = gt1 + gt2; }     // (sel[2:4] were read before pick_bin's barriers)
}
// Launch 4: the last digit = tau's key; n_gt and n_eq exactly from the histograms; the block partials of sum_{v > tau} v.  An uncounted
// pixel's stored 0 may lie above a negative tau: it adds 0.  Keys are compared, so a counted NaN reaches the sum.
__global__ __launch_bounds__(256) void topk_sum_kernel(const float* map, long long P, const unsigned* h3, const unsigned* sel, float* partial,
                                                        float* out2, long long* counts4) {
  const unsigned N = sel[0], K = sel[1], b1 = sel[2], b2 = sel[4], gt2 = sel[5];
  unsigned h[kTopkBins3 / 256], above, total, b3, gt3, n_eq;
  hist_suffix<kTopkBins3>(h3, h, above, total);
  pick_bin<kTopkBins3>(h, above, K - gt2, b3, gt3, n_eq);
  const unsigned tk = (b1 << 21) | (b2 << 10) | b3;
  float sum = 0.f;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const float v = map[pix];
    if (topk_key(v) > tk) sum += v;
  }
  block_partial2(sum, 0.f, partial);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts4[0] = K; counts4[1] = N; counts4[2] = gt2 + gt3; counts4[3] = n_eq;
    out2[1] = N ? topk_unkey(tk) : 0.f;
  }
}
__global__ __launch_bounds__(256) void topk_fin_kernel(const float* partial, int blocks, float* out2, const long long* counts4) {
  float a, b;
  fold_partials(partial, blocks, a, b);
  if (threadIdx.x == 0) out2[0] = topk_value(a, counts4[0], counts4[2], out2[1]);
}
// dl (=|+=) (g a w)(p - y): a = 1 above tau, (K - n_gt) / n_eq on it, 0 below (those pixels get a plain 0 / keep their old value,
// without a look at their logits).  partial non-null (the step): block 0 also folds the sum's partials and writes the value, in
// topk_fin_kernel's order.
template <int C>
__global__ __launch_bounds__(256) void topk_bwd_kernel(const float* logits, const long long* tgt, long long P, int ignore, const float* weight,
                                                        const float* map, const float* out2, const long long* counts4, const float* partial,
                                                        int blocks, float* value_out, const float* gscale, float gmul, float* dl, int acc) {
  const long long K = counts4[0], n_gt = counts4[2], n_eq = counts4[3];
  const float tau = out2[1];
  if (partial && blockIdx.x == 0) {
    float a, b;
    fold_partials(partial, blocks, a, b);
    if (threadIdx.x == 0) value_out[0] = topk_value(a, K, n_gt, tau);
  }
  const WeightedRule<C> rule(ignore, weight, 0.f);
  const float g = (gscale ? gscale[0] : 1.f) * gmul / (float)K;
  const float share = (float)(K - n_gt) / (float)n_eq;
  const unsigned tk = topk_key(tau);
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const unsigned key = topk_key(map[pix]);
    float d[C];
    if (key < tk) {
      if (acc) continue;
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = 0.f;
    } else {
      rule.grad(logits, pix, tgt[pix], key > tk ? g : g * share, d);
    }
    store_px<C>(dl, pix, d, acc);
  }
}

// ---- boundary loss: the softmax weighted by the signed distance map (the rule: include/dct.h, dct_boundary_*) --------------------------
// phi has the layout of the logits: both are read with the same loads (16 bytes at C = 4, two of them at C = 8).
template <int C> __device__ __forceinline__ void load_px16(const float* p, long long pix, float v[C]) {
  if constexpr (C == 8) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + pix * 8), u = *reinterpret_cast<const f32x4*>(p + pix * 8 + 4);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; v[4] = u[0]; v[5] = u[1]; v[6] = u[2]; v[7] = u[3];
  } else {
    load_px<C>(p, pix, v);
  }
}
// partial[2b] = the block's sum over counted pixels of sum_{c in mask} s_c phi_c, partial[2b + 1] = its number of counted pixels
template <int C>
__global__ __launch_bounds__(256) void bd_fwd_kernel(const float* logits, const long long* tgt, const float* phi, long long P, int ignore, int mask,
                                                      float* partial) {
  float sum = 0.f, cnt = 0.f;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    if (!counted<C>(tgt[pix], ignore)) continue;
    float x[C], p[C], f[C];
    load_px16<C>(logits, pix, x);
    load_px16<C>(phi, pix, f);
    softmax_px<C>(x, p);
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) if (mask >> c & 1) a = fmaf(p[c], f[c], a);
    sum += a; cnt += 1.f;
  }
  block_partial2(sum, cnt, partial);
}
// finalize_kernel's fold; out[0] = sum / (N K), 0 when nothing is counted; out[1] = N
__global__ __launch_bounds__(256) void bd_finalize_kernel(const float* partial, int blocks, float* out, float K) {
  float a, b;
  fold_partials(partial, blocks, a, b);
  if (threadIdx.x == 0) {
    out[0] = b > 0.f ? a / (b * K) : 0.f;
    out[1] = b;
  }
}
// dl (=|+=) (g s_c) (q_c - sum_k s_k q_k), q_c = m_c phi_c / (N K); an uncounted pixel gets 0 (N = 0: every pixel is uncounted)
template <int C>
__global__ __launch_bounds__(256) void bd_bwd_kernel(const float* logits, const long long* tgt, const float* phi, long long P, int ignore, int mask,
                                                      float K, const float* count, const float* gscale, float gmul, float* dl, int acc) {
  const float g = (gscale ? gscale[0] : 1.f) * gmul;
  const float nk = count[0] * K;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    const bool on = counted<C>(tgt[pix], ignore);
    float x[C], p[C], q[C], d[C];
    load_px16<C>(logits, pix, x);
    load_px16<C>(phi, pix, q);
    softmax_px<C>(x, p);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      q[c] = (mask >> c & 1) ? q[c] / nk : 0.f;
      dot = fmaf(p[c], q[c], dot);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = on ? (g * p[c]) * (q[c] - dot) : 0.f;
    store_px<C>(dl, pix, d, acc);
  }
}

// ---- the overlap criteria: soft Dice, Tversky and focal Tversky, alone or beside CE (the rules: include/dct.h) -------------------------------
// One kernel family over a rule (DiceTerms, TverskyTerms): the rule is the step from a group's sums {I, S, Y} to (index, term, qa, qb) and
// the line from the masked sum of terms to the reported value, evaluated per block (and by one thread per group for the outputs), never
// per pixel.  The forward kernel, the folds and the per-pixel gradient know no rule.
// Grid: x walks one image's pixels, y is the image (dice_kernel's choice), so a block's partial row is one image's and a group's sums
// depend on that group's pixels alone.  A row is NS = 3 C + 2 floats: {sum w l, sum w, then I, S, Y per class}.  A sum is folded in one
// fixed order wherever it is formed: over all rows by a block (fold_rows: thread tid takes rows tid, tid + 256, ... in order, then the wave
// shuffle, then the four wave sums), over one image's rows by a wave (wave_fold_rows).
constexpr int kDiceFwdBlocks = 512;      // rows every backward block folds: kept small (the fold is L2 traffic per backward block)
constexpr int kDiceBwdBlocks = 1024;
// what every overlap rule shares: coef weighs the overlap term beside ce_coef's cross entropy, inv_gk = 1 / (G K)
struct OverlapArgs { int mask, per_image; float smooth, ce_coef, coef, inv_gk; };

template <int N> __device__ __forceinline__ void block_partial_n(const float a[N], float* row) {
  __shared__ float sm[4 * N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const float v = wave_sum(a[s]);
    if (lane == 0) sm[w * N + s] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) row[threadIdx.x] = sm[threadIdx.x] + sm[N + threadIdx.x] + sm[2 * N + threadIdx.x] + sm[3 * N + threadIdx.x];
}
// out[s] = the sum over rows [first, first + count) of column OFF + s, in every thread of the block (sm: 4 N floats of LDS)
template <int NS, int OFF, int N>
__device__ __forceinline__ void fold_rows(const float* partial, int first, int count, float* sm, float out[N]) {
  float a[N];
#pragma unroll
  for (int s = 0; s < N; ++s) a[s] = 0.f;
  for (int i = threadIdx.x; i < count; i += 256) {
    const float* row = partial + (long long)(first + i) * NS + OFF;
#pragma unroll
    for (int s = 0; s < N; ++s) a[s] += row[s];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();                       // (the previous fold's readers are done with sm)
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const float v = wave_sum(a[s]);
    if (lane == 0) sm[w * N + s] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < N; ++s) out[s] = sm[s] + sm[N + s] + sm[2 * N + s] + sm[3 * N + s];
}
// The same sums by ONE wave, in every lane: lane l takes rows l, l + 64, ... in order, then the wave shuffle.  This is the order of a group's
// sums under per_image (a group is one image's rows, at most kDiceFwdBlocks / B of them): no LDS and no barrier, so the four waves of
// overlap_finish fold four groups at a time and a backward block's waves each fold their image's rows for themselves.
template <int NS, int OFF, int N>
__device__ __forceinline__ void wave_fold_rows(const float* partial, int first, int count, float out[N]) {
  float a[N];
#pragma unroll
  for (int s = 0; s < N; ++s) a[s] = 0.f;
  for (int i = threadIdx.x & 63; i < count; i += 64) {
    const float* row = partial + (long long)(first + i) * NS + OFF;
#pragma unroll
    for (int s = 0; s < N; ++s) a[s] += row[s];
  }
#pragma unroll
  for (int s = 0; s < N; ++s) out[s] = wave_sum(a[s]);
}
// {sum w l, sum w} over every row and group g's {I, S, Y} per class: the one group of the whole batch folds all columns of all rows at once
template <int C>
__device__ __forceinline__ void overlap_fold(const float* partial, int B, int fbx, int per_image, int g, float* sm, float ce2[2], float d[3 * C]) {
  constexpr int NS = 3 * C + 2;
  if (!per_image) {
    float a[NS];
    fold_rows<NS, 0, NS>(partial, 0, B * fbx, sm, a);
    ce2[0] = a[0]; ce2[1] = a[1];
#pragma unroll
    for (int s = 0; s < 3 * C; ++s) d[s] = a[2 + s];
  } else {
    fold_rows<NS, 0, 2>(partial, 0, B * fbx, sm, ce2);
    wave_fold_rows<NS, 2, 3 * C>(partial, g * fbx, fbx, d);
  }
}
// A rule's terms(I, S, Y, smooth, m, index, term, a, b): the index reported per group and class, the term whose masked sum makes the value,
// and the gradient's coefficients a, b with the weight m = m_c / (G K) folded in (q_c = b_c - [t == c] a_c); value(): the reported value
// from the masked sum of terms.  One rounding per operation wherever they are inlined: _step's numbers are _fwd's and _bwd's.
// Dice: D = (2 I + smooth) / (S + Y + smooth) is index and term, a = m 2 / den, b = m D / den; an empty denominator: D = 1, no gradient.
struct DiceTerms {
  __device__ __forceinline__ void terms(float I, float S, float Y, float smooth, float m, float& D, float& term, float& a, float& b) const {
#pragma clang fp contract(off)
    const float den = (S + Y) + smooth;
    const float num = 2.f * I + smooth;
    const bool empty = den == 0.f;
    D = term = empty ? 1.f : num / den;
    a = m * (empty ? 0.f : 2.f / den);
    b = m * (empty ? 0.f : D / den);
  }
  static __device__ __forceinline__ float value(float sum, float inv_gk) {
#pragma clang fp contract(off)
    return 1.f - sum * inv_gk;
  }
};
// Tversky: T = (I + smooth) / Den, Den = c0 I + alpha S + beta Y + smooth in the order written; term = u^e with u = max(1 - T, 0) (u when
// !focal); with f = m e u^(e - 1) (m when !focal): a = f (1 - c0 T) / Den, b = f alpha T / Den.  Den == 0: T = 1; Den == 0 or u == 0:
// term = a = b = 0.  c0 = fl(1 - alpha - beta) and e = fl(1 / gamma), formed on the host in double; focal = gamma != 1 (gamma == 1
// evaluates no power function).
struct TverskyTerms {
  float alpha, beta, c0, e;
  int focal;
  __device__ __forceinline__ void terms(float I, float S, float Y, float smooth, float m, float& T, float& term, float& a, float& b) const {
#pragma clang fp contract(off)
    const float den = ((c0 * I + alpha * S) + beta * Y) + smooth;
    const float num = I + smooth;
    const bool empty = den == 0.f;
    const float ds = empty ? 1.f : den;
    T = empty ? 1.f : num / ds;
    const float u = fmaxf(1.f - T, 0.f);
    const bool some = u > 0.f;                                             // (false under an empty denominator: T = 1)
    const float us = some ? u : 1.f;
    float pw = us, f = m;
    if (focal) {                                                           // (the same in every lane)
      const float lg = log2f(us);
      pw = exp2f(e * lg);
      f = (m * e) * exp2f((e - 1.f) * lg);
    }
    term = some ? pw : 0.f;
    a = some ? (f * (1.f - c0 * T)) / ds : 0.f;
    b = some ? ((f * alpha) * T) / ds : 0.f;
  }
  static __device__ __forceinline__ float value(float sum, float inv_gk) {
#pragma clang fp contract(off)
    return sum * inv_gk;
  }
};
// q_c = qb[c] - [t == c] qa[c] from a group's folded sums d = {I, S, Y} per class
template <int C, class Rule> __device__ __forceinline__ void overlap_coeffs(const float* d, OverlapArgs r, Rule rule, float qa[C], float qb[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float index, term;
    rule.terms(d[3 * c], d[3 * c + 1], d[3 * c + 2], r.smooth, ((r.mask >> c) & 1) ? r.inv_gk : 0.f, index, term, qa[c], qb[c]);
  }
}
// group g's rows of index_gc [G][C] and sums [G][C][3] from its folded sums (one thread); -> the sum of the terms over the classes of the mask
template <int C, class Rule>
__device__ __forceinline__ float overlap_group_out(const float d[3 * C], int g, OverlapArgs r, Rule rule, float* index_gc, float* sums) {
  float tsum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    float index, term, a, b;
    rule.terms(d[3 * c], d[3 * c + 1], d[3 * c + 2], r.smooth, 0.f, index, term, a, b);
    index_gc[g * C + c] = index;
    sums[(g * C + c) * 3 + 0] = d[3 * c]; sums[(g * C + c) * 3 + 1] = d[3 * c + 1]; sums[(g * C + c) * 3 + 2] = d[3 * c + 2];
    if ((r.mask >> c) & 1) tsum += term;
  }
  return tsum;
}
// out4 = {total, ce, sum w, value}, index_gc and sums from the partial rows; the whole block calls it.  Under per_image wave w takes groups
// w, w + 4, ... and the four waves' sums of terms are added in order.
template <int C, class Rule>
__device__ __forceinline__ void overlap_finish(const float* partial, int B, int fbx, OverlapArgs r, Rule rule, float* out4, float* index_gc,
                                               float* sums, float* sm) {
  constexpr int NS = 3 * C + 2;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float ce2[2], d[3 * C], tsum = 0.f;
  if (!r.per_image) {
    overlap_fold<C>(partial, B, fbx, 0, 0, sm, ce2, d);
    if (threadIdx.x == 0) tsum = overlap_group_out<C>(d, 0, r, rule, index_gc, sums);
  } else {
    fold_rows<NS, 0, 2>(partial, 0, B * fbx, sm, ce2);
    for (int g = w; g < B; g += 4) {
      wave_fold_rows<NS, 2, 3 * C>(partial, g * fbx, fbx, d);
      if (lane == 0) tsum += overlap_group_out<C>(d, g, r, rule, index_gc, sums);
    }
    __syncthreads();                     // (fold_rows' readers are done with sm)
    if (lane == 0) sm[w] = tsum;
    __syncthreads();
    tsum = sm[0] + sm[1] + sm[2] + sm[3];
  }
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    const float ce = ce2[0] / ce2[1];
    const float value = Rule::value(tsum, r.inv_gk);
    float total = 0.f;
    if (r.ce_coef != 0.f) total = r.ce_coef * ce;            // a coefficient of exactly 0 removes its term (a NaN ce with it)
    if (r.coef != 0.f) total = total + r.coef * value;
    out4[0] = total; out4[1] = ce; out4[2] = ce2[1]; out4[3] = value;
  }
}
// dl (=|+=) g (ce_coef (w_t / den)(p - y) + coef p (q - sum_k p_k q_k)) over the block's pixels of image blockIdx.y
template <int C>
__device__ __forceinline__ void overlap_grad_pixels(const float* logits, const long long* tgt, long long PPI, int ignore, const float wr[C],
                                                    float g, float den, OverlapArgs r, const float qa[C], const float qb[C], float* dl, int acc) {
  const bool ce_on = r.ce_coef != 0.f, dice_on = r.coef != 0.f;
  const float gce = ce_on ? g * r.ce_coef / den : 0.f;
  const float gd = g * r.coef;
  const long long base = (long long)blockIdx.y * PPI;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < PPI; pix += (long long)gridDim.x * 256) {
    const long long t = tgt[base + pix];
    const bool on = counted<C>(t, ignore);
    float x[C], p[C], q[C], d[C];
    load_px<C>(logits, base + pix, x);
    softmax_px<C>(x, p);
    const float gw = gce * weight_of<C>(t, wr);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { q[c] = qb[c] - (t == c ? qa[c] : 0.f); dot += p[c] * q[c]; }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float a = ce_on ? gw * (p[c] - (t == c ? 1.f : 0.f)) : 0.f;
      const float b = dice_on ? gd * (p[c] * (q[c] - dot)) : 0.f;
      d[c] = on ? a + b : 0.f;
    }
    store_px<C>(dl, base + pix, d, acc);
  }
}
// one softmax per counted pixel feeds both terms: WeightedRule's {w l, w} and {p_t, p_c, [t == c]} per class
template <int C>
__global__ __launch_bounds__(256) void overlap_fwd_kernel(const float* logits, const long long* tgt, long long PPI, int ignore,
                                                           const float* weight, float* partial) {
  constexpr int NS = 3 * C + 2;
  float wr[C];
  load_weights<C>(weight, wr);
  float a[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) a[s] = 0.f;
  const long long base = (long long)blockIdx.y * PPI;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < PPI; pix += (long long)gridDim.x * 256) {
    const long long t = tgt[base + pix];
    if (!counted<C>(t, ignore)) continue;
    float x[C], p[C];
    load_px<C>(logits, base + pix, x);
    const float lse = softmax_px<C>(x, p);
    float xt = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) xt = (t == c) ? x[c] : xt;
    const float w = weight_of<C>(t, wr);
    a[0] += w * (lse - xt); a[1] += w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      a[2 + 3 * c] += (t == c) ? p[c] : 0.f;
      a[3 + 3 * c] += p[c];
      a[4 + 3 * c] += (t == c) ? 1.f : 0.f;
    }
  }
  block_partial_n<NS>(a, partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * NS);
}
template <int C, class Rule>
__global__ __launch_bounds__(256) void overlap_fin_kernel(const float* partial, int B, int fbx, OverlapArgs r, Rule rule, float* out4, float* index_gc,
                                                           float* sums) {
  __shared__ float sm[4 * (3 * C + 2)];
  overlap_finish<C>(partial, B, fbx, r, rule, out4, index_gc, sums, sm);
}
template <int C, class Rule>
__global__ __launch_bounds__(256) void overlap_bwd_kernel(const float* logits, const long long* tgt, long long PPI, int ignore, const float* weight,
                                                           OverlapArgs r, Rule rule, const float* out4, const float* sums, const float* gscale,
                                                           float gmul, float* dl, int acc) {
  float wr[C], qa[C], qb[C];
  load_weights<C>(weight, wr);
  overlap_coeffs<C>(sums + (r.per_image ? (long long)blockIdx.y * C * 3 : 0), r, rule, qa, qb);
  overlap_grad_pixels<C>(logits, tgt, PPI, ignore, wr, (gscale ? gscale[0] : 1.f) * gmul, out4[2], r, qa, qb, dl, acc);
}
// loss_bwd_fin_kernel's pattern: every block folds the forward rows it needs (all of them for sum w; its own group's for the overlap sums)
// in overlap_fin_kernel's order, block (0, 0) also writes what that kernel writes, then the gradient
template <int C, class Rule>
__global__ __launch_bounds__(256) void overlap_bwd_fin_kernel(const float* logits, const long long* tgt, long long PPI, int ignore,
                                                               const float* weight, OverlapArgs r, Rule rule, const float* partial, int fbx,
                                                               float* out4, float* index_gc, float* sums, const float* gscale, float gmul,
                                                               float* dl, int acc) {
  __shared__ float sm[4 * (3 * C + 2)];
  const int B = gridDim.y;
  float ce2[2], d[3 * C];
  overlap_fold<C>(partial, B, fbx, r.per_image, blockIdx.y, sm, ce2, d);
  if (blockIdx.x == 0 && blockIdx.y == 0) overlap_finish<C>(partial, B, fbx, r, rule, out4, index_gc, sums, sm);
  float wr[C], qa[C], qb[C];
  load_weights<C>(weight, wr);
  overlap_coeffs<C>(d, r, rule, qa, qb);
  overlap_grad_pixels<C>(logits, tgt, PPI, ignore, wr, (gscale ? gscale[0] : 1.f) * gmul, ce2[1], r, qa, qb, dl, acc);
}

// ---- softmax / entropy (module API) -------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* logits, float* probs, long long P) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float x[C], p[C];
    load_px<C>(logits, pix, x);
    softmax_px<C>(x, p);
    store_px<C>(probs, pix, p, false);
  }
}
template <int C>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* probs, const float* dprobs, float* dl, long long P, int acc) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float p[C], d[C], o[C];
    load_px<C>(probs, pix, p);
    load_px<C>(dprobs, pix, d);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) dot += d[c] * p[c];
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = p[c] * (d[c] - dot);
    store_px<C>(dl, pix, o, acc);
  }
}
template <int C> __device__ __forceinline__ float entropy_px(const float p[C]) {
  float e = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) e += p[c] * logf(p[c] + kEntEps);
  return -e;
}
template <int C>
__global__ __launch_bounds__(256) void entropy_fwd_kernel(const float* probs, float* map, long long P) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float p[C];
    load_px<C>(probs, pix, p);
    map[pix] = entropy_px<C>(p);
  }
}

// d/dp of  H(p) = -sum p log(p+eps):  -(log(p+eps) + p/(p+eps))
__device__ __forceinline__ float dent(float p) { return -(logf(p + kEntEps) + p / (p + kEntEps)); }
template <int C>
__global__ __launch_bounds__(256) void entropy_bwd_kernel(const float* probs, const float* dmap, float* dprobs, long long P) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float p[C], d[C];
    load_px<C>(probs, pix, p);
    const float g = dmap[pix];
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = g * dent(p[c]);
    store_px<C>(dprobs, pix, d, false);
  }
}

// ---- JSD ------------------------------------------------------------------------------------------
// up to DCT_JSD_MAX_MODELS segmentators per call (the reference sweeps 2 / 4 / 6 views: script/GM/run_multiview.sh:2-6)
constexpr int MAXS = 8;
struct PtrPack { const float* in[MAXS]; float* out[MAXS]; };

template <int C, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void jsd_fwd_kernel(PtrPack pk, int S, long long P, float* map, float* partial) {
  float sum = 0.f;
  const float invS = 1.f / (float)S;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float mean[C];
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = 0.f;
    float hsum = 0.f;
    for (int s = 0; s < S; ++s) {
      float x[C], p[C];
      load_px<C>(pk.in[s], pix, x);
      if constexpr (FROM_LOGITS) softmax_px<C>(x, p);
      else {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = x[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) mean[c] += p[c];
      hsum += entropy_px<C>(p);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] *= invS;   // loss.py:193  reduce(+)/len
    const float j = entropy_px<C>(mean) - hsum * invS;
    if (map) map[pix] = j;
    sum += j;
  }
  if (partial) block_partial2(sum, 0.f, partial);
}
// FROM_LOGITS: dlogits_s (=|+=) g/P * softmax_bwd(dJ/dp_s);  else dprobs_s = dmap[pix] * dJ/dp_s
// SMAX: the models whose probabilities a thread keeps in registers (4: the co-training pairs / triples of the benchmark
// configurations; 8: the multi-view sweeps)
template <int C, bool FROM_LOGITS, int SMAX>
__global__ __launch_bounds__(256) void jsd_bwd_kernel(PtrPack pk, int S, long long P, const float* dmap, const float* gscale,
                                                       float gmul, int acc) {
  const float invS = 1.f / (float)S;
  float g = 0.f;
  if constexpr (FROM_LOGITS) g = (gscale ? gscale[0] : 1.f) * gmul / (float)P;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float p[SMAX][C], mean[C];
#pragma unroll
    for (int c = 0; c < C; ++c) mean[c] = 0.f;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < S) {
        float x[C];
        load_px<C>(pk.in[s], pix, x);
        if constexpr (FROM_LOGITS) softmax_px<C>(x, p[s]);
        else {
#pragma unroll
          for (int c = 0; c < C; ++c) p[s][c] = x[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) mean[c] += p[s][c];
      }
    }
    float dm[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { mean[c] *= invS; dm[c] = dent(mean[c]); }
    const float gp = FROM_LOGITS ? g : dmap[pix];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < S) {
        float d[C];
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = invS * (dm[c] - dent(p[s][c]));
        if constexpr (FROM_LOGITS) {
          float dot = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) dot += d[c] * p[s][c];
          float o[C];
#pragma unroll
          for (int c = 0; c < C; ++c) o[c] = gp * p[s][c] * (d[c] - dot);
          store_px<C>(pk.out[s], pix, o, acc);
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) d[c] *= gp;
          store_px<C>(pk.out[s], pix, d, false);
        }
      }
    }
  }
}

// The co-training step's whole JSD section in ONE pass over the logits (round 5): mean-JSD partial sums (jsd_fwd_kernel<C, true>'s, on its
// grid: same pixels per thread, same order -> the same block partials), the S softmax maps the step returns (softmax_fwd_kernel's) and the S
// logit gradients (jsd_bwd_kernel<C, true>'s arithmetic).  Five launches became two (this + the finalize) in the one stretch of the step where
// nothing else runs: both models' forward passes have just joined (tools/phase_stamps.py).  Bit-identical to the separate launches.
template <int C, int SMAX>
__global__ __launch_bounds__(256) void jsd_step_kernel(PtrPack pk, PtrPack probs, int S, long long P, const float* gscale, float gmul, int acc,
                                                        int want_grad, float* partial) {
  const float invS = 1.f / (float)S;
  const float g = (gscale ? gscale[0] : 1.f) * gmul / (float)P;
  float sum = 0.f;
  // Two of the thread's pixels per trip (two-model case), every load of both (logits and the gradients to add to) issued before the first store: with 1024 blocks
  // a thread walks 2+ pixels and the launch sits where nothing else runs -- the trip used to be six dependent memory round trips per pixel.
  // Per pixel the arithmetic and its order are those of the separate kernels; the thread's pixels are summed in the same order.
  constexpr int NP = SMAX <= 2 ? 2 : 1;       // (two pixels of four or eight models do not fit the register file)
  const long long stride = (long long)gridDim.x * 256;
  for (long long pix0 = (long long)blockIdx.x * 256 + threadIdx.x; pix0 < P; pix0 += NP * stride) {
    const bool two = NP == 2 && pix0 + stride < P;
    float x[NP][SMAX][C], old[NP][SMAX][C];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < S) {
        load_px<C>(pk.in[s], pix0, x[0][s]);
        if constexpr (NP == 2) { if (two) load_px<C>(pk.in[s], pix0 + stride, x[NP - 1][s]); }
        if (want_grad && acc) {
          load_px<C>(pk.out[s], pix0, old[0][s]);
          if constexpr (NP == 2) { if (two) load_px<C>(pk.out[s], pix0 + stride, old[NP - 1][s]); }
        }
      }
    }
#pragma unroll
    for (int h = 0; h < NP; ++h) {
      if (h == 1 && !two) continue;
      const long long pix = pix0 + h * stride;
      float p[SMAX][C], mean[C];
#pragma unroll
      for (int c = 0; c < C; ++c) mean[c] = 0.f;
      float hsum = 0.f;
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        if (s < S) {
          softmax_px<C>(x[h][s], p[s]);
#pragma unroll
          for (int c = 0; c < C; ++c) mean[c] += p[s][c];
          hsum += entropy_px<C>(p[s]);
          if (probs.out[s]) store_px<C>(probs.out[s], pix, p[s], false);
        }
      }
      float dm[C];
#pragma unroll
      for (int c = 0; c < C; ++c) mean[c] *= invS;
      sum += entropy_px<C>(mean) - hsum * invS;
      if (want_grad) {
#pragma unroll
        for (int c = 0; c < C; ++c) dm[c] = dent(mean[c]);
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
          if (s < S) {
            float d[C];
#pragma unroll
            for (int c = 0; c < C; ++c) d[c] = invS * (dm[c] - dent(p[s][c]));
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) dot += d[c] * p[s][c];
            float o[C];
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = g * p[s][c] * (d[c] - dot);
            if (acc) {
#pragma clang fp contract(off)    // store_px's accumulate: round, then add
#pragma unroll
              for (int c = 0; c < C; ++c) o[c] = o[c] + old[h][s][c];
            }
            store_px<C>(pk.out[s], pix, o, false);
          }
        }
      }
    }
  }
  block_partial2(sum, 0.f, partial);
}

// ---- view consistency: hard pseudo-labels, sharpened soft pseudo-labels, softmax-MSE (the rules: include/dct.h, dct_pl_* / dct_spl_* / dct_mse_*) ----
// One kernel family over a rule, as for the cross entropies above.  What every rule starts from exists once, so that first maximum,
// confidence and mask are the same compares on the same fp32 values under all three (include/dct.h promises them bit for bit):
// cross: every view j names k_j = first maximum of p_j and is kept when p_j[k_j] >= tau; ensemble: one teacher, the first maximum of the
// fp32 sums taken in view order, kept when sum[k] * invS >= tau.
// The mode is a uniform branch (a kernel argument), not a template parameter: the two derivations are a few compares per pixel of an
// HBM-bound pass, and everything behind them (logs, gradients, stores) is one code path.
// Nothing here may be addressed at run time (scratch): k is a compile-time-unrolled compare, never an index, and i, j are constants of
// unrolled loops.
// The first maximum of v: returns k, bv = v[k].
template <int C>
__device__ __forceinline__ int cons_first_max(const float (&v)[C], float& bv) {
  bv = v[0];
  int best = 0;
#pragma unroll
  for (int c = 1; c < C; ++c) if (v[c] > bv) { bv = v[c]; best = c; }
  return best;
}
// The ensemble's raw teacher: sum = the views added in view order, best / bv = its first maximum (on the unscaled sums: scaling cannot
// create a tie).  Returns the confidence q = sum[k] * invS.
template <int C, int SMAX>
__device__ __forceinline__ float cons_ensemble(const float (&p)[SMAX][C], int S, float invS, float (&sum)[C], int& best, float& bv) {
#pragma clang fp contract(off)    // the sums and q are formed from the ROUNDED probabilities, as the rule states them: no product of softmax_px may fold into an add here
#pragma unroll
  for (int c = 0; c < C; ++c) sum[c] = p[0][c];
#pragma unroll
  for (int s = 1; s < SMAX; ++s) {
    if (s < S) {
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = sum[c] + p[s][c];
    }
  }
  best = cons_first_max<C>(sum, bv);
  return bv * invS;
}
// Student i against n = terms(c) teacher terms of class c: returns sum_c n * -log(p[c] + eps) (the pixel's map value is wgt times the sum
// over i) and d[c] = d map / d p[c] = -(wgt n) / (p[c] + eps).  No term: no log, and d[c] = 0 exactly.  terms is a callable so that the
// hard rule forms its n inside this loop: an n[C] formed ahead of it costs the map kernel 6 registers and a wave per SIMD at C = 8.
template <int C, class Terms>
__device__ __forceinline__ float cons_log_student(const float (&p)[C], Terms terms, float eps, float wgt, float (&d)[C]) {
  float a = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float n = terms(c);
    d[c] = 0.f;
    if (n != 0.f) {
      const float pe = p[c] + eps;
      a -= n * logf(pe);
      d[c] = -(wgt * n) / pe;
    }
  }
  return a;
}

// A rule is what the three criteria differ in.  It carries its scalars (a kernel argument) and offers
//   State<C, SMAX>                                      the teachers of one pixel, as constants;
//   teachers(p, S, teacher, tau, invS, state) -> kept   fills the state, returns the number of kept teachers;
//   student(p, state, S, teacher, i, wgt, d) -> a       student i's value a_i (the map value is wgt times the sum over i) and
//                                                       d[c] = d map / d p_i[c]; i is a constant of the caller's unrolled loop;
//   kPerClass                                           whether the host's weight divides by C as well.
// Hard pseudo-labels (cross pseudo supervision / voted pseudo-label).  State: cnt[c] = the kept teachers that name class c, own[s] = the
// class view s named itself as a kept teacher (-1: none; a view is no teacher of itself), so that student s meets
// n = cnt[c] - (own[s] == c) teacher terms of class c.
struct HardRule {
  static constexpr bool kPerClass = false;
  float eps;
  template <int C, int SMAX> struct State { float cnt[C]; int own[SMAX]; };
  template <int C, int SMAX>
  __device__ __forceinline__ int teachers(const float (&p)[SMAX][C], int S, int teacher, float tau, float invS, State<C, SMAX>& st) const {
#pragma clang fp contract(off)    // as cons_ensemble: nothing here may fold a product of softmax_px into an add
    int kept = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) st.cnt[c] = 0.f;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) st.own[s] = -1;
    if (teacher == DCT_PL_CROSS) {
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        if (s < S) {
          float bv;
          const int best = cons_first_max<C>(p[s], bv);
          if (bv >= tau) {
            st.own[s] = best;
            ++kept;
#pragma unroll
            for (int c = 0; c < C; ++c) st.cnt[c] = st.cnt[c] + (best == c ? 1.f : 0.f);
          }
        }
      }
    } else {
      float sum[C], bv;
      int best;
      if (cons_ensemble<C, SMAX>(p, S, invS, sum, best, bv) >= tau) {
        kept = 1;
#pragma unroll
        for (int c = 0; c < C; ++c) st.cnt[c] = best == c ? 1.f : 0.f;
      }
    }
    return kept;
  }
  template <int C, int SMAX>
  __device__ __forceinline__ float student(const float (&p)[SMAX][C], const State<C, SMAX>& st, int, int, int i, float wgt, float (&d)[C]) const {
    return cons_log_student<C>(p[i], [&](int c) { return st.cnt[c] - (st.own[i] == c ? 1.f : 0.f); }, eps, wgt, d);
  }
};

// Sharpened soft pseudo-labels: Sharpen(q, T) in place of the argmax, r = 1 / T.  State: t[j] = m_j * Sharpen(p_j) for cross (0 for a
// masked view and for j >= S), t[0] = m * Sharpen(sum) for ensemble; the mask is on the raw confidence, and a masked teacher is never
// sharpened.  The S teachers are HELD (SMAX C floats) and not recomputed per student: recomputing costs S times the 2 C transcendentals
// of every teacher, holding costs 64 registers at SMAX = 8, C = 8, where the file of a 256-thread block (512 per lane) has them.
struct SoftRule {
  static constexpr bool kPerClass = false;
  float eps, r;
  template <int C, int SMAX> struct State { float t[SMAX][C]; };
  // Sharpen(q, T) of one raw teacher vector q with first maximum k (bv = q[k]): u[c] = exp2f(r (log2f(q[c]) - log2f(q[k]))), 0 where
  // q[c] == 0 and 1 exactly at k; t = u / (u[0] + ... + u[C-1]), added in class order.  Scale-free, so the ensemble hands in its
  // unscaled sums.
  template <int C>
  __device__ __forceinline__ void sharpen(const float (&q)[C], int k, float bv, float (&t)[C]) const {
#pragma clang fp contract(off)    // the argument of exp2f is the rounded product of the rounded difference, as the rule states it
    const float lk = log2f(bv);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float u = 1.f;
      if (c != k) u = q[c] == 0.f ? 0.f : exp2f(r * (log2f(q[c]) - lk));
      t[c] = u;
      sum = sum + u;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) t[c] = t[c] / sum;
  }
  template <int C, int SMAX>
  __device__ __forceinline__ int teachers(const float (&p)[SMAX][C], int S, int teacher, float tau, float invS, State<C, SMAX>& st) const {
#pragma clang fp contract(off)    // as cons_ensemble
    int kept = 0;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
#pragma unroll
      for (int c = 0; c < C; ++c) st.t[s][c] = 0.f;
    }
    if (teacher == DCT_PL_CROSS) {
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        if (s < S) {
          float bv;
          const int best = cons_first_max<C>(p[s], bv);
          if (bv >= tau) {
            ++kept;
            sharpen<C>(p[s], best, bv, st.t[s]);
          }
        }
      }
    } else {
      float sum[C], bv;
      int best;
      if (cons_ensemble<C, SMAX>(p, S, invS, sum, best, bv) >= tau) {
        kept = 1;
        sharpen<C>(sum, best, bv, st.t[0]);
      }
    }
    return kept;
  }
  // n[c] of student i: cross: the other views' kept teachers added in ascending j (formed as that sum, never as a total minus the
  // student's own share: (t_0 + t_1) - t_0 is not t_1); ensemble: the one teacher.
  template <int C, int SMAX>
  __device__ __forceinline__ float student(const float (&p)[SMAX][C], const State<C, SMAX>& st, int S, int teacher, int i, float wgt, float (&d)[C]) const {
    float n[C];
    {
#pragma clang fp contract(off)
      if (teacher == DCT_PL_CROSS) {
#pragma unroll
        for (int c = 0; c < C; ++c) n[c] = 0.f;
#pragma unroll
        for (int j = 0; j < SMAX; ++j) {
          if (j < S && j != i) {
#pragma unroll
            for (int c = 0; c < C; ++c) n[c] = n[c] + st.t[j][c];
          }
        }
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) n[c] = st.t[0][c];
      }
    }
    return cons_log_student<C>(p[i], [&](int c) { return n[c]; }, eps, wgt, d);
  }
};

// Softmax-MSE: the squared distance to the other views' (or the mean) prediction; no scalar of its own.  State: cross: m[j] =
// p_j[k_j] >= tau (false for j >= S); ensemble: q[c] = sum[c] * invS and m[0] = q[k] >= tau.
struct MseRule {
  static constexpr bool kPerClass = true;
  template <int C, int SMAX> struct State { bool m[SMAX]; float q[C]; };
  template <int C, int SMAX>
  __device__ __forceinline__ int teachers(const float (&p)[SMAX][C], int S, int teacher, float tau, float invS, State<C, SMAX>& st) const {
#pragma clang fp contract(off)    // as cons_ensemble: q is formed from the ROUNDED sums
    int kept = 0;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) st.m[s] = false;
#pragma unroll
    for (int c = 0; c < C; ++c) st.q[c] = 0.f;
    if (teacher == DCT_PL_CROSS) {
#pragma unroll
      for (int s = 0; s < SMAX; ++s) {
        if (s < S) {
          float bv;
          cons_first_max<C>(p[s], bv);
          if (bv >= tau) { st.m[s] = true; ++kept; }
        }
      }
    } else {
      float sum[C], bv;
      int best;
      const float conf = cons_ensemble<C, SMAX>(p, S, invS, sum, best, bv);
#pragma unroll
      for (int c = 0; c < C; ++c) st.q[c] = sum[c] * invS;
      if (conf >= tau) { st.m[0] = true; kept = 1; }
    }
    return kept;
  }
  // Every difference is the difference of two probabilities (never a total minus the student's own share), every square a rounded
  // product added in class order, a masked teacher's differences are 0.  Only d[C] and two sums are live beside the probabilities.
  template <int C, int SMAX>
  __device__ __forceinline__ float student(const float (&p)[SMAX][C], const State<C, SMAX>& st, int S, int teacher, int i, float wgt, float (&d)[C]) const {
#pragma clang fp contract(off)    // the squares are rounded before they are added, as the rule states them and as the reference bounds them
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = 0.f;
    if (teacher == DCT_PL_CROSS) {
#pragma unroll
      for (int j = 0; j < SMAX; ++j) {
        if (j < S && j != i) {
          float sq = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float e = st.m[j] ? p[i][c] - p[j][c] : 0.f;
            sq = sq + e * e;
            d[c] = d[c] + e;
          }
          a = a + sq;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float e = st.m[0] ? p[i][c] - st.q[c] : 0.f;
        a = a + e * e;
        d[c] = e;
      }
    }
    const float w2 = 2.f * wgt;
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = w2 * d[c];
    return a;
  }
};

// What the three kernels take beside the rule: wgt = the weight of one teacher term in the map (1 / (S (S - 1)) resp. 1 / S, divided by C
// as well under kPerClass), kden = the teacher terms of a pixel (cross: S, ensemble: 1)
struct ConsArgs { int S, teacher; float tau, invS, wgt, kden; long long P; };

// The map over S probability maps, and optionally the per-pixel kept fraction
template <int C, int SMAX, class Rule>
__global__ __launch_bounds__(256) void cons_map_fwd_kernel(Rule rule, ConsArgs ca, PtrPack pk, float* map, float* keptmap) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < ca.P; pix += (long long)gridDim.x * 256) {
    float p[SMAX][C];
    typename Rule::template State<C, SMAX> st;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) load_px<C>(pk.in[s], pix, p[s]);
    }
    const int kept = rule.teachers(p, ca.S, ca.teacher, ca.tau, ca.invS, st);
    float a = 0.f;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) {
        float d[C];
        a += rule.student(p, st, ca.S, ca.teacher, s, ca.wgt, d);
      }
    }
    map[pix] = ca.wgt * a;
    if (keptmap) keptmap[pix] = (float)kept / ca.kden;
  }
}
// dprobs_s = dmap[pix] * d map / d p_s, the teachers recomputed from the probabilities
template <int C, int SMAX, class Rule>
__global__ __launch_bounds__(256) void cons_map_bwd_kernel(Rule rule, ConsArgs ca, PtrPack pk, const float* dmap) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < ca.P; pix += (long long)gridDim.x * 256) {
    float p[SMAX][C];
    typename Rule::template State<C, SMAX> st;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) load_px<C>(pk.in[s], pix, p[s]);
    }
    const float gp = dmap[pix];
    rule.teachers(p, ca.S, ca.teacher, ca.tau, ca.invS, st);
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) {
        float d[C];
        rule.student(p, st, ca.S, ca.teacher, s, ca.wgt, d);
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = d[c] != 0.f ? gp * d[c] : 0.f;     // a masked entry is 0 whatever dmap holds
        store_px<C>(pk.out[s], pix, d, false);
      }
    }
  }
}
// The step's consistency section from logits in one pass, on jsd_step_kernel's structure and grid: block partials of (map value, kept
// teachers) for pl_finalize_kernel, the S softmax maps (softmax_fwd_kernel's bits) and the S logit gradients g p (d - sum_c' d p)
// (jsd_bwd_kernel<_, true>'s form; accumulate: round, then add).  One pixel per trip, every load of the pixel issued before its first store.
template <int C, int SMAX, class Rule>
__global__ __launch_bounds__(256) void cons_step_kernel(Rule rule, ConsArgs ca, PtrPack pk, PtrPack probs, const float* gscale, float gmul, int acc,
                                                         int want_grad, float* partial) {
  const float g = (gscale ? gscale[0] : 1.f) * gmul / (float)ca.P;
  float sum = 0.f, keptsum = 0.f;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < ca.P; pix += (long long)gridDim.x * 256) {
    float x[SMAX][C], old[SMAX][C];
    // More than two views: nothing outstanding at the top of a trip.  The compiler's wait-count pass does not know that a view's load
    // and its use hang on the same uniform guard, so it carries the loads of the last trip across the back edge as pending; where the
    // register allocator forms a load's address in the load's own destination registers (it does for the vector loads of C = 2 and 4,
    // or not, from one build to the next), that puts a vmcnt(0) in front of every view's loads: eight round trips in a row in place of
    // one (measured: 3-6 % of the call at five views).  The two-view kernels the trainer launches show none of it and stay as they were.
    if constexpr (SMAX > 2) __builtin_amdgcn_s_waitcnt(0x0f70);       // vmcnt(0), the other counters left alone
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) {
        load_px<C>(pk.in[s], pix, x[s]);
        if (want_grad && acc) load_px<C>(pk.out[s], pix, old[s]);
      }
    }
    float p[SMAX][C];
    typename Rule::template State<C, SMAX> st;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) {
        softmax_px<C>(x[s], p[s]);
        if (probs.out[s]) store_px<C>(probs.out[s], pix, p[s], false);
      }
    }
    keptsum += (float)rule.teachers(p, ca.S, ca.teacher, ca.tau, ca.invS, st);
    float a = 0.f;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
      if (s < ca.S) {
        float d[C];
        a += rule.student(p, st, ca.S, ca.teacher, s, ca.wgt, d);
        if (want_grad) {
          float dot = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) dot += d[c] * p[s][c];
          float o[C];
#pragma unroll
          for (int c = 0; c < C; ++c) o[c] = g * p[s][c] * (d[c] - dot);
          if (acc) {
#pragma clang fp contract(off)    // store_px's accumulate: round, then add
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = o[c] + old[s][c];
          }
          store_px<C>(pk.out[s], pix, o, false);
        }
      }
    }
    sum += ca.wgt * a;
  }
  block_partial2(sum, keptsum, partial);
}
// finalize_kernel's fold with a denominator of its own for each sum: out[0] = mean map value, out[1] = kept teacher terms / all of them
// (the kept counts are whole numbers held in floats: exact up to 2^24 terms)
__global__ __launch_bounds__(256) void pl_finalize_kernel(const float* partial, int blocks, float* out, float denom_a, float denom_b) {
  float a, b;
  fold_partials(partial, blocks, a, b);
  if (threadIdx.x == 0) { out[0] = a / denom_a; out[1] = b / denom_b; }
}

// ---- KL(y || p) -----------------------------------------------------------------------------------
template <int C, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void kl_fwd_kernel(const float* pin, const float* yin, long long P, float eps, float* map, float* partial) {
  float sum = 0.f;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float a[C], b[C], p[C], y[C];
    load_px<C>(pin, pix, a);
    load_px<C>(yin, pix, b);
    if constexpr (FROM_LOGITS) { softmax_px<C>(a, p); softmax_px<C>(b, y); }
    else {
#pragma unroll
      for (int c = 0; c < C; ++c) { p[c] = a[c]; y[c] = b[c]; }
    }
    float ylogy = 0.f, ylogp = 0.f;   // loss.py:127-130
#pragma unroll
    for (int c = 0; c < C; ++c) { ylogy += y[c] * logf(y[c] + eps); ylogp += y[c] * logf(p[c] + eps); }
    const float k = ylogy - ylogp;
    if (map) map[pix] = k;
    sum += k;
  }
  if (partial) block_partial2(sum, 0.f, partial);
}
template <int C, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void kl_bwd_kernel(const float* pin, const float* yin, long long P, float eps, const float* dmap,
                                                      const float* gscale, float gmul, float* dout, int acc) {
  float g = 0.f;
  if constexpr (FROM_LOGITS) g = (gscale ? gscale[0] : 1.f) * gmul / (float)P;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float a[C], b[C], p[C], y[C], d[C];
    load_px<C>(pin, pix, a);
    load_px<C>(yin, pix, b);
    if constexpr (FROM_LOGITS) { softmax_px<C>(a, p); softmax_px<C>(b, y); }
    else {
#pragma unroll
      for (int c = 0; c < C; ++c) { p[c] = a[c]; y[c] = b[c]; }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = -y[c] / (p[c] + eps);
    if constexpr (FROM_LOGITS) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) dot += d[c] * p[c];
      float o[C];
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = g * p[c] * (d[c] - dot);
      store_px<C>(dout, pix, o, acc);
    } else {
      const float gp = dmap[pix];
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] *= gp;
      store_px<C>(dout, pix, d, false);
    }
  }
}

// ---- argmax / dice / fgsm / adam ---------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void argmax_kernel(const float* x, long long* cls, long long P) {
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < P; pix += (long long)gridDim.x * 256) {
    float v[C];
    load_px<C>(x, pix, v);
    int best = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) if (v[c] > v[best]) best = c;
    cls[pix] = best;
  }
}
template <int C>
__global__ __launch_bounds__(256) void dice_kernel(const float* logits, const long long* gt, long long PPI,
                                                    int* inter, int* psum, int* gsum) {
  __shared__ int h[3 * C];
  if (threadIdx.x < 3 * C) h[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const float* lb = logits + (long long)b * PPI * C;
  const long long* gb = gt + (long long)b * PPI;
  int li[C], lp[C], lg[C];
#pragma unroll
  for (int c = 0; c < C; ++c) { li[c] = 0; lp[c] = 0; lg[c] = 0; }
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < PPI; pix += (long long)gridDim.x * 256) {
    float v[C];
    load_px<C>(lb, pix, v);
    int best = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) if (v[c] > v[best]) best = c;
    const long long t = gb[pix];
#pragma unroll
    for (int c = 0; c < C; ++c) { lp[c] += best == c; lg[c] += t == c; li[c] += (best == c) && (t == c); }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (li[c]) atomicAdd(&h[c], li[c]);
    if (lp[c]) atomicAdd(&h[C + c], lp[c]);
    if (lg[c]) atomicAdd(&h[2 * C + c], lg[c]);
  }
  __syncthreads();
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    if (h[c]) atomicAdd(&inter[b * C + c], h[c]);
    if (h[C + c]) atomicAdd(&psum[b * C + c], h[C + c]);
    if (h[2 * C + c]) atomicAdd(&gsum[b * C + c], h[2 * C + c]);
  }
}

__global__ __launch_bounds__(256) void fgsm_kernel(const float* x, const float* g, float eps, float* xa, float* noise, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float gv = g[i];
    const float s = gv > 0.f ? eps : (gv < 0.f ? -eps : 0.f);   // eps*sign(g), sign(0)=0  (AEGenerator.py:42-45)
    if (noise) noise[i] = s;
    xa[i] = x[i] + s;
  }
}

// omb1/omb2 = 1-beta computed in double on the host, as torch does (float(1-0.999) != 1.f-0.999f)
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float step_size, float bc2s, float omb1, float b2, float omb2, float eps, float wd, float gs) {
  g = fmaf(wd, p, g * gs);                      // gs: 1, or the inverse power-of-two loss scale of an fp16 step (exact)
  m = m + (g - m) * omb1;                       // exp_avg.lerp_(grad, 1-b1)
  v = v * b2 + omb2 * g * g;                    // mul_(b2).addcmul_(g, g, 1-b2)
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}
// state (nullable): device-resident {step count t, learning rate, table base, table length} (doubles).  When given,
// the step-dependent scalars come from device memory so that a captured HIP graph of the step needs no per-step
// host value: table[2*(t-base-1)] = {1 - beta1^t, sqrt(1 - beta2^t)} as the HOST computed them (doubles; the step size
// lr / bc1 is then the same correctly rounded division the host does: bit-identical to the scalar-argument path, and a
// learning-rate change touches only state[1]); outside the table they are formed here in double.
__device__ __forceinline__ void adam_body(float* p, const float* g, float* m, float* v, long long n, float step_size,
                                          float bc2s, float omb1, float b2, float omb2, float eps, float wd, float gs, bf16_t* shadow,
                                          const double* state, const double* table, double beta1, double beta2) {
  if (state) {
    const double t = state[0], lr = state[1];
    const long long idx = (long long)t - (long long)state[2] - 1;
    if (table && idx >= 0 && idx < (long long)state[3]) {
      step_size = (float)(lr / table[2 * idx]);        // the division the host does (lr / bc1 in double, then fp32)
      bc2s = (float)table[2 * idx + 1];
    } else {
      step_size = (float)(lr / (1.0 - pow(beta1, t)));
      bc2s = (float)sqrt(1.0 - pow(beta2, t));
    }
  }
  const long long n4 = n / 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pp = pv[k], mm = mv[k], v2 = vv[k];
      adam1(pp, gv[k], mm, v2, step_size, bc2s, omb1, b2, omb2, eps, wd, gs);
      pv[k] = pp; mv[k] = mm; vv[k] = v2;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv; reinterpret_cast<f32x4*>(m)[i] = mv; reinterpret_cast<f32x4*>(v)[i] = vv;
    if (shadow) {
      bf16x4 s;
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = (bf16_t)pv[k];
      reinterpret_cast<bf16x4*>(shadow)[i] = s;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long long i = n4 * 4 + threadIdx.x;
    float pp = p[i], mm = m[i], v2 = v[i];
    adam1(pp, g[i], mm, v2, step_size, bc2s, omb1, b2, omb2, eps, wd, gs);
    p[i] = pp; m[i] = mm; v[i] = v2;
    if (shadow) shadow[i] = (bf16_t)pp;
  }
}
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long long n, float step_size,
                                                    float bc2s, float omb1, float b2, float omb2, float eps, float wd, float gs, bf16_t* shadow,
                                                    const double* state, const double* table, double beta1, double beta2) {
  adam_body(p, g, m, v, n, step_size, bc2s, omb1, b2, omb2, eps, wd, gs, shadow, state, table, beta1, beta2);
}

__global__ void adam_advance_kernel(double* state) { state[0] += 1.0; }

// ---- the guard in front of the update (dct_adam_guard, include/dct.h) ------------------------------------------------------------
// Sum of squares of g[0..n), one double partial per block.  A finite fp32 squared is exact in double and cannot overflow there, so a
// partial is non-finite iff its block read an inf or a NaN (squares are >= 0 or NaN: +inf and -inf cannot cancel).  One read of the
// buffer at full occupancy (8 blocks of 256 per CU at the largest grid), two 16-byte loads in flight per thread; each thread adds its
// elements in ascending order, the block folds lanes (xor 32 .. 1), then its four waves in order: the same buffer gives the same bits.
constexpr int kSumsqMaxBlocks = 2048;
static inline unsigned sumsq_grid(long long n) {
  long long b = (n / 4 + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > kSumsqMaxBlocks ? kSumsqMaxBlocks : b));
}
__device__ __forceinline__ void sumsq4(double& acc, const f32x4 gv) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { const double d = (double)gv[k]; acc = fma(d, d, acc); }
}
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* g, long long n, double* partials) {
  __shared__ double sw[4];
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  const long long n4 = n / 4, stride = (long long)gridDim.x * 256;
  double acc = 0.0;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const f32x4 a = g4[i], b = g4[i + stride];
    sumsq4(acc, a);
    sumsq4(acc, b);
  }
  if (i < n4) sumsq4(acc, g4[i]);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const double d = (double)g[n4 * 4 + threadIdx.x]; acc = fma(d, d, acc); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// One block of 256: thread t adds partials t, t + 256, ... in ascending order, a halving tree (128 .. 1) folds the 256 sums; thread 0
// takes the decision, writes the record and advances the step count unless the step is skipped (takes adam_advance_kernel's place).
__global__ __launch_bounds__(256) void adam_guard_kernel(const double* partials, int nparts, double* state, dct_adam_guard* guard,
                                                         float gs, int skip_nonfinite, int clip) {
  __shared__ double sm[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int k = t; k < nparts; k += 256) s += partials[k];
  sm[t] = s;
  __syncthreads();
#pragma unroll
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) sm[t] += sm[t + off];
    __syncthreads();
  }
  if (t != 0) return;
  const double sum = sm[0];
  const double norm = fabs((double)gs) * sqrt(sum);
  const bool skip = skip_nonfinite && !isfinite(sum);
  float coef = 1.f;
  if (clip && !skip) {
    const double c = guard->max_norm / (norm + 1e-6);   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
    coef = (float)(c > 1.0 ? 1.0 : c);                  // a NaN stays a NaN, as under torch's clamp
    if (!(c >= 1.0)) guard->clipped += 1;
  }
  guard->norm = norm;
  guard->coef = coef;
  guard->skip = skip ? 1u : 0u;
  if (skip) guard->skipped += 1;
  else state[0] += 1.0;
}

// adam_kernel behind a guard record that the previous launch on the stream wrote: a skipped step returns before its first load, any
// other multiplies the gradient scale by the clip coefficient (one fp32 multiply) and is adam_kernel's table path from there on.
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* p, const float* g, float* m, float* v, long long n,
                                                           float omb1, float b2, float omb2, float eps, float wd, float gs, bf16_t* shadow,
                                                           const double* state, const double* table, double beta1, double beta2,
                                                           const dct_adam_guard* guard) {
  if (guard->skip) return;
  gs *= guard->coef;
  adam_body(p, g, m, v, n, 0.f, 1.f, omb1, b2, omb2, eps, wd, gs, shadow, state, table, beta1, beta2);
}

static inline unsigned grid_for(long long P) {
  long long b = (P + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}
static inline unsigned wide_grid(long long n) {
  long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

#define DISPATCH_C(C_, ...)                                                   \
  switch (C_) {                                                               \
    case 2: { constexpr int C = 2; __VA_ARGS__; break; }                      \
    case 3: { constexpr int C = 3; __VA_ARGS__; break; }                      \
    case 4: { constexpr int C = 4; __VA_ARGS__; break; }                      \
    case 5: { constexpr int C = 5; __VA_ARGS__; break; }                      \
    case 6: { constexpr int C = 6; __VA_ARGS__; break; }                      \
    case 7: { constexpr int C = 7; __VA_ARGS__; break; }                      \
    case 8: { constexpr int C = 8; __VA_ARGS__; break; }                      \
    default: return DCT_ERR_UNSUPPORTED;                                      \
  }

extern "C" size_t dct_loss_workspace_bytes(int64_t) { return (size_t)kMaxBlocks * 2 * sizeof(float); }

static inline bool ws_ok(void* ws, size_t bytes) { return ws && bytes >= (size_t)kMaxBlocks * 2 * sizeof(float); }

// gamma of the focal loss: finite and >= 0 (a NaN fails the comparison)
static inline bool gamma_ok(float gamma) { return gamma >= 0.f && gamma <= 3.402823466e38f; }

// ---- plain, class-weighted and focal cross entropy: the 13 entry points on five launchers over the rule ---------------------------------
// What every call takes.  The plain family passes no weight and gamma = 0, the weighted one gamma = 0; reduction: 0 mean, 1 sum.
// The status of a bad call: BAD_ARG, then (rules with kChecksC) UNSUPPORTED, then WORKSPACE; any other C is UNSUPPORTED at dispatch.
struct PxArgs { const float* logits; const long long* tgt; long long P; int C, ignore; const float* weight; float gamma; hipStream_t st; };
static inline PxArgs px_args(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                             float gamma, dct_stream stream) {
  return PxArgs{logits, (const long long*)targets, (long long)pixels, C_, ignore_index, weight, gamma, (hipStream_t)stream};
}
static inline bool px_ok(const PxArgs& a) { return a.logits && a.tgt && a.P >= 1 && gamma_ok(a.gamma); }
static inline bool reduction_ok(int reduction) { return reduction == 0 || reduction == 1; }

template <template <int> class Rule>
static int loss_fwd(const PxArgs& a, int reduction, float* out2, void* workspace, size_t workspace_bytes) {
  if (!px_ok(a) || !out2 || !reduction_ok(reduction)) return DCT_ERR_BAD_ARG;
  if (Rule<2>::kChecksC && (a.C < 2 || a.C > 8)) return DCT_ERR_UNSUPPORTED;
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  const unsigned grid = grid_for(a.P);
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (loss_fwd_kernel<C, Rule>), dim3(grid), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, a.gamma, (float*)workspace));
  DCT_LAUNCH(DCT_PROF_LOSS, finalize_kernel, dim3(1), dim3(256), 0, a.st, (const float*)workspace, (int)grid, out2, reduction == 0 ? 1 : 0, 1.f, 1);
  return dct_check_launch();
}
// denom: required under the mean, not read under the sum
template <template <int> class Rule>
static int loss_bwd(const PxArgs& a, int reduction, const float* denom, const float* gscale, float gmul, float* dlogits, int accumulate) {
  if (!px_ok(a) || !dlogits || !reduction_ok(reduction) || (reduction == 0 && !denom)) return DCT_ERR_BAD_ARG;
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (loss_bwd_kernel<C, Rule>), dim3(wide_grid(a.P)), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, a.gamma,
                             reduction == 0 ? denom : (const float*)nullptr, gscale, gmul, dlogits, accumulate));
  return dct_check_launch();
}
template <template <int> class Rule>
static int loss_step(const PxArgs& a, int reduction, float* out2, const float* gscale, float gmul, float* dlogits, int accumulate, void* workspace,
                     size_t workspace_bytes) {
  if (!px_ok(a) || !out2 || !dlogits || !reduction_ok(reduction)) return DCT_ERR_BAD_ARG;
  if (Rule<2>::kChecksC && (a.C < 2 || a.C > 8)) return DCT_ERR_UNSUPPORTED;
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  const unsigned grid = grid_for(a.P);       // loss_fwd's grid: the same block partials
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (loss_fwd_kernel<C, Rule>), dim3(grid), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, a.gamma, (float*)workspace));
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (loss_bwd_fin_kernel<C, Rule>), dim3(wide_grid(a.P)), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, a.gamma,
                             reduction == 0 ? 1 : 0, (const float*)workspace, (int)grid, out2, gscale, gmul, dlogits, accumulate));
  return dct_check_launch();
}
template <template <int> class Rule>
static int loss_map_fwd(const PxArgs& a, float* map) {
  if (!px_ok(a) || !map) return DCT_ERR_BAD_ARG;
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (loss_map_fwd_kernel<C, Rule>), dim3(wide_grid(a.P)), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, a.gamma, map));
  return dct_check_launch();
}
template <template <int> class Rule>
static int loss_map_bwd(const PxArgs& a, const float* dmap, float gmul, float* dlogits, int accumulate) {
  if (!px_ok(a) || !dmap || !dlogits) return DCT_ERR_BAD_ARG;
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (loss_map_bwd_kernel<C, Rule>), dim3(wide_grid(a.P)), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, a.gamma, dmap, gmul,
                             dlogits, accumulate));
  return dct_check_launch();
}

extern "C" int dct_ce_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index,
                          float* out2, void* workspace, size_t workspace_bytes, dct_stream stream) {
  return loss_fwd<PlainRule>(px_args(logits, targets, pixels, C_, ignore_index, nullptr, 0.f, stream), 0, out2, workspace, workspace_bytes);
}
extern "C" int dct_ce_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index,
                          const float* count, const float* gscale, float gmul, float* dlogits, int accumulate,
                          dct_stream stream) {
  return loss_bwd<PlainRule>(px_args(logits, targets, pixels, C_, ignore_index, nullptr, 0.f, stream), 0, count, gscale, gmul, dlogits, accumulate);
}
extern "C" int dct_ce_step(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, float* out2,
                           const float* gscale, float gmul, float* dlogits, int accumulate, void* workspace, size_t workspace_bytes,
                           dct_stream stream) {
  return loss_step<PlainRule>(px_args(logits, targets, pixels, C_, ignore_index, nullptr, 0.f, stream), 0, out2, gscale, gmul, dlogits, accumulate,
                              workspace, workspace_bytes);
}
extern "C" int dct_ce_weighted_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                                   int reduction, float* out2, void* workspace, size_t workspace_bytes, dct_stream stream) {
  return loss_fwd<WeightedRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream), reduction, out2, workspace, workspace_bytes);
}
extern "C" int dct_ce_weighted_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                                   int reduction, const float* denom, const float* gscale, float gmul, float* dlogits, int accumulate,
                                   dct_stream stream) {
  return loss_bwd<WeightedRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream), reduction, denom, gscale, gmul, dlogits,
                                accumulate);
}
extern "C" int dct_ce_weighted_step(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                                    int reduction, float* out2, const float* gscale, float gmul, float* dlogits, int accumulate,
                                    void* workspace, size_t workspace_bytes, dct_stream stream) {
  return loss_step<WeightedRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream), reduction, out2, gscale, gmul, dlogits,
                                 accumulate, workspace, workspace_bytes);
}
extern "C" int dct_ce_map_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                              float* map, dct_stream stream) {
  return loss_map_fwd<WeightedRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream), map);
}
extern "C" int dct_ce_map_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                              const float* dmap, float gmul, float* dlogits, int accumulate, dct_stream stream) {
  return loss_map_bwd<WeightedRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream), dmap, gmul, dlogits, accumulate);
}
extern "C" int dct_focal_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                             float gamma, int reduction, float* out2, void* workspace, size_t workspace_bytes, dct_stream stream) {
  return loss_fwd<FocalRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, gamma, stream), reduction, out2, workspace, workspace_bytes);
}
extern "C" int dct_focal_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                             float gamma, int reduction, const float* denom, const float* gscale, float gmul, float* dlogits, int accumulate,
                             dct_stream stream) {
  return loss_bwd<FocalRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, gamma, stream), reduction, denom, gscale, gmul, dlogits,
                             accumulate);
}
extern "C" int dct_focal_step(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                              float gamma, int reduction, float* out2, const float* gscale, float gmul, float* dlogits, int accumulate,
                              void* workspace, size_t workspace_bytes, dct_stream stream) {
  return loss_step<FocalRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, gamma, stream), reduction, out2, gscale, gmul, dlogits,
                              accumulate, workspace, workspace_bytes);
}
extern "C" int dct_focal_map_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                                 float gamma, float* map, dct_stream stream) {
  return loss_map_fwd<FocalRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, gamma, stream), map);
}
extern "C" int dct_focal_map_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                                 float gamma, const float* dmap, float gmul, float* dlogits, int accumulate, dct_stream stream) {
  return loss_map_bwd<FocalRule>(px_args(logits, targets, pixels, C_, ignore_index, weight, gamma, stream), dmap, gmul, dlogits, accumulate);
}
// ---- top-k cross entropy: the weighted rule's map, three histogram launches of the radix select, the sum above tau ----------------------
extern "C" size_t dct_topk_ce_workspace_bytes(int64_t) { return kTopkWsBytes; }

static inline bool k_percent_ok(double k) { return k > 0.0 && k <= 100.0; }      // (a NaN fails both comparisons)
struct TopkWs { unsigned *h1, *h2, *h3, *sel; float* partial; };
static inline TopkWs topk_ws(void* workspace) {
  unsigned* w = (unsigned*)workspace;
  return TopkWs{w, w + kTopkBins1, w + kTopkBins1 + kTopkBins2, w + kTopkHistWords, (float*)(w + kTopkHistWords + kTopkSelWords)};
}
// BAD_ARG, then UNSUPPORTED, then WORKSPACE
static int topk_check(const PxArgs& a, double k_percent, const float* out2, const int64_t* counts4, const float* vmap, void* workspace,
                      size_t workspace_bytes) {
  if (!px_ok(a) || !out2 || !counts4 || !vmap || !k_percent_ok(k_percent)) return DCT_ERR_BAD_ARG;
  if (a.C < 2 || a.C > 8 || a.P > 2147483647LL) return DCT_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < kTopkWsBytes) return DCT_ERR_WORKSPACE;
  return DCT_OK;
}
// the memset of the histograms and launches 1 to 4: vmap, counts4, out2[1] and the partials of the sum above tau; -> the partials' count
static int topk_select(const PxArgs& a, double k_percent, float* out2, int64_t* counts4, float* vmap, const TopkWs& ws, unsigned& grid) {
  grid = grid_for(a.P);
  if (hipMemsetAsync(ws.h1, 0, (size_t)kTopkHistWords * 4, a.st) != hipSuccess) return DCT_ERR_LAUNCH;
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (topk_map_hist_kernel<C>), dim3(grid), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, vmap, ws.h1));
  DCT_LAUNCH(DCT_PROF_LOSS, topk_hist2_kernel, dim3(grid), dim3(256), 0, a.st, (const float*)vmap, a.tgt, a.P, a.ignore, a.C, k_percent,
             (const unsigned*)ws.h1, ws.h2, ws.sel);
  DCT_LAUNCH(DCT_PROF_LOSS, topk_hist3_kernel, dim3(grid), dim3(256), 0, a.st, (const float*)vmap, a.tgt, a.P, a.ignore, a.C, (const unsigned*)ws.h2,
             ws.h3, ws.sel);
  DCT_LAUNCH(DCT_PROF_LOSS, topk_sum_kernel, dim3(grid), dim3(256), 0, a.st, (const float*)vmap, a.P, (const unsigned*)ws.h3, (const unsigned*)ws.sel,
             ws.partial, out2, (long long*)counts4);
  return DCT_OK;
}
extern "C" int dct_topk_ce_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                               double k_percent, float* out2, int64_t* counts4, float* vmap, void* workspace, size_t workspace_bytes,
                               dct_stream stream) {
  const PxArgs a = px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream);
  if (const int rc = topk_check(a, k_percent, out2, counts4, vmap, workspace, workspace_bytes)) return rc;
  const TopkWs ws = topk_ws(workspace);
  unsigned grid;
  if (const int rc = topk_select(a, k_percent, out2, counts4, vmap, ws, grid)) return rc;
  DCT_LAUNCH(DCT_PROF_LOSS, topk_fin_kernel, dim3(1), dim3(256), 0, a.st, (const float*)ws.partial, (int)grid, out2, (const long long*)counts4);
  return dct_check_launch();
}
extern "C" int dct_topk_ce_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                               const float* vmap, const float* out2, const int64_t* counts4, const float* gscale, float gmul, float* dlogits,
                               int accumulate, dct_stream stream) {
  const PxArgs a = px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream);
  if (!px_ok(a) || !out2 || !counts4 || !vmap || !dlogits) return DCT_ERR_BAD_ARG;
  if (a.C < 2 || a.C > 8 || a.P > 2147483647LL) return DCT_ERR_UNSUPPORTED;
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (topk_bwd_kernel<C>), dim3(wide_grid(a.P)), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight, vmap, out2,
                             (const long long*)counts4, (const float*)nullptr, 0, (float*)nullptr, gscale, gmul, dlogits, accumulate));
  return dct_check_launch();
}
extern "C" int dct_topk_ce_step(const float* logits, const int64_t* targets, int64_t pixels, int C_, int ignore_index, const float* weight,
                                double k_percent, float* out2, int64_t* counts4, float* vmap, const float* gscale, float gmul, float* dlogits,
                                int accumulate, void* workspace, size_t workspace_bytes, dct_stream stream) {
  const PxArgs a = px_args(logits, targets, pixels, C_, ignore_index, weight, 0.f, stream);
  if (!dlogits) return DCT_ERR_BAD_ARG;
  if (const int rc = topk_check(a, k_percent, out2, counts4, vmap, workspace, workspace_bytes)) return rc;
  const TopkWs ws = topk_ws(workspace);
  unsigned grid;
  if (const int rc = topk_select(a, k_percent, out2, counts4, vmap, ws, grid)) return rc;
  DISPATCH_C(a.C, DCT_LAUNCH(DCT_PROF_LOSS, (topk_bwd_kernel<C>), dim3(wide_grid(a.P)), dim3(256), 0, a.st, a.logits, a.tgt, a.P, a.ignore, a.weight,
                             (const float*)vmap, (const float*)out2, (const long long*)counts4, (const float*)ws.partial, (int)grid, out2, gscale, gmul,
                             dlogits, accumulate));
  return dct_check_launch();
}
// K of a boundary mask (the number of its bits below C), or a status
static inline int boundary_k(int64_t pixels, int C_, int class_mask, float& K) {
  if (pixels < 1) return DCT_ERR_BAD_ARG;
  if (C_ < 2 || C_ > 8) return DCT_ERR_UNSUPPORTED;
  const int k = __builtin_popcount((unsigned)class_mask & ((1u << C_) - 1u));
  if (k == 0) return DCT_ERR_BAD_ARG;
  K = (float)k;
  return DCT_OK;
}
extern "C" int dct_boundary_fwd(const float* logits, const int64_t* targets, const float* phi, int64_t pixels, int C_, int ignore_index,
                                int class_mask, float* out2, void* workspace, size_t workspace_bytes, dct_stream stream) {
  if (!logits || !targets || !phi || !out2 || !workspace) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)logits | (uintptr_t)phi) & 15) return DCT_ERR_BAD_ARG;
  float K;
  const int status = boundary_k(pixels, C_, class_mask, K);
  if (status != DCT_OK) return status;
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(pixels);
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, bd_fwd_kernel<C>, dim3(grid), dim3(256), 0, st, logits, (const long long*)targets, phi, (long long)pixels, ignore_index, class_mask,
                            (float*)workspace));
  DCT_LAUNCH(DCT_PROF_LOSS, bd_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (int)grid, out2, K);
  return dct_check_launch();
}
extern "C" int dct_boundary_bwd(const float* logits, const int64_t* targets, const float* phi, int64_t pixels, int C_, int ignore_index,
                                int class_mask, const float* count, const float* gscale, float gmul, float* dlogits, int accumulate,
                                dct_stream stream) {
  if (!logits || !targets || !phi || !count || !dlogits) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)logits | (uintptr_t)phi | (uintptr_t)dlogits) & 15) return DCT_ERR_BAD_ARG;
  float K;
  const int status = boundary_k(pixels, C_, class_mask, K);
  if (status != DCT_OK) return status;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, bd_bwd_kernel<C>, dim3(wide_grid(pixels)), dim3(256), 0, st, logits, (const long long*)targets, phi, (long long)pixels, ignore_index,
                            class_mask, K, count, gscale, gmul, dlogits, accumulate));
  return dct_check_launch();
}
// blocks along x of one image: at most cap / B (at least one), so that B of them stay within cap rows (B rows when B > cap)
static inline unsigned dice_grid_x(long long ppi, int B, int cap) {
  long long b = (ppi + 255) / 256;
  const long long c = cap / B < 1 ? 1 : cap / B;
  return (unsigned)(b < c ? b : c);
}
static inline size_t dice_ws_bytes(int B, int C_) {
  return (size_t)(B > kDiceFwdBlocks ? B : kDiceFwdBlocks) * (size_t)(3 * C_ + 2) * sizeof(float);
}
// what the three calls of both families take beside their outputs: the tensors and sizes, the common block as the kernels take it and the
// status of the rule's check
struct OverlapCall { const float* logits; const long long* targets; int B; long long ppi; int C_, ignore; const float* weight; hipStream_t st; OverlapArgs r; int status; };
// The rule check, from an entry point's arguments: the checks the three calls share (pointers apart) and, with tv, the Tversky parameters'
// own and their rule (Dice has none): 1 - alpha - beta and 1 / gamma are formed in double and rounded once each.
static OverlapCall overlap_call(const float* logits, const int64_t* targets, int B, int64_t ppi, int C_, int ignore_index, const float* weight,
                                int class_mask, float smooth, int per_image, float ce_coef, float coef, dct_stream stream, float alpha = .5f,
                                float beta = .5f, float gamma = 1.f, TverskyTerms* tv = nullptr) {
  OverlapCall c{logits, (const long long*)targets, B, (long long)ppi, C_, ignore_index, weight, (hipStream_t)stream, OverlapArgs{}, DCT_ERR_BAD_ARG};
  if (B < 1 || ppi < 1 || !(smooth >= 0.f) || __builtin_isinf(smooth) || (per_image != 0 && per_image != 1)) return c;
  if (C_ < 2 || C_ > 8 || B > 65535) { c.status = DCT_ERR_UNSUPPORTED; return c; }
  const int mask = class_mask & ((1 << C_) - 1);
  if (!mask) return c;
  if (!(alpha >= 0.f) || !(beta >= 0.f) || __builtin_isinf(alpha) || __builtin_isinf(beta) || alpha + beta == 0.f) return c;
  if (!(gamma > 0.f) || __builtin_isinf(gamma)) return c;
  const int G = per_image ? B : 1, K = __builtin_popcount((unsigned)mask);
  c.r = OverlapArgs{mask, per_image, smooth, ce_coef, coef, 1.f / (float)((long long)G * K)};
  if (tv) *tv = TverskyTerms{alpha, beta, (float)(1.0 - (double)alpha - (double)beta), (float)(1.0 / (double)gamma), gamma != 1.f};
  c.status = DCT_OK;
  return c;
}
// The status of a bad call: BAD_ARG (the pointers, then the rule's check), UNSUPPORTED (C, B), then WORKSPACE
#define OVERLAP_LAUNCH(kernel, blocks, ...)                                                                                                 \
  DISPATCH_C(c.C_, DCT_LAUNCH(DCT_PROF_LOSS, kernel, dim3(dice_grid_x(c.ppi, c.B, blocks), (unsigned)c.B), dim3(256), 0, c.st, c.logits, c.targets, \
                              c.ppi, c.ignore, c.weight, __VA_ARGS__))
template <class Rule>
static int overlap_fwd(const Rule& rule, const OverlapCall& c, float* out4, float* index_gc, float* sums, void* workspace, size_t workspace_bytes) {
  if (!c.logits || !c.targets || !out4 || !index_gc || !sums) return DCT_ERR_BAD_ARG;
  if (c.status != DCT_OK) return c.status;
  if (!workspace || workspace_bytes < dice_ws_bytes(c.B, c.C_)) return DCT_ERR_WORKSPACE;
  const int fbx = (int)dice_grid_x(c.ppi, c.B, kDiceFwdBlocks);
  OVERLAP_LAUNCH(overlap_fwd_kernel<C>, kDiceFwdBlocks, (float*)workspace);
  DISPATCH_C(c.C_, DCT_LAUNCH(DCT_PROF_LOSS, (overlap_fin_kernel<C, Rule>), dim3(1), dim3(256), 0, c.st, (const float*)workspace, c.B, fbx, c.r, rule,
                              out4, index_gc, sums));
  return dct_check_launch();
}
template <class Rule>
static int overlap_bwd(const Rule& rule, const OverlapCall& c, const float* out4, const float* sums, const float* gscale, float gmul, float* dlogits,
                       int accumulate) {
  if (!c.logits || !c.targets || !out4 || !sums || !dlogits) return DCT_ERR_BAD_ARG;
  if (c.status != DCT_OK) return c.status;
  OVERLAP_LAUNCH((overlap_bwd_kernel<C, Rule>), kDiceBwdBlocks, c.r, rule, out4, sums, gscale, gmul, dlogits, accumulate);
  return dct_check_launch();
}
// overlap_fwd's forward launch (the same partial rows) and overlap_bwd's grid
template <class Rule>
static int overlap_step(const Rule& rule, const OverlapCall& c, float* out4, float* index_gc, float* sums, const float* gscale, float gmul,
                        float* dlogits, int accumulate, void* workspace, size_t workspace_bytes) {
  if (!c.logits || !c.targets || !out4 || !index_gc || !sums || !dlogits) return DCT_ERR_BAD_ARG;
  if (c.status != DCT_OK) return c.status;
  if (!workspace || workspace_bytes < dice_ws_bytes(c.B, c.C_)) return DCT_ERR_WORKSPACE;
  const int fbx = (int)dice_grid_x(c.ppi, c.B, kDiceFwdBlocks);
  OVERLAP_LAUNCH(overlap_fwd_kernel<C>, kDiceFwdBlocks, (float*)workspace);
  OVERLAP_LAUNCH((overlap_bwd_fin_kernel<C, Rule>), kDiceBwdBlocks, c.r, rule, (const float*)workspace, fbx, out4, index_gc, sums, gscale, gmul,
                 dlogits, accumulate);
  return dct_check_launch();
}
#undef OVERLAP_LAUNCH

extern "C" size_t dct_ce_dice_workspace_bytes(int B, int C_, int /*per_image*/) {
  return dice_ws_bytes(B < 1 ? 1 : B, C_ < 2 ? 2 : (C_ > 8 ? 8 : C_));
}
extern "C" int dct_ce_dice_fwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C_, int ignore_index,
                               const float* weight, int class_mask, float smooth, int per_image, float ce_coef, float dice_coef, float* out4,
                               float* dice_gc, float* sums, void* workspace, size_t workspace_bytes, dct_stream stream) {
  const OverlapCall c = overlap_call(logits, targets, B, pixels_per_image, C_, ignore_index, weight, class_mask, smooth, per_image, ce_coef, dice_coef, stream);
  return overlap_fwd(DiceTerms{}, c, out4, dice_gc, sums, workspace, workspace_bytes);
}
extern "C" int dct_ce_dice_bwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C_, int ignore_index,
                               const float* weight, int class_mask, float smooth, int per_image, float ce_coef, float dice_coef,
                               const float* out4, const float* sums, const float* gscale, float gmul, float* dlogits, int accumulate,
                               dct_stream stream) {
  const OverlapCall c = overlap_call(logits, targets, B, pixels_per_image, C_, ignore_index, weight, class_mask, smooth, per_image, ce_coef, dice_coef, stream);
  return overlap_bwd(DiceTerms{}, c, out4, sums, gscale, gmul, dlogits, accumulate);
}
extern "C" int dct_ce_dice_step(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C_, int ignore_index,
                                const float* weight, int class_mask, float smooth, int per_image, float ce_coef, float dice_coef, float* out4,
                                float* dice_gc, float* sums, const float* gscale, float gmul, float* dlogits, int accumulate,
                                void* workspace, size_t workspace_bytes, dct_stream stream) {
  const OverlapCall c = overlap_call(logits, targets, B, pixels_per_image, C_, ignore_index, weight, class_mask, smooth, per_image, ce_coef, dice_coef, stream);
  return overlap_step(DiceTerms{}, c, out4, dice_gc, sums, gscale, gmul, dlogits, accumulate, workspace, workspace_bytes);
}
extern "C" size_t dct_ce_tversky_workspace_bytes(int B, int C_, int per_image) { return dct_ce_dice_workspace_bytes(B, C_, per_image); }
extern "C" int dct_ce_tversky_fwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C_, int ignore_index,
                                  const float* weight, int class_mask, float smooth, float alpha, float beta, float gamma, int per_image,
                                  float ce_coef, float tversky_coef, float* out4, float* tversky_gc, float* sums, void* workspace,
                                  size_t workspace_bytes, dct_stream stream) {
  TverskyTerms tv;
  const OverlapCall c = overlap_call(logits, targets, B, pixels_per_image, C_, ignore_index, weight, class_mask, smooth, per_image, ce_coef, tversky_coef,
                                     stream, alpha, beta, gamma, &tv);
  return overlap_fwd(tv, c, out4, tversky_gc, sums, workspace, workspace_bytes);
}
extern "C" int dct_ce_tversky_bwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C_, int ignore_index,
                                  const float* weight, int class_mask, float smooth, float alpha, float beta, float gamma, int per_image,
                                  float ce_coef, float tversky_coef, const float* out4, const float* sums, const float* gscale, float gmul,
                                  float* dlogits, int accumulate, dct_stream stream) {
  TverskyTerms tv;
  const OverlapCall c = overlap_call(logits, targets, B, pixels_per_image, C_, ignore_index, weight, class_mask, smooth, per_image, ce_coef, tversky_coef,
                                     stream, alpha, beta, gamma, &tv);
  return overlap_bwd(tv, c, out4, sums, gscale, gmul, dlogits, accumulate);
}
extern "C" int dct_ce_tversky_step(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C_, int ignore_index,
                                   const float* weight, int class_mask, float smooth, float alpha, float beta, float gamma, int per_image,
                                   float ce_coef, float tversky_coef, float* out4, float* tversky_gc, float* sums, const float* gscale,
                                   float gmul, float* dlogits, int accumulate, void* workspace, size_t workspace_bytes, dct_stream stream) {
  TverskyTerms tv;
  const OverlapCall c = overlap_call(logits, targets, B, pixels_per_image, C_, ignore_index, weight, class_mask, smooth, per_image, ce_coef, tversky_coef,
                                     stream, alpha, beta, gamma, &tv);
  return overlap_step(tv, c, out4, tversky_gc, sums, gscale, gmul, dlogits, accumulate, workspace, workspace_bytes);
}
extern "C" int dct_softmax_fwd(const float* logits, float* probs, int64_t pixels, int C_, dct_stream stream) {
  if (!logits || !probs || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, softmax_fwd_kernel<C>, dim3(wide_grid(pixels)), dim3(256), 0, st, logits, probs, (long long)pixels));
  return dct_check_launch();
}
extern "C" int dct_softmax_bwd(const float* probs, const float* dprobs, float* dlogits, int64_t pixels, int C_,
                               int accumulate, dct_stream stream) {
  if (!probs || !dprobs || !dlogits || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, softmax_bwd_kernel<C>, dim3(wide_grid(pixels)), dim3(256), 0, st, probs, dprobs, dlogits, (long long)pixels, accumulate));
  return dct_check_launch();
}
extern "C" int dct_entropy_fwd(const float* probs, float* map, int64_t pixels, int C_, dct_stream stream) {
  if (!probs || !map || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, entropy_fwd_kernel<C>, dim3(wide_grid(pixels)), dim3(256), 0, st, probs, map, (long long)pixels));
  return dct_check_launch();
}

extern "C" int dct_entropy_bwd(const float* probs, const float* dmap, float* dprobs, int64_t pixels, int C_, dct_stream stream) {
  if (!probs || !dmap || !dprobs || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, entropy_bwd_kernel<C>, dim3(wide_grid(pixels)), dim3(256), 0, st, probs, dmap, dprobs, (long long)pixels));
  return dct_check_launch();
}

static bool fill_pack(PtrPack& pk, const float* const* in, float* const* out, int S) {
  if (S < 1 || S > MAXS || !in) return false;
  for (int s = 0; s < MAXS; ++s) { pk.in[s] = nullptr; pk.out[s] = nullptr; }
  for (int s = 0; s < S; ++s) {
    if (!in[s]) return false;
    pk.in[s] = in[s];
    if (out) { if (!out[s]) return false; pk.out[s] = out[s]; }
  }
  return true;
}

extern "C" int dct_jsd_map_fwd(const float* const* probs, int S, float* map, int64_t pixels, int C_, dct_stream stream) {
  PtrPack pk;
  if (!fill_pack(pk, probs, nullptr, S) || !map || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_fwd_kernel<C, false>), dim3(wide_grid(pixels)), dim3(256), 0, st, pk, S, (long long)pixels, map, (float*)nullptr));
  return dct_check_launch();
}
extern "C" int dct_jsd_map_bwd(const float* const* probs, int S, const float* dmap, float* const* dprobs,
                               int64_t pixels, int C_, dct_stream stream) {
  PtrPack pk;
  if (!fill_pack(pk, probs, dprobs, S) || !dmap || !dprobs || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (S <= 4) { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_bwd_kernel<C, false, 4>), dim3(wide_grid(pixels)), dim3(256), 0, st, pk, S, (long long)pixels, dmap, (const float*)nullptr, 1.f, 0)); }
  else { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_bwd_kernel<C, false, MAXS>), dim3(wide_grid(pixels)), dim3(256), 0, st, pk, S, (long long)pixels, dmap, (const float*)nullptr, 1.f, 0)); }
  return dct_check_launch();
}
extern "C" int dct_jsd_logits_fwd(const float* const* logits, int S, int64_t pixels, int C_, float* out1,
                                  void* workspace, size_t workspace_bytes, dct_stream stream) {
  PtrPack pk;
  if (!fill_pack(pk, logits, nullptr, S) || !out1 || pixels < 1) return DCT_ERR_BAD_ARG;
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(pixels);
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_fwd_kernel<C, true>), dim3(grid), dim3(256), 0, st, pk, S, (long long)pixels, (float*)nullptr, (float*)workspace));
  DCT_LAUNCH(DCT_PROF_LOSS, finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (int)grid, out1, 0, (float)pixels, 0);
  return dct_check_launch();
}
extern "C" int dct_jsd_logits_bwd(const float* const* logits, int S, int64_t pixels, int C_, const float* gscale,
                                  float gmul, float* const* dlogits, int accumulate, dct_stream stream) {
  PtrPack pk;
  if (!fill_pack(pk, logits, dlogits, S) || !dlogits || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (S <= 4) { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_bwd_kernel<C, true, 4>), dim3(wide_grid(pixels)), dim3(256), 0, st, pk, S, (long long)pixels, (const float*)nullptr, gscale, gmul, accumulate)); }
  else { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_bwd_kernel<C, true, MAXS>), dim3(wide_grid(pixels)), dim3(256), 0, st, pk, S, (long long)pixels, (const float*)nullptr, gscale, gmul, accumulate)); }
  return dct_check_launch();
}

extern "C" int dct_jsd_logits_step(const float* const* logits, int S, int64_t pixels, int C_, float* out1, float* const* probs,
                                   const float* gscale, float gmul, float* const* dlogits, int accumulate,
                                   void* workspace, size_t workspace_bytes, dct_stream stream) {
  PtrPack pk, pp;
  if (!fill_pack(pk, logits, dlogits, S) || !out1 || pixels < 1) return DCT_ERR_BAD_ARG;
  for (int s = 0; s < MAXS; ++s) { pp.in[s] = nullptr; pp.out[s] = (probs && s < S) ? probs[s] : nullptr; }
  if (!dlogits) { for (int s = 0; s < MAXS; ++s) pk.out[s] = nullptr; }
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(pixels);       // dct_jsd_logits_fwd's grid: the block partials, hence the mean, come out bit for bit
  const int want = dlogits ? 1 : 0;
  if (S <= 2) { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_step_kernel<C, 2>), dim3(grid), dim3(256), 0, st, pk, pp, S, (long long)pixels, gscale, gmul, accumulate, want, (float*)workspace)); }
  else if (S <= 4) { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_step_kernel<C, 4>), dim3(grid), dim3(256), 0, st, pk, pp, S, (long long)pixels, gscale, gmul, accumulate, want, (float*)workspace)); }
  else { DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (jsd_step_kernel<C, MAXS>), dim3(grid), dim3(256), 0, st, pk, pp, S, (long long)pixels, gscale, gmul, accumulate, want, (float*)workspace)); }
  DCT_LAUNCH(DCT_PROF_LOSS, finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (int)grid, out1, 0, (float)pixels, 0);
  return dct_check_launch();
}

// ---- view consistency: the nine entry points on three launchers over the rule ---------------------------------------------------------
namespace {
// What every rule checks, and the host-side constants: 1 / S as the ensemble confidence scales by it, the teacher terms of a pixel and
// the ordered pairs (cross) or views (ensemble) that the weight divides by
bool cons_rule(int S, int teacher, float tau, int64_t pixels, ConsArgs& a, int& terms) {
  if (teacher != DCT_PL_CROSS && teacher != DCT_PL_ENSEMBLE) return false;
  if (S < (teacher == DCT_PL_CROSS ? 2 : 1) || S > MAXS) return false;
  if (!(tau >= 0.f) || pixels < 1) return false;             // (a NaN fails the first)
  a = ConsArgs{S, teacher, tau, 1.f / (float)S, 0.f, teacher == DCT_PL_CROSS ? (float)S : 1.f, (long long)pixels};
  terms = teacher == DCT_PL_CROSS ? S * (S - 1) : S;
  return true;
}
// w = 1 / (S (S - 1)) resp. 1 / S, under kPerClass 1 / (C S (S - 1)) resp. 1 / (C S): formed where C is known to be in 2..8
template <class Rule, int C>
inline ConsArgs cons_weighted(ConsArgs a, int terms) {
  a.wgt = 1.f / (float)((Rule::kPerClass ? C : 1) * terms);
  return a;
}
// the rules' own checks (a NaN fails each first comparison); the temperature: finite and > 0, and so is r = 1.f / T formed in fp32 (a
// subnormal T gives inf)
inline bool eps_ok(float eps) { return eps > 0.f; }
bool soft_rule(float temperature, float eps, SoftRule& rule) {
  rule = SoftRule{eps, 1.f / temperature};
  return eps_ok(eps) && temperature > 0.f && __builtin_isfinite(temperature) && rule.r > 0.f && __builtin_isfinite(rule.r);
}
}  // namespace

// The SMAX instantiation of `kernel` for C_, with the rule, the weighted arguments and what follows
#define CONS_LAUNCH(kernel, SMAX_, grid, ...)                                                                                          \
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (kernel<C, SMAX_, Rule>), dim3(grid), dim3(256), 0, st, rule, cons_weighted<Rule, C>(a, terms), __VA_ARGS__))

// The status of a bad call: BAD_ARG (the rule's check first), then UNSUPPORTED at dispatch; the step: BAD_ARG, WORKSPACE, UNSUPPORTED.
template <class Rule>
static int cons_map_fwd(const Rule& rule, bool rule_ok, const float* const* probs, int S, int teacher, float tau, float* map, float* kept,
                        int64_t pixels, int C_, dct_stream stream) {
  PtrPack pk;
  ConsArgs a;
  int terms;
  if (!rule_ok || !cons_rule(S, teacher, tau, pixels, a, terms) || !fill_pack(pk, probs, nullptr, S) || !map) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = wide_grid(pixels);
  if (S <= 4) { CONS_LAUNCH(cons_map_fwd_kernel, 4, grid, pk, map, kept); }
  else { CONS_LAUNCH(cons_map_fwd_kernel, MAXS, grid, pk, map, kept); }
  return dct_check_launch();
}
template <class Rule>
static int cons_map_bwd(const Rule& rule, bool rule_ok, const float* const* probs, int S, int teacher, float tau, const float* dmap,
                        float* const* dprobs, int64_t pixels, int C_, dct_stream stream) {
  PtrPack pk;
  ConsArgs a;
  int terms;
  if (!rule_ok || !cons_rule(S, teacher, tau, pixels, a, terms) || !dprobs || !fill_pack(pk, probs, dprobs, S) || !dmap) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = wide_grid(pixels);
  if (S <= 4) { CONS_LAUNCH(cons_map_bwd_kernel, 4, grid, pk, dmap); }
  else { CONS_LAUNCH(cons_map_bwd_kernel, MAXS, grid, pk, dmap); }
  return dct_check_launch();
}
template <class Rule>
static int cons_step(const Rule& rule, bool rule_ok, const float* const* logits, int S, int teacher, float tau, int64_t pixels, int C_, float* out2,
                     float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate, void* workspace,
                     size_t workspace_bytes, dct_stream stream) {
  PtrPack pk, pp;
  ConsArgs a;
  int terms;
  if (!rule_ok || !cons_rule(S, teacher, tau, pixels, a, terms) || !fill_pack(pk, logits, dlogits, S) || !out2) return DCT_ERR_BAD_ARG;
  for (int s = 0; s < MAXS; ++s) { pp.in[s] = nullptr; pp.out[s] = (probs && s < S) ? probs[s] : nullptr; }
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(pixels);       // dct_jsd_logits_step's grid
  const int want = dlogits ? 1 : 0;
  if (S <= 2) { CONS_LAUNCH(cons_step_kernel, 2, grid, pk, pp, gscale, gmul, accumulate, want, (float*)workspace); }
  else if (S <= 4) { CONS_LAUNCH(cons_step_kernel, 4, grid, pk, pp, gscale, gmul, accumulate, want, (float*)workspace); }
  else { CONS_LAUNCH(cons_step_kernel, MAXS, grid, pk, pp, gscale, gmul, accumulate, want, (float*)workspace); }
  DCT_LAUNCH(DCT_PROF_LOSS, pl_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (int)grid, out2, (float)pixels, (float)pixels * a.kden);
  return dct_check_launch();
}
#undef CONS_LAUNCH

extern "C" int dct_pl_map_fwd(const float* const* probs, int S, int teacher, float tau, float eps, float* map, float* kept,
                              int64_t pixels, int C_, dct_stream stream) {
  return cons_map_fwd(HardRule{eps}, eps_ok(eps), probs, S, teacher, tau, map, kept, pixels, C_, stream);
}
extern "C" int dct_pl_map_bwd(const float* const* probs, int S, int teacher, float tau, float eps, const float* dmap, float* const* dprobs,
                              int64_t pixels, int C_, dct_stream stream) {
  return cons_map_bwd(HardRule{eps}, eps_ok(eps), probs, S, teacher, tau, dmap, dprobs, pixels, C_, stream);
}
extern "C" int dct_pl_logits_step(const float* const* logits, int S, int teacher, float tau, float eps, int64_t pixels, int C_, float* out2,
                                  float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate,
                                  void* workspace, size_t workspace_bytes, dct_stream stream) {
  return cons_step(HardRule{eps}, eps_ok(eps), logits, S, teacher, tau, pixels, C_, out2, probs, gscale, gmul, dlogits, accumulate, workspace,
                   workspace_bytes, stream);
}
extern "C" int dct_spl_map_fwd(const float* const* probs, int S, int teacher, float tau, float temperature, float eps, float* map, float* kept,
                               int64_t pixels, int C_, dct_stream stream) {
  SoftRule rule;
  const bool ok = soft_rule(temperature, eps, rule);
  return cons_map_fwd(rule, ok, probs, S, teacher, tau, map, kept, pixels, C_, stream);
}
extern "C" int dct_spl_map_bwd(const float* const* probs, int S, int teacher, float tau, float temperature, float eps, const float* dmap,
                               float* const* dprobs, int64_t pixels, int C_, dct_stream stream) {
  SoftRule rule;
  const bool ok = soft_rule(temperature, eps, rule);
  return cons_map_bwd(rule, ok, probs, S, teacher, tau, dmap, dprobs, pixels, C_, stream);
}
extern "C" int dct_spl_logits_step(const float* const* logits, int S, int teacher, float tau, float temperature, float eps, int64_t pixels, int C_,
                                   float* out2, float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate,
                                   void* workspace, size_t workspace_bytes, dct_stream stream) {
  SoftRule rule;
  const bool ok = soft_rule(temperature, eps, rule);
  return cons_step(rule, ok, logits, S, teacher, tau, pixels, C_, out2, probs, gscale, gmul, dlogits, accumulate, workspace, workspace_bytes, stream);
}
extern "C" int dct_mse_map_fwd(const float* const* probs, int S, int teacher, float tau, float* map, float* kept, int64_t pixels, int C_,
                               dct_stream stream) {
  return cons_map_fwd(MseRule{}, true, probs, S, teacher, tau, map, kept, pixels, C_, stream);
}
extern "C" int dct_mse_map_bwd(const float* const* probs, int S, int teacher, float tau, const float* dmap, float* const* dprobs,
                               int64_t pixels, int C_, dct_stream stream) {
  return cons_map_bwd(MseRule{}, true, probs, S, teacher, tau, dmap, dprobs, pixels, C_, stream);
}
extern "C" int dct_mse_logits_step(const float* const* logits, int S, int teacher, float tau, int64_t pixels, int C_, float* out2,
                                   float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate,
                                   void* workspace, size_t workspace_bytes, dct_stream stream) {
  return cons_step(MseRule{}, true, logits, S, teacher, tau, pixels, C_, out2, probs, gscale, gmul, dlogits, accumulate, workspace,
                   workspace_bytes, stream);
}

extern "C" int dct_kl_map_fwd(const float* p, const float* y, float* map, int64_t pixels, int C_, float eps, dct_stream stream) {
  if (!p || !y || !map || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (kl_fwd_kernel<C, false>), dim3(wide_grid(pixels)), dim3(256), 0, st, p, y, (long long)pixels, eps, map, (float*)nullptr));
  return dct_check_launch();
}
extern "C" int dct_kl_map_bwd(const float* p, const float* y, const float* dmap, float* dp, int64_t pixels,
                              int C_, float eps, dct_stream stream) {
  if (!p || !y || !dmap || !dp || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (kl_bwd_kernel<C, false>), dim3(wide_grid(pixels)), dim3(256), 0, st, p, y, (long long)pixels, eps, dmap, (const float*)nullptr, 1.f, dp, 0));
  return dct_check_launch();
}
extern "C" int dct_kl_logits_fwd(const float* p_logits, const float* y_logits, int64_t pixels, int C_, float eps,
                                 float* out1, void* workspace, size_t workspace_bytes, dct_stream stream) {
  if (!p_logits || !y_logits || !out1 || pixels < 1) return DCT_ERR_BAD_ARG;
  if (!ws_ok(workspace, workspace_bytes)) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(pixels);
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (kl_fwd_kernel<C, true>), dim3(grid), dim3(256), 0, st, p_logits, y_logits, (long long)pixels, eps, (float*)nullptr, (float*)workspace));
  DCT_LAUNCH(DCT_PROF_LOSS, finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (int)grid, out1, 0, (float)pixels, 0);
  return dct_check_launch();
}
extern "C" int dct_kl_logits_bwd(const float* p_logits, const float* y_logits, int64_t pixels, int C_, float eps,
                                 const float* gscale, float gmul, float* dp_logits, int accumulate, dct_stream stream) {
  if (!p_logits || !y_logits || !dp_logits || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, (kl_bwd_kernel<C, true>), dim3(wide_grid(pixels)), dim3(256), 0, st, p_logits, y_logits, (long long)pixels, eps, (const float*)nullptr, gscale, gmul, dp_logits, accumulate));
  return dct_check_launch();
}

extern "C" int dct_argmax(const float* x, int64_t* cls, int64_t pixels, int C_, dct_stream stream) {
  if (!x || !cls || pixels < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, argmax_kernel<C>, dim3(wide_grid(pixels)), dim3(256), 0, st, x, (long long*)cls, (long long)pixels));
  return dct_check_launch();
}

extern "C" int dct_dice_counts(const float* logits, const int64_t* gt, int B, int64_t pixels_per_image, int C_,
                               int32_t* inter, int32_t* psum, int32_t* gsum, dct_stream stream) {
  if (!logits || !gt || !inter || !psum || !gsum || B < 1 || pixels_per_image < 1) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  long long bx = (pixels_per_image + 255) / 256;
  if (bx > 64) bx = 64;
  DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, dice_kernel<C>, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, st, logits, (const long long*)gt, (long long)pixels_per_image, inter, psum, gsum));
  return dct_check_launch();
}

// Dice of one DiceMeter.add from the counts, plus the meter's running moments, in ONE launch (one block): rows = B (2-D, per
// slice) or 1 (3-D, counts summed over the batch); dice[row][c] = (2 inter + smooth) / (psum + gsum + smooth) in fp32 as
// the reference's einsum formula gives it; acc[0][j] += value, acc[1][j] += value^2 (double) for the C classes and, at
// j = C, for the row's mean over the report axes (bit c of axes_mask).  Rows are folded in order by one thread per column.
__global__ __launch_bounds__(256) void dice_update_kernel(const int* inter, const int* psum, const int* gsum, int B, int C_, int rows,
                                                          unsigned axes_mask, float smooth, float* dice, double* acc) {
  __shared__ float sd[64 * 8];
  for (int i = threadIdx.x; i < rows * C_; i += 256) {
    const int r = i / C_, c = i - r * C_;
    long long a = 0, b = 0, g = 0;
    if (rows == B) { a = inter[i]; b = psum[i]; g = gsum[i]; }
    else for (int k = 0; k < B; ++k) { a += inter[k * C_ + c]; b += psum[k * C_ + c]; g += gsum[k * C_ + c]; }
    const float d = (2.f * (float)a + smooth) / ((float)(b + g) + smooth);
    dice[i] = d;
    if (r < 64) sd[r * 8 + c] = d;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j <= C_) {
    double s0 = 0.0, s1 = 0.0;
    int naxes = 0;
    for (int c = 0; c < C_; ++c) naxes += (axes_mask >> c) & 1;
    for (int r = 0; r < rows; ++r) {
      float v;
      if (j < C_) v = sd[r * 8 + j];
      else {
        float t = 0.f;
        for (int c = 0; c < C_; ++c) if ((axes_mask >> c) & 1) t += sd[r * 8 + c];
        v = t / (float)naxes;
      }
      s0 += (double)v; s1 += (double)v * (double)v;
    }
    acc[j] += s0; acc[(C_ + 1) + j] += s1;
  }
}

extern "C" int dct_dice_update(const int32_t* inter, const int32_t* psum, const int32_t* gsum, int B, int C_, int method3d,
                               uint32_t axes_mask, float smooth, float* dice, double* acc, dct_stream stream) {
  if (!inter || !psum || !gsum || !dice || !acc || B < 1 || B > 64 || C_ < 1 || C_ > 8 || !(axes_mask & ((1u << C_) - 1))) return DCT_ERR_BAD_ARG;
  DCT_LAUNCH(DCT_PROF_LOSS, dice_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, inter, psum, gsum, B, C_, method3d ? 1 : B,
             axes_mask, smooth, dice, acc);
  return dct_check_launch();
}

extern "C" int dct_fgsm_step(const float* x, const float* g, float eps, float* x_adv, float* noise, int64_t n,
                             dct_stream stream) {
  if (!x || !g || !x_adv || n < 1) return DCT_ERR_BAD_ARG;
  DCT_LAUNCH(DCT_PROF_OTHER, fgsm_kernel, dim3(wide_grid(n)), dim3(256), 0, (hipStream_t)stream, x, g, eps, x_adv, noise, (long long)n);
  return dct_check_launch();
}

extern "C" int dct_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float step_size,
                             float bc2_sqrt, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                             void* bf16_shadow, dct_stream stream) {
  if (!p || !g || !m || !v || n < 1) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return DCT_ERR_UNSUPPORTED;
  if (bf16_shadow && ((uintptr_t)bf16_shadow & 7)) return DCT_ERR_UNSUPPORTED;
  DCT_LAUNCH(DCT_PROF_ADAM, adam_kernel, dim3(wide_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n,
             step_size, bc2_sqrt, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, weight_decay, grad_scale, (bf16_t*)bf16_shadow,
             (const double*)nullptr, (const double*)nullptr, beta1, beta2);
  return dct_check_launch();
}

extern "C" int dct_adam_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, double* state,
                                 const double* table, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                                 void* bf16_shadow, dct_stream stream) {
  if (!p || !g || !m || !v || !state || n < 1) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return DCT_ERR_UNSUPPORTED;
  if (bf16_shadow && ((uintptr_t)bf16_shadow & 7)) return DCT_ERR_UNSUPPORTED;
  if ((uintptr_t)state & 7) return DCT_ERR_UNSUPPORTED;
  DCT_LAUNCH(DCT_PROF_ADAM, adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  DCT_LAUNCH(DCT_PROF_ADAM, adam_kernel, dim3(wide_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n,
             0.f, 1.f, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, weight_decay, grad_scale, (bf16_t*)bf16_shadow,
             (const double*)state, table, beta1, beta2);
  return dct_check_launch();
}

extern "C" size_t dct_grad_sumsq_workspace_bytes(int64_t n) { return n < 1 ? 0 : (size_t)sumsq_grid(n) * sizeof(double); }

extern "C" int dct_grad_sumsq(const float* g, int64_t n, void* workspace, size_t workspace_bytes, dct_stream stream) {
  if (!g || !workspace || n < 1) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)g & 15) || ((uintptr_t)workspace & 7)) return DCT_ERR_UNSUPPORTED;
  if (workspace_bytes < dct_grad_sumsq_workspace_bytes(n)) return DCT_ERR_WORKSPACE;
  DCT_LAUNCH(DCT_PROF_ADAM, grad_sumsq_kernel, dim3(sumsq_grid(n)), dim3(256), 0, (hipStream_t)stream, g, (long long)n, (double*)workspace);
  return dct_check_launch();
}

extern "C" int dct_adam_flat_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, double* state,
                                         const double* table, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                                         void* bf16_shadow, void* workspace, size_t workspace_bytes, dct_adam_guard* guard,
                                         int skip_nonfinite, int clip, dct_stream stream) {
  if (!p || !g || !m || !v || !state || !workspace || !guard || n < 1) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return DCT_ERR_UNSUPPORTED;
  if (bf16_shadow && ((uintptr_t)bf16_shadow & 7)) return DCT_ERR_UNSUPPORTED;
  if (((uintptr_t)state | (uintptr_t)workspace | (uintptr_t)guard) & 7) return DCT_ERR_UNSUPPORTED;
  if (workspace_bytes < dct_grad_sumsq_workspace_bytes(n)) return DCT_ERR_WORKSPACE;
  DCT_LAUNCH(DCT_PROF_ADAM, grad_sumsq_kernel, dim3(sumsq_grid(n)), dim3(256), 0, (hipStream_t)stream, g, (long long)n, (double*)workspace);
  DCT_LAUNCH(DCT_PROF_ADAM, adam_guard_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, (int)sumsq_grid(n),
             state, guard, grad_scale, skip_nonfinite, clip);
  DCT_LAUNCH(DCT_PROF_ADAM, adam_guarded_kernel, dim3(wide_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n,
             (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, weight_decay, grad_scale, (bf16_t*)bf16_shadow,
             (const double*)state, table, beta1, beta2, (const dct_adam_guard*)guard);
  return dct_check_launch();
}
