// Virtual adversarial examples (the rule: include/dct.h, "VAT"): Gaussian noise a captured step redraws on every replay, the L2 norm of
// every sample in a fixed order, and x + (radius / norm) * d.
//
// One walk for all three kernels.  A sample of `per` elements is cut into vat_bps(per) chunks of vat_chunk(per) elements (a multiple of
// four), one block of 256 per chunk: block (n, b) = blockIdx.x / bps, blockIdx.x % bps.  Where the sample's first element is 16-byte aligned
// (the pointers are, and n * per is a multiple of four) thread t takes the groups of four elements lo / 4 + t, + 256, ... of its chunk as
// 16-byte accesses and the last block's first per % 4 threads take the tail one element each; elsewhere (an odd `per` misaligns every
// second sample) thread t takes the elements lo + t, + 256, ... one by one.  A thread adds the squares of its elements in that order in
// double -- a finite fp32 squared is exact there and cannot overflow, so 1e-20 and 1e+20 keep their direction -- the block folds its lanes
// (xor 32 .. 1) and then its four waves in order.  Noise and sumsq share the walk, so the partials the noise launch writes beside d are
// bit for bit those dct_vat_sumsq gives for d.  The perturb launch has the same grid: the first wave of every block folds its sample's
// partials, lane l holding partial l (0.0 from bps on), xor 32 .. 1 -- commutative adds, so every lane of every block of a sample holds
// the same bits and no finalize launch is needed between.
#include "dct_common.h"
#include <cmath>

namespace {

constexpr int kVatChunk = 4096;      // elements of a sample per block (16 per thread) ...
constexpr int kVatMaxBlocks = 64;    // ... until a sample has this many blocks: one lane of a wave per partial in the fold

inline int vat_bps(long long per) {
  const long long b = (per + kVatChunk - 1) / kVatChunk;
  return (int)(b < 1 ? 1 : (b > kVatMaxBlocks ? kVatMaxBlocks : b));
}
inline long long vat_chunk(long long per, int bps) { return (((per + bps - 1) / bps) + 3) & ~3ll; }

// Box-Muller on two words: u1 in (0, 1], u2 in [0, 1), both exact in fp32; the precise logf / sqrtf / cosf / sinf.
__device__ __forceinline__ void vat_normal_pair(unsigned ra, unsigned rb, float& even, float& odd) {
  const float u1 = (float)((ra >> 8) + 1u) * 5.9604644775390625e-08f;
  const float u2 = (float)(rb >> 8) * 5.9604644775390625e-08f;
  const float rho = sqrtf(-2.f * logf(u1));
  const float a = 6.283185307179586f * u2;
  even = rho * cosf(a);
  odd = rho * sinf(a);
}

struct VatRange {
  long long base, lo, hi;     // the sample's first flat element; this block's elements [lo, hi) of the sample
  int n, b;
  bool vec;
};
__device__ __forceinline__ VatRange vat_range(long long per, int bps, long long chunk, int ptr_aligned) {
  VatRange r;
  r.n = (int)(blockIdx.x / (unsigned)bps);
  r.b = (int)(blockIdx.x % (unsigned)bps);
  r.base = (long long)r.n * per;
  const long long lo = (long long)r.b * chunk;
  r.lo = lo < per ? lo : per;
  r.hi = r.lo + chunk < per ? r.lo + chunk : per;
  r.vec = ptr_aligned && !(r.base & 3);
  return r;
}

// f4(i) handles the sample's elements i .. i + 3 (i a multiple of four, the sample's base aligned), f1(i) element i; both return the sum
// of squares so far with theirs added.
template <typename F4, typename F1>
__device__ __forceinline__ double vat_walk(const VatRange& r, F4 f4, F1 f1) {
  double acc = 0.0;
  if (r.vec) {
    const long long g_hi = r.hi >> 2;
    for (long long g = (r.lo >> 2) + threadIdx.x; g < g_hi; g += 256) acc = f4(g << 2, acc);
    const long long t = (g_hi << 2) + threadIdx.x;      // (only the block that ends the sample has a tail)
    if (t < r.hi) acc = f1(t, acc);
  } else {
    for (long long i = r.lo + threadIdx.x; i < r.hi; i += 256) acc = f1(i, acc);
  }
  return acc;
}
__device__ __forceinline__ double sq_add(float v, double acc) {
  const double d = (double)v;
  return fma(d, d, acc);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ void vat_store_partial(double acc, double* partials) {
  __shared__ double sw[4];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

__global__ __launch_bounds__(256) void vat_noise_kernel(float* __restrict__ d, long long per, int bps, long long chunk, int ptr_aligned,
                                                         unsigned long long seed, const unsigned long long* __restrict__ calls,
                                                         unsigned long long offset, double* __restrict__ partials) {
  const unsigned long long call = calls ? calls[0] + 1ull : offset;
  const unsigned long long ctr0 = call << 40;
  const VatRange r = vat_range(per, bps, chunk, ptr_aligned);
  const double acc = vat_walk(
      r,
      [&](long long i, double a) {          // the group's four flat elements share one counter: base + i is a multiple of four
        unsigned w[4];
        philox4x32_10(seed, ctr0 + (unsigned long long)((r.base + i) >> 2), w);
        f32x4 v;
        float e, o;
        vat_normal_pair(w[0], w[1], e, o); v[0] = e; v[1] = o;
        vat_normal_pair(w[2], w[3], e, o); v[2] = e; v[3] = o;
        *reinterpret_cast<f32x4*>(d + r.base + i) = v;
#pragma unroll
        for (int k = 0; k < 4; ++k) a = sq_add(v[k], a);
        return a;
      },
      [&](long long i, double a) {
        const long long e = r.base + i;
        unsigned w[4];
        philox4x32_10(seed, ctr0 + (unsigned long long)(e >> 2), w);
        float ev, od;
        if (e & 2) vat_normal_pair(w[2], w[3], ev, od);
        else vat_normal_pair(w[0], w[1], ev, od);
        const float v = (e & 1) ? od : ev;
        d[e] = v;
        return sq_add(v, a);
      });
  vat_store_partial(acc, partials);
}

__global__ __launch_bounds__(256) void vat_sumsq_kernel(const float* __restrict__ g, long long per, int bps, long long chunk, int ptr_aligned,
                                                         double* __restrict__ partials) {
  const VatRange r = vat_range(per, bps, chunk, ptr_aligned);
  const double acc = vat_walk(
      r,
      [&](long long i, double a) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + r.base + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) a = sq_add(v[k], a);
        return a;
      },
      [&](long long i, double a) { return sq_add(g[r.base + i], a); });
  vat_store_partial(acc, partials);
}

// scale * d and x + that as two ROUNDED operations: x_out is fl(x + r_out) of the r_out that is stored.  (hipcc contracts a * b + c
// into a fused multiply-add by default, through __fmul_rn / __fadd_rn too: the pragma is what keeps the two roundings.)
__device__ __forceinline__ void vat_move(float x, float d, float scale, bool ok, float& xo, float& ro) {
#pragma clang fp contract(off)
  const float p = scale * d;
  ro = ok ? p : 0.f;                        // a sample without a direction takes neither the product nor the sum: 0 * NaN is NaN
  xo = ok ? x + p : x;
}

__global__ __launch_bounds__(256) void vat_perturb_kernel(const float* __restrict__ x, const float* __restrict__ d, double radius, long long per,
                                                           int bps, long long chunk, int ptr_aligned, const double* __restrict__ partials,
                                                           float* __restrict__ x_out, float* __restrict__ r_out, double* __restrict__ norms_out,
                                                           unsigned long long* calls_advance) {
  __shared__ double s_sum;
  const VatRange r = vat_range(per, bps, chunk, ptr_aligned);
  if (threadIdx.x < 64) {
    const double s = wave_sum_f64((int)threadIdx.x < bps ? partials[(long long)r.n * bps + threadIdx.x] : 0.0);
    if (threadIdx.x == 0) s_sum = s;
  }
  __syncthreads();
  const double norm = sqrt(s_sum);
  const bool ok = norm > 0.0 && norm <= 1.7976931348623157e308;      // 0, inf and NaN: no direction, a zero perturbation
  const float scale = ok ? (float)(radius / norm) : 0.f;
  if (threadIdx.x == 0) {
    if (norms_out && r.b == 0) norms_out[r.n] = norm;
    // the noise launch in front read this word; no block of THIS launch does, so one thread may advance it in place
    if (calls_advance && blockIdx.x == 0) calls_advance[0] = calls_advance[0] + 1ull;
  }
  vat_walk(
      r,
      [&](long long i, double a) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r.base + i);
        const f32x4 dv = *reinterpret_cast<const f32x4*>(d + r.base + i);
        f32x4 xo, ro;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float a_, b_;
          vat_move(xv[k], dv[k], scale, ok, a_, b_);
          xo[k] = a_; ro[k] = b_;
        }
        *reinterpret_cast<f32x4*>(x_out + r.base + i) = xo;
        if (r_out) *reinterpret_cast<f32x4*>(r_out + r.base + i) = ro;
        return a;
      },
      [&](long long i, double a) {
        float xo, ro;
        vat_move(x[r.base + i], d[r.base + i], scale, ok, xo, ro);
        x_out[r.base + i] = xo;
        if (r_out) r_out[r.base + i] = ro;
        return a;
      });
}

// N * per elements: the Philox counter keeps 40 bits for the group index, the grid 31 for the blocks
inline bool vat_shape_ok(int64_t N, int64_t per) {
  if (N < 1 || per < 1) return false;
  if (per > (1ll << 40) || N > (1ll << 31)) return false;
  if ((__int128)N * per > ((__int128)1 << 42)) return false;
  return (long long)N * vat_bps(per) < (1ll << 31);
}
inline int aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* e = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)e) & 15) == 0;
}

}  // namespace

extern "C" size_t dct_vat_workspace_bytes(int64_t N, int64_t per) {
  return vat_shape_ok(N, per) ? (size_t)N * vat_bps(per) * sizeof(double) : 0;
}

extern "C" int dct_vat_noise(float* d, int64_t N, int64_t per, uint64_t seed, const uint64_t* calls, uint64_t offset, void* workspace,
                             size_t workspace_bytes, dct_stream stream) {
  if (!d || !workspace || !vat_shape_ok(N, per) || ((uintptr_t)d & 3) || ((uintptr_t)workspace & 7) || ((uintptr_t)calls & 7)) return DCT_ERR_BAD_ARG;
  if (workspace_bytes < dct_vat_workspace_bytes(N, per)) return DCT_ERR_WORKSPACE;
  const int bps = vat_bps(per);
  DCT_LAUNCH(DCT_PROF_OTHER, vat_noise_kernel, dim3((unsigned)(N * bps)), dim3(256), 0, (hipStream_t)stream, d, (long long)per, bps,
             vat_chunk(per, bps), aligned16(d), (unsigned long long)seed, (const unsigned long long*)calls, (unsigned long long)offset,
             (double*)workspace);
  return dct_check_launch();
}

extern "C" int dct_vat_sumsq(const float* g, int64_t N, int64_t per, void* workspace, size_t workspace_bytes, dct_stream stream) {
  if (!g || !workspace || !vat_shape_ok(N, per) || ((uintptr_t)g & 3) || ((uintptr_t)workspace & 7)) return DCT_ERR_BAD_ARG;
  if (workspace_bytes < dct_vat_workspace_bytes(N, per)) return DCT_ERR_WORKSPACE;
  const int bps = vat_bps(per);
  DCT_LAUNCH(DCT_PROF_OTHER, vat_sumsq_kernel, dim3((unsigned)(N * bps)), dim3(256), 0, (hipStream_t)stream, g, (long long)per, bps,
             vat_chunk(per, bps), aligned16(g), (double*)workspace);
  return dct_check_launch();
}

extern "C" int dct_vat_perturb(const float* x, const float* d, double radius, int64_t N, int64_t per, const void* workspace,
                               size_t workspace_bytes, float* x_out, float* r_out, double* norms_out, uint64_t* calls_advance,
                               dct_stream stream) {
  if (!x || !d || !x_out || !workspace || !vat_shape_ok(N, per) || !(radius > 0.0) || !(radius <= 1.7976931348623157e308)) return DCT_ERR_BAD_ARG;
  if ((((uintptr_t)x | (uintptr_t)d | (uintptr_t)x_out | (uintptr_t)r_out) & 3) || ((uintptr_t)workspace & 7) || ((uintptr_t)norms_out & 7) ||
      ((uintptr_t)calls_advance & 7))
    return DCT_ERR_BAD_ARG;
  if (workspace_bytes < dct_vat_workspace_bytes(N, per)) return DCT_ERR_WORKSPACE;
  const int bps = vat_bps(per);
  DCT_LAUNCH(DCT_PROF_OTHER, vat_perturb_kernel, dim3((unsigned)(N * bps)), dim3(256), 0, (hipStream_t)stream, x, d, radius, (long long)per, bps,
             vat_chunk(per, bps), aligned16(x, d, x_out, r_out), (const double*)workspace, x_out, r_out, norms_out,
             (unsigned long long*)calls_advance);
  return dct_check_launch();
}
