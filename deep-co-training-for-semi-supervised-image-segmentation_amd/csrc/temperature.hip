// Temperature scaling of the raters of a batch (rule: include/dct.h): the sums behind the fit of one inverse temperature per rater,
// and the scaled probabilities.
//
// temperature_sums_kernel: for K candidate inverse temperatures per rater, the NLL and its derivative dNLL/dbeta summed over the
// counted pixels, for the S views and, on request, their mean.  Shape of calibration_kernel: grid = (blocks, B), a block owns a
// stretch of one image's pixels, the 16- / 8-byte loads at C = 4 / C = 2, gt decides what counts.  The work is transcendentals, not
// bytes: (C + 1) per rater and candidate and pixel (C expf, one logf; + S C expf and C logf for the mean), about 300 per pixel at
// S = 2 + mean, K = 16, C = 4.  All R * K * 2 sums as per-lane 64-bit accumulators would be up to 288 register pairs, so a block
// walks its stretch once per CHUNK of KC candidates (4; 2 with more than four views) with R * KC * 2 accumulators in registers; the
// first walk fetches the stretch from HBM ((4 C S + 8) bytes per pixel), the others hit L2.  After a walk the wave reduces its
// accumulators, one lane adds them to the block's LDS table of R * K * 2 64-bit cells (2304 bytes at most), and at the end the
// non-zero cells leave through 64-bit integer atomics.  Everything that leaves a lane is an integer: bit-identical from run to run.
//
// temperature_apply_kernel: element-wise, one pass, R outputs; the softmax is calibration_common.h's.
#include "calibration_common.h"

namespace {

constexpr int TP_MAXK = 16;
constexpr float TP_Q = 1048576.0f;                          // 2^20: the fixed-point unit of the NLL and gradient words
struct TpBeta { float b[CB_MAXR]; };                       // slot CB_MAXS is the mean's, whatever S is: no runtime index into a
struct TpOut { float* out[CB_MAXR]; };                      // by-value argument

template <int C> __device__ __forceinline__ void tp_store(float* p, const float v[C]) {
  if constexpr (C == 4) {
    f32x4 t; t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else if constexpr (C == 2) {
    f32x2 t; t[0] = v[0]; t[1] = v[1];
    *reinterpret_cast<f32x2*>(p) = t;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = v[c];
  }
}

// One rater's logits z on one counted pixel of class t against nk <= KC candidates.  The class loops select, they do not index
// (a runtime index would put the array in scratch memory).  x = beta * z is a rounded product of its own (no fused multiply-add
// with the subtraction of the maximum): the rule says so, and (2 z, beta / 2) gives the same words as (z, beta) either way.
// nll >= 0 here (s >= 1: the maximum contributes exactly 1) and min(nll, 4095) * 2^20 < 2^32: one v_cvt_u32_f32; the gradient word
// fits 32 signed bits (2047 * 2^20 < 2^31).  A NaN contributes 0, explicitly: fminf / fmaxf would hand back the bound.
template <int C, int KC>
__device__ __forceinline__ void tp_rater(const float z[C], int t, const float beta[KC], int nk, long long snll[KC], long long sg[KC]) {
  float zy = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) if (c == t) zy = z[c];
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (j < nk) {                           // (uniform)
      float x[C];
#pragma unroll
      for (int c = 0; c < C; ++c) x[c] = __fmul_rn(beta[j], z[c]);
      float m = x[0];
#pragma unroll
      for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
      float s = 0.f, ez = 0.f, xy = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float e = expf(x[c] - m);
        s += e;
        ez += e * z[c];
        if (c == t) xy = x[c];
      }
      const float nll = logf(s) - (xy - m);
      const float g = ez / s - zy;
      const float nc = nll == nll ? fminf(nll, 4095.f) : 0.f;
      const float gc = g == g ? fminf(fmaxf(g, -2047.f), 2047.f) : 0.f;
      snll[j] += (long long)(unsigned)rintf(nc * TP_Q);
      sg[j] += (long long)(int)rintf(gc * TP_Q);
    }
  }
}

__device__ __forceinline__ long long tp_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// NS = 2, 4 or 8 >= S: the loads of a pixel are issued together; the slots from S on read view 0 again (a cache hit) and are not
// looked at.  Accumulator slot NS is the mean of the views; in the table it is rater S.
template <int C, int NS, int KC>
__global__ __launch_bounds__(256) void temperature_sums_kernel(CbPack pk, int S, int ens, const long long* gt, long long PPI, unsigned class_mask,
                                                               const float* betas, int K, unsigned long long* sums,
                                                               unsigned long long* counted_out) {
  __shared__ unsigned long long h[CB_MAXR * TP_MAXK * 2 + 1];
  const int R = S + (ens ? 1 : 0), cells = R * K * 2;
  for (int i = threadIdx.x; i <= cells; i += 256) h[i] = 0;      // cell `cells`: the counted pixels
  __syncthreads();
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const long long img = (long long)b * PPI;
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int nk = K - k0 < KC ? K - k0 : KC;
    float beta[NS + 1][KC];
    long long snll[NS + 1][KC], sg[NS + 1][KC];
#pragma unroll
    for (int s = 0; s <= NS; ++s) {
      const int r = s < NS ? (s < S ? s : 0) : (ens ? S : 0);
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        beta[s][j] = betas[r * K + k0 + (j < nk ? j : 0)];
        snll[s][j] = 0;
        sg[s][j] = 0;
      }
    }
    int n = 0;
    for (long long base = (long long)blockIdx.x * 256; base < PPI; base += (long long)gridDim.x * 256) {
      const long long pix = base + threadIdx.x;
      if (pix < PPI) {
        float v[NS][C];
#pragma unroll
        for (int s = 0; s < NS; ++s) cb_load<C>((s < S ? pk.in[s] : pk.in[0]) + (img + pix) * C, v[s]);
        const long long g = gt[img + pix];
        if (g >= 0 && g < C && ((class_mask >> (g & 31)) & 1u)) {
          const int t = (int)g;
          ++n;
          float e[C];
#pragma unroll
          for (int c = 0; c < C; ++c) e[c] = 0.f;
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            if (s < S) {                    // (uniform)
              tp_rater<C, KC>(v[s], t, beta[s], nk, snll[s], sg[s]);
              if (ens) {
                cb_softmax<C>(v[s]);        // at temperature 1: the calibration rule's mean
#pragma unroll
                for (int c = 0; c < C; ++c) e[c] += v[s][c];    // in view order
              }
            }
          }
          if (ens) {
            const float fs = (float)S;
#pragma unroll
            for (int c = 0; c < C; ++c) e[c] = logf(e[c] / fs + 1e-10f);
            tp_rater<C, KC>(e, t, beta[NS], nk, snll[NS], sg[NS]);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s <= NS; ++s) {
      if (s < NS ? s < S : ens != 0) {      // (uniform)
        unsigned long long* hp = h + ((s < NS ? s : S) * K + k0) * 2;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
          if (j < nk) {
            const long long a = tp_wave_sum(snll[s][j]), d = tp_wave_sum(sg[s][j]);
            if (lane == 0) {
              if (a) atomicAdd(hp + j * 2, (unsigned long long)a);
              if (d) atomicAdd(hp + j * 2 + 1, (unsigned long long)d);       // two's complement: the signed sum
            }
          }
        }
      }
    }
    if (k0 == 0) {
      const long long c = tp_wave_sum((long long)n);
      if (lane == 0 && c) atomicAdd(h + cells, (unsigned long long)c);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += 256) {
    const unsigned long long v = h[i];
    if (v) atomicAdd(sums + i, v);
  }
  if (threadIdx.x == 0 && h[cells]) atomicAdd(counted_out, h[cells]);
}

template <int C, int NS>
__global__ __launch_bounds__(256) void temperature_apply_kernel(CbPack pk, int S, int ens, long long PPI, TpBeta bt, TpOut po) {
  const long long img = (long long)blockIdx.y * PPI;
  for (long long pix = (long long)blockIdx.x * 256 + threadIdx.x; pix < PPI; pix += (long long)gridDim.x * 256) {
    const long long at = (img + pix) * C;
    float v[NS][C];
#pragma unroll
    for (int s = 0; s < NS; ++s) cb_load<C>((s < S ? pk.in[s] : pk.in[0]) + at, v[s]);
    float e[C];
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s < S) {                          // (uniform)
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = __fmul_rn(bt.b[s], v[s][c]);
        cb_softmax<C>(x);
        tp_store<C>(po.out[s] + at, x);
        if (ens) {
          cb_softmax<C>(v[s]);
#pragma unroll
          for (int c = 0; c < C; ++c) e[c] += v[s][c];
        }
      }
    }
    if (ens) {
      const float fs = (float)S;
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = __fmul_rn(bt.b[CB_MAXS], logf(e[c] / fs + 1e-10f));
      cb_softmax<C>(e);
      tp_store<C>(po.out[CB_MAXS] + at, e);
    }
  }
}

// The refusals the two entry points share; leaves the pack and the grid's x extent.
int tp_check(const float* const* logits, int S, int B, int64_t ppi, int C_, int with_ensemble, CbPack& pk, long long& bx) {
  if (!logits || S < 1 || B < 1 || ppi < 1) return DCT_ERR_BAD_ARG;
  if (with_ensemble != 0 && with_ensemble != 1) return DCT_ERR_BAD_ARG;
  if (S > CB_MAXS || C_ < 1 || C_ > 8 || ppi >= (int64_t)1 << 31 || B > 65535) return DCT_ERR_UNSUPPORTED;
  const uintptr_t palign = C_ == 4 ? 15 : (C_ == 2 ? 7 : 3);      // the widest load of cb_load<C>
  for (int s = 0; s < CB_MAXS; ++s) pk.in[s] = nullptr;
  for (int s = 0; s < S; ++s) {
    if (!logits[s] || ((uintptr_t)logits[s] & palign)) return DCT_ERR_BAD_ARG;
    pk.in[s] = logits[s];
  }
  bx = (ppi + 255) / 256;
  if (bx > 64) bx = 64;
  return DCT_OK;
}

}  // namespace

extern "C" int dct_temperature_sums(const float* const* logits, int S, const int64_t* gt, int B, int64_t pixels_per_image, int C_,
                                    uint32_t class_mask, int with_ensemble, const float* betas, int K, int64_t* sums, int64_t* counted,
                                    dct_stream stream) {
  if (!gt || !betas || !sums || !counted) return DCT_ERR_BAD_ARG;
  CbPack pk;
  long long bx = 0;
  const int rc = tp_check(logits, S, B, pixels_per_image, C_, with_ensemble, pk, bx);
  if (rc == DCT_ERR_BAD_ARG) return rc;
  if (rc != DCT_OK || K < 1 || K > TP_MAXK) return DCT_ERR_UNSUPPORTED;
  if (((uintptr_t)gt & 7) || ((uintptr_t)betas & 3) || ((uintptr_t)sums & 7) || ((uintptr_t)counted & 7)) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
#define TP_LAUNCH(NS, KC) DCT_LAUNCH(DCT_PROF_LOSS, (temperature_sums_kernel<C, NS, KC>), dim3((unsigned)bx, (unsigned)B), dim3(256), 0, st, pk, S,  \
                                     with_ensemble, (const long long*)gt, (long long)pixels_per_image, (unsigned)class_mask, betas, K,                   \
                                     (unsigned long long*)sums, (unsigned long long*)counted)
  if (S <= 2) { CB_DISPATCH_C(C_, TP_LAUNCH(2, 4)); }
  else if (S <= 4) { CB_DISPATCH_C(C_, TP_LAUNCH(4, 4)); }
  else { CB_DISPATCH_C(C_, TP_LAUNCH(8, 2)); }
#undef TP_LAUNCH
  return dct_check_launch();
}

extern "C" int dct_temperature_apply(const float* const* logits, int S, int B, int64_t pixels_per_image, int C_, const float* beta,
                                     int with_ensemble, float* const* out, dct_stream stream) {
  if (!beta || !out) return DCT_ERR_BAD_ARG;
  CbPack pk;
  long long bx = 0;
  const int rc = tp_check(logits, S, B, pixels_per_image, C_, with_ensemble, pk, bx);
  if (rc != DCT_OK) return rc;
  const uintptr_t palign = C_ == 4 ? 15 : (C_ == 2 ? 7 : 3);
  TpBeta bt;
  TpOut po;
  const int R = S + with_ensemble;
  for (int r = 0; r < CB_MAXR; ++r) { bt.b[r] = 0.f; po.out[r] = nullptr; }
  for (int r = 0; r < R; ++r) {
    if (!out[r] || ((uintptr_t)out[r] & palign)) return DCT_ERR_BAD_ARG;
    const int slot = r < S ? r : CB_MAXS;
    bt.b[slot] = beta[r];
    po.out[slot] = out[r];
  }
  hipStream_t st = (hipStream_t)stream;
#define TP_LAUNCH(NS) DCT_LAUNCH(DCT_PROF_LOSS, (temperature_apply_kernel<C, NS>), dim3((unsigned)bx, (unsigned)B), dim3(256), 0, st, pk, S,  \
                                 with_ensemble, (long long)pixels_per_image, bt, po)
  if (S <= 2) { CB_DISPATCH_C(C_, TP_LAUNCH(2)); }
  else if (S <= 4) { CB_DISPATCH_C(C_, TP_LAUNCH(4)); }
  else { CB_DISPATCH_C(C_, TP_LAUNCH(8)); }
#undef TP_LAUNCH
  return dct_check_launch();
}
