// Pairwise confusion matrices of the raters of a batch (the counts behind Cohen's kappa of Summary.py:70-252 and behind the
// reference's ConfusionMatrix / IoU meters): ONE pass over the S logit tensors and gt leaves counts[b][pair][a][c] for every pair
// of raters (rule and pair order: include/dct.h).  HBM-bound by design: (16 S + 8) bytes per pixel at C = 4.
//
// A block owns a stretch of one image's pixels and a histogram of P * C * C int32 in LDS (9 KiB at S = 8 + gt, C = 8).  Register
// counters per thread (dice_kernel) do not scale to P * C^2 cells, and 64 lanes adding 1 to one LDS address serialise -- on a
// segmentation map ~90 % of the pixels of every pair land in cell (0, 0).  So the wave aggregates first: per pair, take the cell
// of the first lane that still has one, ballot the lanes that share it, one lane adds the popcount, those lanes retire.  That is
// one to three trips per pair on blob maps and at most min(64, C^2) on noise.  The block's non-zero cells go to global memory by
// integer atomics: sums of integers do not depend on their order, the result is bit-identical from run to run.
#include "dct_common.h"

namespace {

constexpr int CF_MAXS = 8;                                  // predictions; + gt = 9 raters, 36 pairs
constexpr int CF_MAXP = (CF_MAXS + 1) * CF_MAXS / 2;
struct CfPack { const float* in[CF_MAXS]; };                // the S device pointers travel by value (PtrPack of loss.hip)

template <int C> __device__ __forceinline__ void cf_load(const float* p, float v[C]) {
  if constexpr (C == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if constexpr (C == 2) {
    const f32x2 t = *reinterpret_cast<const f32x2*>(p);
    v[0] = t[0]; v[1] = t[1];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[c];
  }
}

// grid = (blocks, B); every wave runs the same number of trips of the pixel loop (a lane past the image's end is merely inactive),
// so the ballots below see whole waves.  NS = 2, 4 or 8 >= S: the loads of a pixel are issued together, without a branch between
// them; the slots from S on read rater 0 again (a cache hit) and are left out of the code word.
template <int C, int NS>
__global__ __launch_bounds__(256) void confusion_kernel(CfPack pk, int S, const long long* gt, long long PPI, int* counts) {
  constexpr int CC = C * C;
  __shared__ int h[CF_MAXP * CC];
  const int R = S + (gt ? 1 : 0), P = R * (R - 1) / 2;
  for (int i = threadIdx.x; i < P * CC; i += 256) h[i] = 0;
  __syncthreads();
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const long long img = (long long)b * PPI;
  for (long long base = (long long)blockIdx.x * 256; base < PPI; base += (long long)gridDim.x * 256) {
    const long long pix = base + threadIdx.x;
    const bool active = pix < PPI;
    unsigned code = 0;                      // three bits per rater: C <= 8
    bool gt_ok = false;
    if (active) {
      float v[NS][C];
      long long t = -1;
#pragma unroll
      for (int s = 0; s < NS; ++s) cf_load<C>((s < S ? pk.in[s] : pk.in[0]) + (img + pix) * C, v[s]);
      if (gt) t = gt[img + pix];
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        int best = 0;                       // first maximum, as dct_argmax (the running value beside the index: v[s][best] would
        float top = v[s][0];                // be a runtime index, and the array would live in scratch memory)
#pragma unroll
        for (int c = 1; c < C; ++c) if (v[s][c] > top) { top = v[s][c]; best = c; }
        if (s < S) code |= (unsigned)best << (3 * s);
      }
      gt_ok = t >= 0 && t < C;              // outside [0, C): in no pair that contains gt
      if (gt_ok) code |= (unsigned)t << (3 * S);
    }
    int* hp = h;
    for (int i = 0; i < R - 1; ++i) {
      const int a = (code >> (3 * i)) & 7;
      for (int j = i + 1; j < R; ++j, hp += CC) {
        const int cell = a * C + (int)((code >> (3 * j)) & 7);
        bool todo = active && (j < S || gt_ok);
        for (;;) {
          const unsigned long long rem = __ballot(todo);
          if (!rem) break;
          const int first = __ffsll((long long)rem) - 1;
          const int fc = __builtin_amdgcn_readlane(cell, first);
          const unsigned long long same = __ballot(todo && cell == fc);
          if (lane == first) atomicAdd(hp + fc, __popcll(same));
          todo = todo && cell != fc;
        }
      }
    }
  }
  __syncthreads();
  int* out = counts + (long long)b * P * CC;
  for (int i = threadIdx.x; i < P * CC; i += 256) {
    const int v = h[i];
    if (v) atomicAdd(out + i, v);
  }
}

}  // namespace

#define CF_DISPATCH_C(Cv, ...)                                       \
  switch (Cv) {                                                      \
    case 1: { constexpr int C = 1; __VA_ARGS__; } break;             \
    case 2: { constexpr int C = 2; __VA_ARGS__; } break;             \
    case 3: { constexpr int C = 3; __VA_ARGS__; } break;             \
    case 4: { constexpr int C = 4; __VA_ARGS__; } break;             \
    case 5: { constexpr int C = 5; __VA_ARGS__; } break;             \
    case 6: { constexpr int C = 6; __VA_ARGS__; } break;             \
    case 7: { constexpr int C = 7; __VA_ARGS__; } break;             \
    default: { constexpr int C = 8; __VA_ARGS__; } break;            \
  }

extern "C" int dct_confusion_counts(const float* const* logits, int S, const int64_t* gt, int B, int64_t pixels_per_image, int C_,
                                    int32_t* counts, dct_stream stream) {
  if (!logits || !counts || S < 1 || B < 1 || pixels_per_image < 1) return DCT_ERR_BAD_ARG;
  if (S + (gt ? 1 : 0) < 2) return DCT_ERR_BAD_ARG;
  if (S > CF_MAXS || C_ < 1 || C_ > 8 || pixels_per_image >= (int64_t)1 << 31 || B > 65535) return DCT_ERR_UNSUPPORTED;
  const uintptr_t lalign = C_ == 4 ? 15 : (C_ == 2 ? 7 : 3);      // the widest load of cf_load<C>
  CfPack pk;
  for (int s = 0; s < CF_MAXS; ++s) pk.in[s] = nullptr;
  for (int s = 0; s < S; ++s) {
    if (!logits[s] || ((uintptr_t)logits[s] & lalign)) return DCT_ERR_BAD_ARG;
    pk.in[s] = logits[s];
  }
  if (((uintptr_t)gt & 7) || ((uintptr_t)counts & 3)) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  long long bx = (pixels_per_image + 255) / 256;
  if (bx > 64) bx = 64;
#define CF_LAUNCH(NS) DCT_LAUNCH(DCT_PROF_LOSS, (confusion_kernel<C, NS>), dim3((unsigned)bx, (unsigned)B), dim3(256), 0, st, pk, S, \
                              (const long long*)gt, (long long)pixels_per_image, counts)
  if (S <= 2) { CF_DISPATCH_C(C_, CF_LAUNCH(2)); }
  else if (S <= 4) { CF_DISPATCH_C(C_, CF_LAUNCH(4)); }
  else { CF_DISPATCH_C(C_, CF_LAUNCH(8)); }
#undef CF_LAUNCH
  return dct_check_launch();
}
