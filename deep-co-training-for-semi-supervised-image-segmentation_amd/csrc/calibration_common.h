// What calibration.hip and temperature.hip share: the pack of view pointers, the pixel load and THE softmax of the calibration rule
// (include/dct.h): one definition, so that a probability written by dct_temperature_apply at beta = 1 is the one the calibration
// kernel forms from the same logits, bit for bit.
#pragma once
#include "dct_common.h"

namespace {

constexpr int CB_MAXS = 8;                                  // views; + their mean = 9 raters
constexpr int CB_MAXR = CB_MAXS + 1;
struct CbPack { const float* in[CB_MAXS]; };                // the S device pointers travel by value (CfPack of confusion.hip)

template <int C> __device__ __forceinline__ void cb_load(const float* p, float v[C]) {
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

// p = softmax(x) in fp32, max-subtracted, the sum in class order, a true division (include/dct.h)
template <int C> __device__ __forceinline__ void cb_softmax(float v[C]) {
  float m = v[0];
#pragma unroll
  for (int c = 1; c < C; ++c) m = fmaxf(m, v[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { v[c] = expf(v[c] - m); sum += v[c]; }
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = v[c] / sum;
}

}  // namespace

#define CB_DISPATCH_C(Cv, ...)                                       \
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
