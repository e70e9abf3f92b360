// Hausdorff distance between the predicted and the ground-truth mask of every class (Summary.py:70-252 reports it next to the
// Dice score), by the exact separable squared-distance transform: its cost does not depend on the masks, where all pairs of
// surface pixels would be ~1e9 per slice and class on the noise an untrained network predicts.
//
//   P = {argmax == c} (first maximum, as dct_argmax / dct_dice_counts), G = {gt == c}; a gt value outside [0, C) is in no class.
//   surface = foreground pixels with a background neighbour among the 4 in-plane (2-D) / 6 (3-D: the batch is the volume)
//             neighbours; outside the array is background.
//   hd2 = max( max_{p in dP} min_{q in dG} d2(p, q), max_{q in dG} min_{p in dP} d2(p, q) ),  d2 = (sz dz)^2 + (sy dy)^2 + (sx dx)^2
//   P or G empty: NaN.
//
// Launch chain (all on the caller's stream, everything between them lives in the caller's workspace):
//   1. hd_classify   one read of the logits (argmax in registers) and of gt -> one class byte per pixel and side (255 = no class)
//   2. hd_surface    class bytes -> surface bytes: the pixel's class where it is on that class's surface, 255 elsewhere.  A pixel
//                    belongs to one class only, so ONE byte map per side carries the surfaces of all C classes.
//   3. hd_columns    g[side][b][c][y][x] = (sy (y - y'))^2 to the nearest surface pixel y' of class c in column x (two scans), +inf
//                    where the column has none
//   4. hd_slices     3-D only: g3[z] = min_z' (sz (z - z'))^2 + g[z']
//   5. hd_rows       a block owns one image row of one (side, b, c) map and holds its g values in LDS; every thread whose pixel is
//                    on the OTHER side's surface of class c takes min_x' (sx (x - x'))^2 + g[x'] (LDS reads are broadcasts: all
//                    lanes read the same four x'); the wave maxima go to acc[row][c] by atomic max on the bit pattern (+ 1, so that
//                    0 means "nothing arrived").  Non-negative floats order like their bit patterns and a maximum does not depend on
//                    the order of its operands: the result is bit-identical from run to run.
//   6. hd_finish     acc -> hd2 (NaN where nothing arrived or +inf did: one of the masks is empty)
// With unit spacing every intermediate is an integer below 2^24: fp32 is exact.
#include "dct_common.h"
#include <math.h>

#define HD_NONE 255
#define HD_MAX_EXTENT 1024

namespace {

struct HdWs {               // byte offsets into the workspace
  size_t acc, pcls, surf, g, g3, total;
};
inline size_t hd_round(size_t v) { return (v + 255) & ~(size_t)255; }
inline HdWs hd_layout(int B, int H, int W, int C, int method3d) {
  const size_t px = (size_t)B * H * W;
  HdWs w;
  w.acc = 0;
  w.pcls = hd_round((size_t)B * C * 4);
  w.surf = w.pcls + hd_round(2 * px);
  w.g = w.surf + hd_round(2 * px);
  w.g3 = w.g + hd_round(2 * px * C * 4);
  w.total = method3d ? w.g3 + hd_round(2 * px * C * 4) : w.g3;
  return w;
}

template <int C> __device__ __forceinline__ int hd_argmax(const float* p) {
  float v[C];
  if constexpr (C == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if constexpr (C == 8) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p), u = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; v[4] = u[0]; v[5] = u[1]; v[6] = u[2]; v[7] = u[3];
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[c];
  }
  int best = 0;
#pragma unroll
  for (int c = 1; c < C; ++c) if (v[c] > v[best]) best = c;
  return best;
}
__device__ __forceinline__ unsigned hd_gt_class(long long t, int C) { return (t >= 0 && t < C) ? (unsigned)t : HD_NONE; }

// cls[0][px] = argmax, cls[1][px] = gt class; four pixels per thread (16-byte gt loads, 4-byte class stores).  Also clears acc.
template <int C>
__global__ __launch_bounds__(256) void hd_classify(const float* logits, const long long* gt, long long px, uint8_t* cls, unsigned* acc, int nacc) {
  if (blockIdx.x == 0) for (int i = threadIdx.x; i < nacc; i += 256) acc[i] = 0u;
  uint8_t* pc = cls;
  uint8_t* gc = cls + px;
  for (long long q = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; q < px; q += (long long)gridDim.x * 1024) {
    if (q + 4 <= px && (px & 3) == 0) {       // (the gt classes start at cls + px: 4-byte stores need px % 4 == 0)
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      const i64x2 t0 = *reinterpret_cast<const i64x2*>(gt + q), t1 = *reinterpret_cast<const i64x2*>(gt + q + 2);
      unsigned p = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) p |= (unsigned)hd_argmax<C>(logits + (q + k) * C) << (8 * k);
      const unsigned g = hd_gt_class(t0[0], C) | hd_gt_class(t0[1], C) << 8 | hd_gt_class(t1[0], C) << 16 | hd_gt_class(t1[1], C) << 24;
      *reinterpret_cast<unsigned*>(pc + q) = p;
      *reinterpret_cast<unsigned*>(gc + q) = g;
    } else {
      for (long long i = q; i < px && i < q + 4; ++i) {
        pc[i] = (uint8_t)hd_argmax<C>(logits + i * C);
        gc[i] = (uint8_t)hd_gt_class(gt[i], C);
      }
    }
  }
}

// surf[side][b][y][x] = cls where a neighbour (4 in the plane; + the two slices beside it in 3-D) differs or lies outside, else 255
__global__ __launch_bounds__(256) void hd_surface(const uint8_t* cls, uint8_t* surf, int B, int H, int W, int method3d) {
  const long long px = (long long)B * H * W, plane = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 2 * px; i += (long long)gridDim.x * 256) {
    const long long j = i < px ? i : i - px;
    const int x = (int)(j % W), y = (int)((j / W) % H), b = (int)(j / plane);
    const uint8_t v = cls[i];
    bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1 && (!method3d || (b > 0 && b < B - 1));
    if (inner && v != HD_NONE) {
      inner = cls[i - 1] == v && cls[i + 1] == v && cls[i - W] == v && cls[i + W] == v;
      if (method3d) inner = inner && cls[i - plane] == v && cls[i + plane] == v;
    }
    surf[i] = inner ? (uint8_t)HD_NONE : v;
  }
}

// One thread per (side, b, c, column): a scan down writes the squared distance to the nearest surface pixel above, a scan up takes
// the minimum with the one below.  cnt counts pixels since the last surface pixel; +inf until one is met (inf + 1 = inf).
__global__ __launch_bounds__(64) void hd_columns(const uint8_t* surf, float* g, int B, int H, int W, int C, float sy) {
  const int xchunks = (W + 63) / 64;
  const int b = blockIdx.x / xchunks, x = (blockIdx.x - b * xchunks) * 64 + threadIdx.x, c = blockIdx.y, side = blockIdx.z;
  if (x >= W) return;
  const uint8_t* sp = surf + ((size_t)side * B + b) * H * W + x;
  float* gp = g + (((size_t)side * B + b) * C + c) * H * W + x;
  float cnt = INFINITY;
#pragma unroll 4
  for (int y = 0; y < H; ++y) {
    cnt = sp[(size_t)y * W] == c ? 0.f : cnt + 1.f;
    const float t = cnt * sy;
    gp[(size_t)y * W] = t * t;
  }
  cnt = INFINITY;
#pragma unroll 4
  for (int y = H - 1; y >= 0; --y) {
    cnt = sp[(size_t)y * W] == c ? 0.f : cnt + 1.f;
    const float t = cnt * sy;
    gp[(size_t)y * W] = fminf(gp[(size_t)y * W], t * t);
  }
}

// g3[side][z][c][y][x] = min_z' (sz (z - z'))^2 + g[side][z'][c][y][x]
__global__ __launch_bounds__(256) void hd_slices(const float* g, float* g3, int B, int H, int W, int C, float sz) {
  const int xchunks = (W + 255) / 256;
  const int zy = blockIdx.x / xchunks, x = (blockIdx.x - zy * xchunks) * 256 + threadIdx.x, c = blockIdx.y, side = blockIdx.z;
  if (x >= W) return;
  const int z = zy / H, y = zy - z * H;
  const size_t plane = (size_t)H * W, in_plane = (size_t)y * W + x;
  const float* gp = g + ((size_t)side * B * C + c) * plane + in_plane;
  float best = INFINITY;
  for (int k = 0; k < B; ++k) {
    const float d = (float)(z - k) * sz;
    best = fminf(best, fmaf(d, d, gp[(size_t)k * C * plane]));
  }
  g3[(((size_t)side * B + z) * C + c) * plane + in_plane] = best;
}

// blockIdx.x = b * H + y (one image row), .y = class, .z = side whose distance map is read; the threads stand on the OTHER side's surface
__global__ __launch_bounds__(256) void hd_rows(const float* g, const uint8_t* surf, int B, int H, int W, int C, float sx, int method3d, unsigned* acc) {
  __shared__ __attribute__((aligned(16))) float row[HD_MAX_EXTENT];
  const int by = blockIdx.x, c = blockIdx.y, side = blockIdx.z;
  const int b = by / H, y = by - b * H;
  const uint8_t* sp = surf + (((size_t)(1 - side) * B + b) * H + y) * W;
  unsigned mine = 0;                      // bit k: pixel x = threadIdx.x + 256 k is a surface pixel of class c on the other side
  for (int k = 0; k < HD_MAX_EXTENT / 256; ++k) {
    const int x = threadIdx.x + 256 * k;
    if (x < W && sp[x] == c) mine |= 1u << k;
  }
  if (!__syncthreads_or((int)mine)) return;
  const float* gp = g + ((((size_t)side * B + b) * C + c) * H + y) * W;
  const int W4 = (W + 3) & ~3;
  for (int x = threadIdx.x; x < W4; x += 256) row[x] = x < W ? gp[x] : INFINITY;
  __syncthreads();
  float worst = 0.f;                      // (a wave without a surface pixel falls through both loops)
  for (int k = 0; k < HD_MAX_EXTENT / 256; ++k) {
    if (!(mine >> k & 1)) continue;
    float df = (float)(threadIdx.x + 256 * k);       // x - x', an exact integer all the way down
    float best = INFINITY;
    for (int x4 = 0; x4 < W4; x4 += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + x4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = df * sx;
        best = fminf(best, fmaf(d, d, v[j]));
        df -= 1.f;
      }
    }
    worst = fmaxf(worst, best);
  }
  unsigned bits = mine ? __float_as_uint(worst) + 1u : 0u;      // worst >= 0 (or +inf): ordered like its bit pattern
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)bits, off, 64);
    bits = o > bits ? o : bits;
  }
  // acc only grows: a wave whose maximum is not above what is there already has nothing to add.  (In 3-D all B * H rows of a class
  // meet in ONE word; without the look first the atomics of a million blocks queue up on C addresses.)
  if ((threadIdx.x & 63) == 0 && bits) {
    unsigned* word = acc + (method3d ? 0 : b) * C + c;
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(word, bits);
  }
}

__global__ __launch_bounds__(256) void hd_finish(const unsigned* acc, float* hd2, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned v = acc[i];
  hd2[i] = (v == 0u || v - 1u >= 0x7F800000u) ? __uint_as_float(0x7FC00000u) : __uint_as_float(v - 1u);
}

// B <= 65535 in 2-D: not a property of the kernels (their grids put B * H and B * W / 64 in grid.x) but a ceiling that keeps every such
// product and the rows * C accumulator count far inside 32 bits without a second set of checks; a loader batch is tens of slices.
inline int hd_shape_status(int B, int H, int W, int C, int method3d) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return DCT_ERR_BAD_ARG;
  if (C > 8 || H > HD_MAX_EXTENT || W > HD_MAX_EXTENT || (method3d && B > 256) || B > 65535) return DCT_ERR_UNSUPPORTED;
  return DCT_OK;
}

// ---- signed distance maps of the boundary loss (the rule: include/dct.h, dct_signed_distance) -------------------------------------------
// The same separable transform, dense and per class.  A pixel belongs to exactly one of C + 1 sets: the C classes and "none" (a target
// outside [0, C)), so the pixels NOT in class c are the union of the other C sets, and the distance to the nearest of them is the minimum
// of the distances to those sets.  One to-set map per set therefore carries both sides of every class:
//   outside G_c:  d2 = best[c];      inside G_c:  d2 = min_{c' != c} best[c']      (best[c'] = min_x' (sx (x - x'))^2 + g[c'][x'])
// and that minimum is bit for bit the row pass over the column map of "not c" (which is min_{c' != c} g[c']): fma(d, d, .) is monotone
// in its addend and a minimum does not round.  C + 1 column maps and row scans instead of 2 C, and no select in the inner loop.
// Launch chain (the caller's stream, everything between the launches in the caller's workspace):
//   1. sd_classify   targets -> one class byte per pixel (255 = none); clears the per-(image, set) pixel counters
//   2. sd_columns    hd_columns with the predicate on the class byte, for the C + 1 sets; a thread counts its column's pixels of the set on
//                    the way down and a wave adds its sum to cnt[b][set] with ONE integer atomic (integers: the same counts every run)
//   3. sd_rows       a block owns one image row and holds the row of all C + 1 column maps in LDS; a thread scans the full row for all sets
//                    at once (every LDS read is a 16-byte broadcast of four x'; d = (x - x') sx is formed once per x' for all sets), then
//                    takes the root, the sign and the - 1 (inside: in fp64, rounded once), applies the zero rule from the counters and stores its pixel's C values together.
// The row scan is not bounded by the running minimum: the bound differs from lane to lane and a wave runs as long as its slowest lane.
struct SdWs { size_t cnt, cls, g, total; };
inline SdWs sd_layout(int B, int H, int W, int C) {
  const size_t px = (size_t)B * H * W;
  SdWs w;
  w.cnt = 0;
  w.cls = hd_round((size_t)B * (C + 1) * 4);
  w.g = w.cls + hd_round(px);
  w.total = w.g + hd_round(px * (C + 1) * 4);
  return w;
}

// four pixels per thread: 16-byte target loads, one 4-byte class store (cls is 256-byte aligned in the workspace)
__global__ __launch_bounds__(256) void sd_classify(const long long* gt, long long px, int C, uint8_t* cls, unsigned* cnt, int ncnt) {
  if (blockIdx.x == 0) for (int i = threadIdx.x; i < ncnt; i += 256) cnt[i] = 0u;
  for (long long q = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; q < px; q += (long long)gridDim.x * 1024) {
    if (q + 4 <= px) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      const i64x2 t0 = *reinterpret_cast<const i64x2*>(gt + q), t1 = *reinterpret_cast<const i64x2*>(gt + q + 2);
      *reinterpret_cast<unsigned*>(cls + q) = hd_gt_class(t0[0], C) | hd_gt_class(t0[1], C) << 8 | hd_gt_class(t1[0], C) << 16 | hd_gt_class(t1[1], C) << 24;
    } else {
      for (long long i = q; i < px; ++i) cls[i] = (uint8_t)hd_gt_class(gt[i], C);
    }
  }
}

// One thread per (b, set, column); blockIdx.y = set, C = "none".  g[b][set][y][x] = (sy (y - y'))^2 to the nearest pixel y' of the set in
// column x, +inf where the column has none.
// (__restrict__: the class bytes and the map do not overlap, so the unrolled scans may take their loads ahead of the stores between them
// instead of one memory round trip per row)
__global__ __launch_bounds__(64) void sd_columns(const uint8_t* __restrict__ cls, float* __restrict__ g, unsigned* cnt, int B, int H, int W, int C, float sy) {
  const int xchunks = (W + 63) / 64;
  const int b = blockIdx.x / xchunks, x = (blockIdx.x - b * xchunks) * 64 + threadIdx.x, set = blockIdx.y;
  const unsigned key = set == C ? HD_NONE : set;
  int n = 0;
  if (x < W) {
    const uint8_t* __restrict__ sp = cls + (size_t)b * H * W + x;
    float* __restrict__ gp = g + ((size_t)b * (C + 1) + set) * H * W + x;
    float run = INFINITY;
#pragma unroll 16
    for (int y = 0; y < H; ++y) {
      const bool hit = sp[(size_t)y * W] == key;
      n += hit;
      run = hit ? 0.f : run + 1.f;
      const float t = run * sy;
      gp[(size_t)y * W] = t * t;
    }
    run = INFINITY;
    for (int y0 = H - 1; y0 >= 0; y0 -= 16) {   // sixteen rows a trip: their loads first (a store to gp in between would hold the next load back)
      unsigned k[16];
      float down[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int y = y0 - j;
        if (y >= 0) { k[j] = sp[(size_t)y * W]; down[j] = gp[(size_t)y * W]; }
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int y = y0 - j;
        if (y >= 0) {
          run = k[j] == key ? 0.f : run + 1.f;
          const float t = run * sy;
          gp[(size_t)y * W] = fminf(down[j], t * t);
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if (threadIdx.x == 0 && n) atomicAdd(cnt + b * (C + 1) + set, (unsigned)n);
}

// blockIdx.x = b * H + y; dynamic LDS: (C + 1) rows of W rounded up to 4 floats (the pad holds +inf)
template <int C>
__global__ __launch_bounds__(256) void sd_rows(const float* g, const uint8_t* cls, const unsigned* cnt, int H, int W, float sx, int class_mask,
                                               float* phi) {
  extern __shared__ __attribute__((aligned(16))) float sd_row[];
  constexpr int CP = C + 1;
  const int b = blockIdx.x / H, y = blockIdx.x - b * H;
  const int W4 = (W + 3) & ~3;
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float* gp = g + ((size_t)b * CP + c) * plane + (size_t)y * W;
    for (int x = threadIdx.x; x < W4; x += 256) sd_row[c * W4 + x] = x < W ? gp[x] : INFINITY;
  }
  unsigned live = 0;                      // bit c: class c is in the mask and has a contour in this image (neither absent nor filling it)
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const unsigned n = cnt[b * CP + c];
    if ((class_mask >> c & 1) && n != 0u && n != (unsigned)(H * W)) live |= 1u << c;
  }
  __syncthreads();
  const uint8_t* cp = cls + ((size_t)b * H + y) * W;
  float* out = phi + ((size_t)b * H + y) * W * C;
  for (int x = threadIdx.x; x < W; x += 256) {
    float best[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) best[c] = INFINITY;
    float df = (float)x;                  // x - x', an exact integer all the way down
    for (int x4 = 0; x4 < W4; x4 += 4) {
      float d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { d[j] = df * sx; df -= 1.f; }
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(sd_row + c * W4 + x4);
#pragma unroll
        for (int j = 0; j < 4; ++j) best[c] = fminf(best[c], fmaf(d[j], d[j], v[j]));
      }
    }
    const unsigned t = cp[x];
    float other = INFINITY;               // the nearest pixel that is not in the pixel's own set
#pragma unroll
    for (int c = 0; c < CP; ++c) other = fminf(other, t == (c == C ? (unsigned)HD_NONE : (unsigned)c) ? INFINITY : best[c]);
    // Inside, the root and the "- 1" are taken in fp64 and rounded to fp32 ONCE: 1.f - sqrtf(d2) rounds the root at the root's magnitude
    // and lands up to an ulp of the smaller difference away from the rounded exact value (seen on the device against float64: 1 - sqrt(2)).
    // One fp64 root per pixel, beside a row scan of W x (C + 1) candidates.
    const float inside = (float)(1.0 - sqrt((double)other));
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float s = t == (unsigned)c ? inside : sqrtf(best[c]);
      v[c] = (live >> c & 1) ? s : 0.f;
    }
    float* o = out + (size_t)x * C;
    if constexpr (C == 4) *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    else if constexpr (C == 8) {
      *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else if constexpr (C == 2) *reinterpret_cast<f32x2*>(o) = f32x2{v[0], v[1]};
    else {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = v[c];
    }
  }
}

inline int sd_shape_status(int B, int H, int W, int C) {
  if (B < 1 || H < 1 || W < 1) return DCT_ERR_BAD_ARG;
  if (C < 2 || C > 8 || H > HD_MAX_EXTENT || W > HD_MAX_EXTENT || B > 65535) return DCT_ERR_UNSUPPORTED;
  return DCT_OK;
}

}  // namespace

extern "C" size_t dct_signed_distance_workspace_bytes(int B, int H, int W, int C) {
  if (sd_shape_status(B, H, W, C) != DCT_OK) return 0;
  return sd_layout(B, H, W, C).total;
}

extern "C" int dct_signed_distance(const int64_t* targets, int B, int H, int W, int C_, int class_mask, float sy, float sx, float* phi,
                                   void* workspace, size_t workspace_bytes, dct_stream stream) {
  if (!targets || !phi || !workspace) return DCT_ERR_BAD_ARG;
  if (!(sy > 0.f) || !(sx > 0.f) || __builtin_isinf(sy) || __builtin_isinf(sx)) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)targets | (uintptr_t)phi | (uintptr_t)workspace) & 15) return DCT_ERR_BAD_ARG;
  const int shape = sd_shape_status(B, H, W, C_);
  if (shape != DCT_OK) return shape;
  if (!(class_mask & ((1 << C_) - 1))) return DCT_ERR_BAD_ARG;
  const SdWs w = sd_layout(B, H, W, C_);
  if (workspace_bytes < w.total) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned* cnt = (unsigned*)(ws + w.cnt);
  uint8_t* cls = (uint8_t*)(ws + w.cls);
  float* g = (float*)(ws + w.g);
  const long long px = (long long)B * H * W;
  long long blocks = (px + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  DCT_LAUNCH(DCT_PROF_LOSS, sd_classify, dim3((unsigned)blocks), dim3(256), 0, st, (const long long*)targets, px, C_, cls, cnt, B * (C_ + 1));
  DCT_LAUNCH(DCT_PROF_LOSS, sd_columns, dim3((unsigned)(B * ((W + 63) / 64)), (unsigned)(C_ + 1)), dim3(64), 0, st, (const uint8_t*)cls, g, cnt, B, H, W, C_, sy);
  const size_t lds = (size_t)(C_ + 1) * ((W + 3) & ~3) * sizeof(float);
#define SD_ROWS(Cv) case Cv: DCT_LAUNCH(DCT_PROF_LOSS, sd_rows<Cv>, dim3((unsigned)(B * H)), dim3(256), lds, st, (const float*)g, (const uint8_t*)cls, \
                                        (const unsigned*)cnt, H, W, sx, class_mask, phi); break;
  switch (C_) { SD_ROWS(2) SD_ROWS(3) SD_ROWS(4) SD_ROWS(5) SD_ROWS(6) SD_ROWS(7) SD_ROWS(8) }
#undef SD_ROWS
  return dct_check_launch();
}

extern "C" size_t dct_hausdorff_workspace_bytes(int B, int H, int W, int C, int method3d) {
  if (hd_shape_status(B, H, W, C, method3d) != DCT_OK) return 0;
  return hd_layout(B, H, W, C, method3d).total;
}

#define HD_DISPATCH_C(Cv, ...)                                       \
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

extern "C" int dct_hausdorff(const float* logits, const int64_t* gt, int B, int H, int W, int C_, int method3d, float sz, float sy, float sx,
                             float* hd2, void* workspace, size_t workspace_bytes, dct_stream stream) {
  if (!logits || !gt || !hd2 || !workspace) return DCT_ERR_BAD_ARG;
  if (!(sz > 0.f) || !(sy > 0.f) || !(sx > 0.f)) return DCT_ERR_BAD_ARG;
  if (((uintptr_t)logits | (uintptr_t)gt | (uintptr_t)workspace) & 15) return DCT_ERR_BAD_ARG;
  const int shape = hd_shape_status(B, H, W, C_, method3d);
  if (shape != DCT_OK) return shape;
  const HdWs w = hd_layout(B, H, W, C_, method3d);
  if (workspace_bytes < w.total) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned* acc = (unsigned*)(ws + w.acc);
  uint8_t* cls = (uint8_t*)(ws + w.pcls);
  uint8_t* surf = (uint8_t*)(ws + w.surf);
  float* g = (float*)(ws + w.g);
  float* g3 = (float*)(ws + w.g3);
  const long long px = (long long)B * H * W;
  const int rows = method3d ? 1 : B;
  long long blocks = (px + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  HD_DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, hd_classify<C>, dim3((unsigned)blocks), dim3(256), 0, st, logits, (const long long*)gt, px, cls, acc, rows * C_));
  blocks = (2 * px + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  DCT_LAUNCH(DCT_PROF_LOSS, hd_surface, dim3((unsigned)blocks), dim3(256), 0, st, (const uint8_t*)cls, surf, B, H, W, method3d);
  DCT_LAUNCH(DCT_PROF_LOSS, hd_columns, dim3((unsigned)(B * ((W + 63) / 64)), (unsigned)C_, 2), dim3(64), 0, st, (const uint8_t*)surf, g, B, H, W, C_, sy);
  if (method3d) {
    DCT_LAUNCH(DCT_PROF_LOSS, hd_slices, dim3((unsigned)(B * H * ((W + 255) / 256)), (unsigned)C_, 2), dim3(256), 0, st, (const float*)g, g3, B, H, W, C_, sz);
  }
  DCT_LAUNCH(DCT_PROF_LOSS, hd_rows, dim3((unsigned)(B * H), (unsigned)C_, 2), dim3(256), 0, st, (const float*)(method3d ? g3 : g), (const uint8_t*)surf, B, H, W, C_, sx,
             method3d, acc);
  DCT_LAUNCH(DCT_PROF_LOSS, hd_finish, dim3(div_up(rows * C_, 256)), dim3(256), 0, st, (const unsigned*)acc, hd2, rows * C_);
  return dct_check_launch();
}
