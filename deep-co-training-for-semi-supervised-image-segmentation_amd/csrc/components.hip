// Largest connected component of every class of an argmax map: what every ACDC-style pipeline applies to a prediction before it
// scores it (scipy.ndimage.label per slice and class on the host), here on the device in front of the meters.
//
//   class of a pixel = argmax of its logits (first maximum, as dct_argmax / dct_dice_counts / dct_hausdorff)
//   row              = one slice (2-D) or the whole batch as a volume, z = batch index (method3d)
//   neighbours       = full 0: the 4 / 6 that share a face; full 1: the 8 / 26 that share a face, an edge or a corner
//   component        = maximal connected set of pixels of one class inside one row
//   kept             = per (row, class in class_mask) the component with the most pixels; ties: the one whose first pixel in raster
//                      order comes first.  Every other pixel of the class becomes `background`.
//
// Labels are 32-bit pixel indices inside the row.  The label pass is union-find over label equivalences (Komura 2015;
// Playne & Hawick 2018) in ONE launch: no host loop, no "changed" flag (components_uf.h holds the routines, why they terminate and why
// the root of a component is its first pixel in raster order whatever order the atomics land in).
//
// Launch chain (all on the caller's stream, everything between them lives in the caller's workspace; bytes per pixel in brackets):
//   1. cc_classify  one read of the logits (argmax in registers) -> one class byte; parent = first pixel of the pixel's run of equal
//                   classes inside its 64-pixel wave segment (a ballot: no atomics, no chain longer than a hop); size = 0; also clears
//                   the per-(row, class) words                                                          [reads 4 C, writes 1 + 4 + 4]
//   2. cc_merge     every pixel unites itself with its already-visited neighbours of the same class (left across a segment border, up,
//                   the two upper diagonals with full, slice z - 1 in a volume), leaving out the pairs that are connected through
//                   others: inside a blob only the first pixel of each segment-run touches parent[] at all.   [reads ~3-6 class bytes
//                   (cache), + 4 per hop of a find, one atomic per union that changes something]
//   3. cc_count     every pixel finds its root and stores it in parent (the forest no longer changes); size[root] += 1, combined twice
//                   before it reaches memory: runs of equal roots along the wave by a ballot, then the runs of a block's 2048 pixels
//                   in an LDS table keyed by the root -- one global atomic per (block, root)                [reads 4 per hop, writes 4]
//   4. cc_select    every root: best[row][class] = max( size << 32 | ~root ) by 64-bit atomic max -- the largest size wins, ties go to
//                   the lowest root; pixels[row][class] += size, components += 1; a block combines the roots of its 2048 pixels in
//                   LDS first, and a look before the max keeps the losers away                            [reads 4, + 1 + 4 per root]
//   5. cc_apply     a pixel keeps its class when the class is outside class_mask or its root is the winner, else it becomes
//                   background -> onehot, cls; the first rows * C threads write stats                [reads 1 + 4, writes 4 C + 8]
// Integer sums, a maximum and a minimum: nothing depends on the order of the atomics, the outputs are bit-identical from run to run.
#include "dct_common.h"
#include "components_uf.h"

namespace {

struct CcWs {               // byte offsets into the workspace
  size_t best, ncomp, npix, cls, parent, size, total;
};
inline size_t cc_round(size_t v) { return (v + 255) & ~(size_t)255; }
inline CcWs cc_layout(int B, int H, int W, int C, int method3d) {
  const size_t px = (size_t)B * H * W, words = (size_t)(method3d ? 1 : B) * C;
  CcWs w;
  w.best = 0;
  w.ncomp = cc_round(words * 8);
  w.npix = w.ncomp + cc_round(words * 4);
  w.cls = w.npix + cc_round(words * 4);
  w.parent = w.cls + cc_round(px);
  w.size = w.parent + cc_round(px * 4);
  w.total = w.size + cc_round(px * 4);
  return w;
}

template <int C> __device__ __forceinline__ int cc_argmax(const float* p) {
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

// parent[] on the device: loads that go to the coherent level every time, 32-bit vector atomics
struct CcParent {
  int* p;
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int min(int i, int v) const { return atomicMin(p + i, v); }
};

// Every kernel below walks the pixels as blocks of 256 consecutive ones, a lane per pixel: lane = pixel index & 63, so that the "64-pixel
// segment" of a pixel is the same in all of them.  The loops are uniform over the block (ballots need every lane).
#define CC_FOR_PIXELS(p, px) for (long long base_ = (long long)blockIdx.x * 256, p = base_ + threadIdx.x; base_ < (px); base_ += (long long)gridDim.x * 256, p = base_ + threadIdx.x)

template <int C>
__global__ __launch_bounds__(256) void cc_classify(const float* logits, long long px, int rowpx, int W, uint8_t* cls, int* parent, int* size,
                                                   unsigned long long* best, int* ncomp, int* npix, int words) {
  if (blockIdx.x == 0) for (int i = threadIdx.x; i < words; i += 256) { best[i] = 0ull; ncomp[i] = 0; npix[i] = 0; }
  const int lane = threadIdx.x & 63;
  CC_FOR_PIXELS(p, px) {
    const bool valid = p < px;
    int c = 255;
    if (valid) c = cc_argmax<C>(logits + p * C);
    const int left = __shfl_up(c, 1, 64);
    const int l = valid ? (int)(p % rowpx) : 0;
    const bool start = lane == 0 || l % W == 0 || left != c;
    const unsigned long long starts = __ballot(start);
    if (valid) {
      const int first = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));      // the last start at or below this lane
      cls[p] = (uint8_t)c;
      parent[p] = l - (lane - first);
      size[p] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void cc_merge(const uint8_t* cls, int* parent, long long px, int rowpx, int H, int W, int full, int method3d) {
  CC_FOR_PIXELS(p, px) {
    if (p >= px) continue;
    const long long rowbase = p - p % rowpx;
    const int l = (int)(p - rowbase), x = l % W, y = (l / W) % H, z = l / (W * H);
    CcParent a{parent + rowbase};
    cc_merge_pixel(a, cls + rowbase, l, x, y, z, H, W, full, method3d, (threadIdx.x & 63) == 0);
  }
}

// A block owns CC_CHUNK consecutive pixels and collects its adds to size[] in an LDS table keyed by the root (open addressing, a bounded
// number of probes; an add that finds no slot goes to global memory directly), then sends one add per root it met: a blob that covers
// thousands of the chunk's pixels costs one global atomic per chunk, not one per pixel or per run.
#define CC_CHUNK 2048
#define CC_SLOTS 1024
#define CC_PROBES 8

__global__ __launch_bounds__(256) void cc_count(int* parent, int* size, long long px, int rowpx) {
  __shared__ unsigned long long slot_root[CC_SLOTS];
  __shared__ int slot_count[CC_SLOTS];
  const int lane = threadIdx.x & 63;
  const unsigned long long kEmpty = ~0ull;
  for (long long chunk = (long long)blockIdx.x * CC_CHUNK; chunk < px; chunk += (long long)gridDim.x * CC_CHUNK) {
    for (int i = threadIdx.x; i < CC_SLOTS; i += 256) { slot_root[i] = kEmpty; slot_count[i] = 0; }
    __syncthreads();
    for (int it = 0; it < CC_CHUNK / 256; ++it) {
      const long long p = chunk + it * 256 + threadIdx.x;
      const bool valid = p < px;
      long long groot = -1;           // root as an index into the whole array: equal in two lanes <=> same row and same root
      if (valid) {
        const long long rowbase = p - p % rowpx;
        const int l = (int)(p - rowbase);
        CcParent a{parent + rowbase};
        const int r = cc_find(a, l);
        // the forest is final: a pixel may point at its root directly (a reader meets the old parent or the root, both on its way)
        if (r != l) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        groot = rowbase + r;
      }
      // one add per run of equal roots along the wave
      const long long prev = __shfl_up(groot, 1, 64);
      const bool head = lane == 0 || prev != groot;
      const unsigned long long heads = __ballot(head);
      if (valid && head) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = above ? __ffsll((long long)above) : 64 - lane;
        unsigned h = ((unsigned)groot * 0x9E3779B1u) >> 22;          // 10 bits: CC_SLOTS
        bool placed = false;
        for (int probe = 0; probe < CC_PROBES && !placed; ++probe) {
          const unsigned long long was = atomicCAS(&slot_root[h], kEmpty, (unsigned long long)groot);
          if (was == kEmpty || was == (unsigned long long)groot) {
            atomicAdd(&slot_count[h], len);
            placed = true;
          } else {
            h = (h + 1) & (CC_SLOTS - 1);
          }
        }
        if (!placed) atomicAdd(size + groot, len);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_SLOTS; i += 256)
      if (slot_root[i] != kEmpty) atomicAdd(size + slot_root[i], slot_count[i]);
    __syncthreads();
  }
}

// Roots only.  The (row, class) words of all rows lie in a few cache lines: every atomic on them queues in one place.  A block therefore
// owns CC_CHUNK consecutive pixels, collects what their roots have to say in LDS -- the words a chunk can touch are consecutive, so the
// slot is the word's offset from the chunk's first one -- and sends one add of sizes, one add of the number and one 64-bit max per word;
// a look before the max keeps a maximum that cannot win away from memory.  (A chunk over more than CC_WORDS words -- tiny images --
// sends the rest directly.)
#define CC_WORDS 64

__global__ __launch_bounds__(256) void cc_select(const uint8_t* cls, const int* parent, const int* size, unsigned long long* best, int* ncomp,
                                                 int* npix, long long px, int rowpx, int C) {
  __shared__ int s_pix[CC_WORDS], s_cnt[CC_WORDS];
  __shared__ unsigned long long s_best[CC_WORDS];
  for (long long chunk = (long long)blockIdx.x * CC_CHUNK; chunk < px; chunk += (long long)gridDim.x * CC_CHUNK) {
    const int k0 = (int)(chunk / rowpx) * C;
    if (threadIdx.x < CC_WORDS) { s_pix[threadIdx.x] = 0; s_cnt[threadIdx.x] = 0; s_best[threadIdx.x] = 0ull; }
    __syncthreads();
    for (int it = 0; it < CC_CHUNK / 256; ++it) {
      const long long p = chunk + it * 256 + threadIdx.x;
      if (p >= px) continue;
      const int l = (int)(p % rowpx);
      if (parent[p] != l) continue;
      const int k = (int)(p / rowpx) * C + cls[p], sz = size[p], slot = k - k0;
      const unsigned long long v = (unsigned long long)(unsigned)sz << 32 | (unsigned)~(unsigned)l;
      if (slot < CC_WORDS) {
        atomicAdd(&s_pix[slot], sz);
        atomicAdd(&s_cnt[slot], 1);
        atomicMax(&s_best[slot], v);
      } else {
        atomicAdd(npix + k, sz);
        atomicAdd(ncomp + k, 1);
        atomicMax(best + k, v);
      }
    }
    __syncthreads();
    if (threadIdx.x < CC_WORDS && s_cnt[threadIdx.x]) {
      const int k = k0 + threadIdx.x;
      atomicAdd(npix + k, s_pix[threadIdx.x]);
      atomicAdd(ncomp + k, s_cnt[threadIdx.x]);
      if (__hip_atomic_load(best + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < s_best[threadIdx.x]) atomicMax(best + k, s_best[threadIdx.x]);
    }
    __syncthreads();
  }
}

template <int C>
__global__ __launch_bounds__(256) void cc_apply(const uint8_t* cls, const int* parent, const unsigned long long* best, const int* ncomp,
                                                const int* npix, long long px, int rowpx, unsigned class_mask, int background, float* onehot,
                                                long long* out_cls, int* stats, int words) {
  if (stats) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) {       // (H * W may be smaller than C)
      stats[3 * i] = ncomp[i];
      stats[3 * i + 1] = (int)(best[i] >> 32);
      stats[3 * i + 2] = npix[i];
    }
  }
  CC_FOR_PIXELS(p, px) {
    if (p >= px) continue;
    int c = cls[p];
    if (class_mask >> c & 1u) {
      const unsigned winner = ~(unsigned)best[(p / rowpx) * C + c];
      if ((unsigned)parent[p] != winner) c = background;
    }
    if (out_cls) out_cls[p] = c;
    if (onehot) {
      float* o = onehot + p * C;
      if constexpr (C == 4) {
        const f32x4 v = {c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f, c == 3 ? 1.f : 0.f};
        *reinterpret_cast<f32x4*>(o) = v;
      } else if constexpr (C == 8) {
        const f32x4 v = {c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f, c == 3 ? 1.f : 0.f};
        const f32x4 u = {c == 4 ? 1.f : 0.f, c == 5 ? 1.f : 0.f, c == 6 ? 1.f : 0.f, c == 7 ? 1.f : 0.f};
        *reinterpret_cast<f32x4*>(o) = v;
        *reinterpret_cast<f32x4*>(o + 4) = u;
      } else if constexpr (C == 2) {
        const f32x2 v = {c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f};
        *reinterpret_cast<f32x2*>(o) = v;
      } else {
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = c == k ? 1.f : 0.f;
      }
    }
  }
}

// A row below 2^31 pixels: labels, sizes and the per-(row, class) counts are 32-bit.  rows * C stays far inside 32 bits too: B < 2^27.
inline int cc_shape_status(int B, int H, int W, int C, int method3d) {
  if (B < 1 || H < 1 || W < 1 || C < 1) return DCT_ERR_BAD_ARG;
  const long long rowpx = (long long)H * W * (method3d ? B : 1);
  if (C > 8 || (long long)H * W >= (1ll << 31) || rowpx >= (1ll << 31) || B >= (1 << 27)) return DCT_ERR_UNSUPPORTED;
  return DCT_OK;
}

}  // namespace

extern "C" size_t dct_components_workspace_bytes(int B, int H, int W, int C, int method3d) {
  if (cc_shape_status(B, H, W, C, method3d) != DCT_OK) return 0;
  return cc_layout(B, H, W, C, method3d).total;
}

#define CC_DISPATCH_C(Cv, ...)                                       \
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

extern "C" int dct_largest_component(const float* logits, int B, int H, int W, int C_, int method3d, int full, uint32_t class_mask,
                                     int background, float* onehot, int64_t* out_cls, int32_t* stats, void* workspace, size_t workspace_bytes,
                                     dct_stream stream) {
  if (!logits || (!onehot && !out_cls) || !workspace) return DCT_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || C_ < 1 || (full != 0 && full != 1)) return DCT_ERR_BAD_ARG;
  if (C_ > 8) return DCT_ERR_UNSUPPORTED;
  if (background < 0 || background >= C_ || (class_mask >> background & 1u) || (class_mask >> C_) != 0u) return DCT_ERR_BAD_ARG;
  if ((((uintptr_t)logits | (uintptr_t)onehot | (uintptr_t)workspace) & 15) || ((uintptr_t)out_cls & 7) || ((uintptr_t)stats & 3)) return DCT_ERR_BAD_ARG;
  const int shape = cc_shape_status(B, H, W, C_, method3d);
  if (shape != DCT_OK) return shape;
  const CcWs w = cc_layout(B, H, W, C_, method3d);
  if (workspace_bytes < w.total) return DCT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned long long* best = (unsigned long long*)(ws + w.best);
  int* ncomp = (int*)(ws + w.ncomp);
  int* npix = (int*)(ws + w.npix);
  uint8_t* cls = (uint8_t*)(ws + w.cls);
  int* parent = (int*)(ws + w.parent);
  int* size = (int*)(ws + w.size);
  const long long px = (long long)B * H * W;
  const int rowpx = method3d ? (int)px : H * W;
  const int words = (method3d ? 1 : B) * C_;
  long long nb = (px + 255) / 256;
  if (nb > (1 << 20)) nb = 1 << 20;
  const dim3 grid((unsigned)nb), block(256);
  CC_DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, cc_classify<C>, grid, block, 0, st, logits, px, rowpx, W, cls, parent, size, best, ncomp, npix, words));
  DCT_LAUNCH(DCT_PROF_LOSS, cc_merge, grid, block, 0, st, (const uint8_t*)cls, parent, px, rowpx, H, W, full, method3d ? 1 : 0);
  long long chunks = (px + CC_CHUNK - 1) / CC_CHUNK;
  if (chunks > (1 << 20)) chunks = 1 << 20;
  DCT_LAUNCH(DCT_PROF_LOSS, cc_count, dim3((unsigned)chunks), block, 0, st, parent, size, px, rowpx);
  DCT_LAUNCH(DCT_PROF_LOSS, cc_select, dim3((unsigned)chunks), block, 0, st, (const uint8_t*)cls, (const int*)parent, (const int*)size, best, ncomp, npix, px, rowpx, C_);
  CC_DISPATCH_C(C_, DCT_LAUNCH(DCT_PROF_LOSS, cc_apply<C>, grid, block, 0, st, (const uint8_t*)cls, (const int*)parent, (const unsigned long long*)best,
                               (const int*)ncomp, (const int*)npix, px, rowpx, class_mask, background, onehot, (long long*)out_cls, (int*)stats, words));
  return dct_check_launch();
}
