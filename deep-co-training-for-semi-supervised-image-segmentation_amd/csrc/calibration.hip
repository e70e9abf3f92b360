// Calibration tables of the raters of a batch (the counts behind ECE / MCE, the reliability diagram and the coverage-accuracy curve,
// and the sums behind the Brier score and the negative log-likelihood): ONE pass over the S probability (or logit) tensors and gt
// leaves bins[b][r][k][3] and scores[b][r][2] for the S views and, on request, their mean (rule: include/dct.h).  HBM-bound by
// design: (4 C S + 8) bytes per pixel.  The first metric kernel here that uses the VALUES of the probabilities, not only their argmax.
//
// Shape of confusion_kernel: a block owns a stretch of one image's pixels and a table of R * n_bins * 3 + R * 2 64-bit cells in LDS
// (at most 9 * 32 * 3 + 18 cells, 7056 bytes).  The contention finding of confusion.hip holds more strongly here: on a real map nearly
// every lane of a wave lands in the top bin, and 64 lanes adding to one LDS address serialise.  So the wave aggregates first: per
// rater, take the bin of the first lane that still has one, ballot the lanes that share it, popcount that ballot (pixels) and the
// ballot of the correct ones among them, sum their confidence words with a masked wave sum (64 words of at most 2^24 fit 32 bits),
// one lane adds the three numbers, those lanes retire.  One or two trips per rater on real maps, at most min(64, n_bins) on noise.
// The Brier and NLL words have one cell per rater: every lane keeps them in registers across its pixels, and the wave reduces them
// once, after the pixel loop.  Everything that leaves the block is an integer: the sums do not depend on their order, the result is
// bit-identical from run to run.
#include "calibration_common.h"      // CbPack, cb_load, cb_softmax, CB_DISPATCH_C: shared with temperature.hip

namespace {

constexpr int CB_MAXBINS = 32;
constexpr float CB_Q = 16777216.0f;                         // 2^24: the fixed-point unit of the confidence, Brier and NLL words

// Sum of v over the 64 lanes of a wave that is wholly active, the same value in every lane.  DPP adds in the vector ALU: a scan
// inside each row of 16 (row_shr 1, 2, 4, 8, zero fill), then lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast:15) and lane 31 into
// rows 2 and 3 (row_bcast:31); lane 63 holds the total.  The same six steps as __shfl_xor go through ds_bpermute_b32, one LDS-pipe
// round trip each on a dependent chain: measured 72.9 against 44.0 us on noise at 8 x 256 x 256 (calibration_kernel).
__device__ __forceinline__ unsigned cb_wave_sum(unsigned v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);      // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);      // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);      // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);      // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, true);      // row_bcast:15 into rows 1 and 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, true);      // row_bcast:31 into rows 2 and 3
  return (unsigned)__builtin_amdgcn_readlane(x, 63);
}

// What one rater says about one counted pixel of class t.  The class loops select, they do not index: p[t] would be a runtime index
// and the array would live in scratch memory.  The bin is clamped from below as well: the rule expects probabilities, but a
// negative or NaN input must not index outside the table.
template <int C>
__device__ __forceinline__ void cb_pixel(const float p[C], int t, int n_bins, int& bin, bool& correct, unsigned& confq, unsigned& brierq,
                                         unsigned& nllq) {
  int best = 0;                             // first maximum, as dct_argmax and confusion_kernel
  float top = p[0];
#pragma unroll
  for (int c = 1; c < C; ++c) if (p[c] > top) { top = p[c]; best = c; }
  float brier = 0.f, pg = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const bool is = c == t;
    const float d = p[c] - (is ? 1.f : 0.f);
    brier += d * d;
    if (is) pg = p[c];
  }
  const int k = (int)(top * (float)n_bins);
  bin = k < 0 ? 0 : (k > n_bins - 1 ? n_bins - 1 : k);
  correct = best == t;
  confq = (unsigned)(top * CB_Q);
  brierq = (unsigned)(brier * CB_Q);                    // <= 2 * 2^24, and nll <= -log(1e-10) = 23.03: both words fit 32 bits, and
  nllq = (unsigned)(-logf(pg + 1e-10f) * CB_Q);        // one v_cvt_u32_f32 replaces the long sequence behind a cast to int64
}

// grid = (blocks, B); every wave runs the same number of trips of the pixel loop (a lane past the image's end, or on a pixel that does
// not count, is merely idle in the ballots), so the ballots below see whole waves.  NS = 2, 4 or 8 >= S: the loads of a pixel are
// issued together, without a branch between them; the slots from S on read view 0 again (a cache hit) and are not looked at.
// Register slot NS is the mean of the views; in the tables it is rater S.
template <int C, int NS, bool LOGITS>
__global__ __launch_bounds__(256) void calibration_kernel(CbPack pk, int S, int ens, const long long* gt, long long PPI, unsigned class_mask,
                                                          int n_bins, unsigned long long* bins, unsigned long long* scores) {
  __shared__ unsigned long long h[CB_MAXR * CB_MAXBINS * 3];
  __shared__ unsigned long long hs[CB_MAXR * 2];
  const int R = S + (ens ? 1 : 0), cells = R * n_bins * 3;
  for (int i = threadIdx.x; i < cells; i += 256) h[i] = 0;
  if (threadIdx.x < R * 2) hs[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const long long img = (long long)b * PPI;
  long long sbrier[NS + 1], snll[NS + 1];
#pragma unroll
  for (int s = 0; s <= NS; ++s) { sbrier[s] = 0; snll[s] = 0; }
  for (long long base = (long long)blockIdx.x * 256; base < PPI; base += (long long)gridDim.x * 256) {
    const long long pix = base + threadIdx.x;
    bool counted = false;
    int bin[NS + 1];
    bool ok[NS + 1];
    unsigned cq[NS + 1];
#pragma unroll
    for (int s = 0; s <= NS; ++s) { bin[s] = 0; ok[s] = false; cq[s] = 0; }
    if (pix < PPI) {
      float v[NS][C];
#pragma unroll
      for (int s = 0; s < NS; ++s) cb_load<C>((s < S ? pk.in[s] : pk.in[0]) + (img + pix) * C, v[s]);
      const long long g = gt[img + pix];
      counted = g >= 0 && g < C && ((class_mask >> (g & 31)) & 1u);
      if (counted) {
        const int t = (int)g;
        float e[C];
#pragma unroll
        for (int c = 0; c < C; ++c) e[c] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s < S) {                      // (uniform)
            unsigned bq, nq;
            if constexpr (LOGITS) cb_softmax<C>(v[s]);
            cb_pixel<C>(v[s], t, n_bins, bin[s], ok[s], cq[s], bq, nq);
            sbrier[s] += bq;
            snll[s] += nq;
#pragma unroll
            for (int c = 0; c < C; ++c) e[c] += v[s][c];        // in view order
          }
        }
        if (ens) {
          unsigned bq, nq;
          const float fs = (float)S;
#pragma unroll
          for (int c = 0; c < C; ++c) e[c] = e[c] / fs;         // a true division: exact when S is a power of two
          cb_pixel<C>(e, t, n_bins, bin[NS], ok[NS], cq[NS], bq, nq);
          sbrier[NS] += bq;
          snll[NS] += nq;
        }
      }
    }
#pragma unroll
    for (int s = 0; s <= NS; ++s) {
      if (s < NS ? s < S : ens != 0) {      // (uniform)
        unsigned long long* hp = h + (s < NS ? s : S) * n_bins * 3;
        bool todo = counted;
        for (;;) {
          const unsigned long long rem = __ballot(todo);
          if (!rem) break;
          const int first = __ffsll((long long)rem) - 1;
          const int fb = __builtin_amdgcn_readlane(bin[s], first);
          const bool mine = todo && bin[s] == fb;
          const unsigned long long same = __ballot(mine);
          const unsigned long long right = __ballot(mine && ok[s]);
          const unsigned w = cb_wave_sum(mine ? cq[s] : 0u);     // at most 64 * 2^24 = 2^30
          if (lane == first) {
            atomicAdd(hp + fb * 3, (unsigned long long)__popcll(same));
            if (right) atomicAdd(hp + fb * 3 + 1, (unsigned long long)__popcll(right));
            atomicAdd(hp + fb * 3 + 2, (unsigned long long)w);
          }
          todo = todo && bin[s] != fb;
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s <= NS; ++s) {
    if (s < NS ? s < S : ens != 0) {        // (uniform)
      long long a = sbrier[s], n = snll[s];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) { a += __shfl_xor(a, off); n += __shfl_xor(n, off); }
      if (lane == 0) {
        unsigned long long* sp = hs + (s < NS ? s : S) * 2;
        if (a) atomicAdd(sp, (unsigned long long)a);
        if (n) atomicAdd(sp + 1, (unsigned long long)n);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = bins + (long long)b * cells;
  for (int i = threadIdx.x; i < cells; i += 256) {
    const unsigned long long v = h[i];
    if (v) atomicAdd(out + i, v);
  }
  if (threadIdx.x < R * 2) {
    const unsigned long long v = hs[threadIdx.x];
    if (v) atomicAdd(scores + (long long)b * R * 2 + threadIdx.x, v);
  }
}

}  // namespace

extern "C" int dct_calibration_counts(const float* const* probs, int S, const int64_t* gt, int B, int64_t pixels_per_image, int C_,
                                      int n_bins, uint32_t class_mask, int with_ensemble, int from_logits, int64_t* bins,
                                      int64_t* scores, dct_stream stream) {
  if (!probs || !gt || !bins || !scores || S < 1 || B < 1 || pixels_per_image < 1) return DCT_ERR_BAD_ARG;
  if ((with_ensemble != 0 && with_ensemble != 1) || (from_logits != 0 && from_logits != 1)) return DCT_ERR_BAD_ARG;
  if (S > CB_MAXS || C_ < 1 || C_ > 8 || n_bins < 1 || n_bins > CB_MAXBINS || pixels_per_image >= (int64_t)1 << 31 || B > 65535)
    return DCT_ERR_UNSUPPORTED;
  const uintptr_t palign = C_ == 4 ? 15 : (C_ == 2 ? 7 : 3);      // the widest load of cb_load<C>
  CbPack pk;
  for (int s = 0; s < CB_MAXS; ++s) pk.in[s] = nullptr;
  for (int s = 0; s < S; ++s) {
    if (!probs[s] || ((uintptr_t)probs[s] & palign)) return DCT_ERR_BAD_ARG;
    pk.in[s] = probs[s];
  }
  if (((uintptr_t)gt & 7) || ((uintptr_t)bins & 7) || ((uintptr_t)scores & 7)) return DCT_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  long long bx = (pixels_per_image + 255) / 256;
  if (bx > 64) bx = 64;
#define CB_LAUNCH2(NS, LG) DCT_LAUNCH(DCT_PROF_LOSS, (calibration_kernel<C, NS, LG>), dim3((unsigned)bx, (unsigned)B), dim3(256), 0, st, pk, S, \
                                      with_ensemble, (const long long*)gt, (long long)pixels_per_image, (unsigned)class_mask, n_bins,             \
                                      (unsigned long long*)bins, (unsigned long long*)scores)
#define CB_LAUNCH(NS) do { if (from_logits) { CB_LAUNCH2(NS, true); } else { CB_LAUNCH2(NS, false); } } while (0)
  if (S <= 2) { CB_DISPATCH_C(C_, CB_LAUNCH(2)); }
  else if (S <= 4) { CB_DISPATCH_C(C_, CB_LAUNCH(4)); }
  else { CB_DISPATCH_C(C_, CB_LAUNCH(8)); }
#undef CB_LAUNCH
#undef CB_LAUNCH2
  return dct_check_launch();
}
