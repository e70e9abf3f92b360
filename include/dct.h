/* dct.h -- C ABI of the MI355X-native co-training step library (libdct_hip.so).
 *
 * Drop-in boundary: the reference has no FFI; its hot path is Python calling
 * third-party ATen ops.  This header declares one entry point per ATen op family the step
 * invokes; each comment cites the reference call site it replaces.
 * The Python host (package `dct_amd`) binds these with ctypes and puts them under the
 * reference's own object API (CoTrainer / Segmentator / loss modules / FSGMGenerator).
 *
 * Conventions
 *   - device pointers only; the library never allocates or frees device memory; workspaces are
 *     caller-provided (size from the matching *_workspace_bytes);
 *   - tensors are NHWC *views*: channel stride 1, element strides for n/h/w (so channel slices
 *     of a concat buffer and interior windows of padded buffers are plain views);
 *   - every launch goes to the hipStream_t passed in (void* here: no HIP headers needed);
 *   - return 0 on success, negative dct_status on failure; no exceptions cross the ABI;
 *   - the compute entry points keep no state between calls and are re-entrant from any thread.  The ONLY process-global
 *     mutable state is diagnostic: the A/B tuning knobs (dct_tune_set, defaults = the shipped configuration; read at
 *     launch time, so set them between launches from one thread) and the per-class event timing (dct_prof_enable /
 *     dct_prof_read).  SURVEY.md 8b sketched a `dct_init(device)` handle; it was dropped on purpose: every launch
 *     already names its device through the stream it is given and the pointers it receives, and nothing else (no
 *     allocation, no cached workspace, no per-device table) would live in such a handle.
 */
#ifndef DCT_H_
#define DCT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dct_status {
  DCT_OK = 0,
  DCT_ERR_BAD_ARG = -1,      /* null pointer, negative size, inconsistent shapes */
  DCT_ERR_UNSUPPORTED = -2,  /* shape/dtype outside what the kernels are built for */
  DCT_ERR_LAUNCH = -3,       /* hipGetLastError() != hipSuccess after a launch */
  DCT_ERR_WORKSPACE = -4     /* workspace too small */
} dct_status;

/* DCT_F16 (IEEE half, BASELINE configs[4] "fp16"): storage type of the Enet kernels' activations and activation gradients
 * (dct_enet_*), with fp32 raw conv outputs / statistics / parameters exactly as in bf16 mode.  Half's 5-bit exponent cannot
 * hold per-pixel loss gradients of a mean over ~1e6 pixels, so the host scales the loss gradients by a power of two (the
 * `gmul` argument of the loss backward kernels) and the optimizer divides it out (`grad_scale` of dct_adam_flat*): exact,
 * because a power-of-two factor commutes with every rounding on the way.  The MFMA UNet kernels take F32 / BF16 only. */
typedef enum dct_dtype { DCT_F32 = 0, DCT_BF16 = 1, DCT_F16 = 2 } dct_dtype;

/* NHWC strided view; strides in ELEMENTS of the view's dtype; channel stride is 1. */
typedef struct dct_view {
  void* ptr;
  int32_t n, h, w, c;
  int64_t sn, sh, sw;
} dct_view;

typedef void* dct_stream; /* hipStream_t */

/* ABI version: dct_version() of the loaded library returns the DCT_VERSION it was built with.  It goes up whenever a struct
 * or a signature below changes incompatibly (INTEGRATION.md lists the changes); a caller built against another value must not call on. */
#define DCT_VERSION 101
int dct_version(void);
const char* dct_status_string(int status);

/* ---- K1/K2/K3: convolutions as implicit GEMM on MFMA -----------------------------------
 * Replaces F.conv2d / F.conv_transpose2d behind nn.Conv2d / nn.ConvTranspose2d
 * (arch/network.py:120-223, arch/enet.py:21-122) and their autograd backward.
 *
 * y[n,oy,ox,co] = epi( sum_{r,s,ci} x[n, oy*stride + r*dil - pad_h, ox*stride + s*dil - pad_w, ci]
 *                                   * w[co][r][s][ci] )
 * w is K-major packed: [Cout][R][S][Cin] in `dtype`.  Out-of-range taps read zero.
 * epi: +bias[co] (fp32, nullable) -> relu (flag) -> * (mask[n,oy,ox,co] > 0 ? mask_scale : 0) for
 *      co < mask_channels (mask nullable; ReLU / dropout backward fused) -> (+= old y if accumulate).
 * scatter2x2 != 0: the N dimension is (a,b,co) = 4*Cout and element (pixel, (a,b,co)) is stored at
 *      y[n, 2*oy+a, 2*ox+b, co]  (ConvTranspose2d k=2 s=2 forward, network.py:126,169).
 * With dgrad-packed weights ([Cin][flipped taps][Cout]) and pad = k-1 the same entry computes
 * the input gradient of a stride-1 conv; with R=S=2, stride 2 it computes ConvTranspose2d's.
 * Cin must be a multiple of 32 (bf16) / 16 (f32); Cout (or 4*Cout) a multiple of 64.
 */
typedef struct dct_conv_desc {
  int32_t R, S, stride, dil, pad_h, pad_w;
  int32_t relu;
  int32_t scatter2x2;
  int32_t accumulate;
  int32_t mask_channels;
  float mask_scale;
  /* ReLU-gate bits: one bit per element of a DENSE bf16 NHWC tensor, byte (pixel * C/8 + c/8), bit c%8 = "element > 0".
   * relu_bits_out (nullable): dct_conv2d / dct_conv_cin1_fwd also leave the bits of y there (y dense, C % 8 == 0, bf16).
   * mask_bits (nullable, with `mask` still passed): the same information as `mask` (dense, mask_channels = all of y's
   * channels) at 1/16 of the bytes; the kernels whose epilogue can, read it instead of the activation. */
  const uint8_t* mask_bits;
  uint8_t* relu_bits_out;
  /* 2x2 / stride 2 / ceil-mode max pooling of y in the same call (nn.MaxPool2d behind the conv + ReLU of a UNet encoder block,
   * arch/network.py:120-130): pool_out (nullable) is a DENSE NHWC tensor [n][(h+1)/2][(w+1)/2][c] of y's type; pool_codes
   * (nullable) the routing codes of dct_maxpool2x2_fwd_codes, one byte per pooled element.  The shared-halo kernel pools its
   * staged output tile before the tile leaves LDS (the pool no longer re-reads y from memory; y itself is still written unless
   * pool_only says nobody reads it); every other path launches the pooling kernel behind the conv.  Results are those of
   * dct_conv2d followed by dct_maxpool2x2_fwd[_codes], bit for bit.  Not with scatter2x2 / accumulate, and not with mask /
   * mask_bits (a forward-pass feature: the staged tile is pooled before the gates of a data gradient would be applied). */
  void* pool_out;
  uint8_t* pool_codes;
  /* pool_only != 0 (with pool_out): the caller consumes only the pooled tensor -- y must still be a valid buffer, but its contents
   * after the call are unspecified: the shared-halo kernel then skips its row stores (a UNet encoder block's full-resolution output
   * is read by the pooling alone once the backward pass routes by pool_codes: 130 MB less to write at the first level). */
  int32_t pool_only;
  /* The UNet stem's weight gradient from the epilogue of the data gradient that produces its dy (network.py:159-161: Conv2d(1, 64, 3),
   * ReLU, Conv2d(64, 64, 3)): with stem_x (nullable; dense fp32 [n][y->h + 2][y->w + 2], the single-channel input of the stem) a
   * bf16 64 -> 64 channel 3x3 data gradient with mask_bits (mask_scale 1) also forms stem_dw[64][9] (+)= sum_px y[px][c] * x[px + tap] and
   * stem_db[64] (+)= sum_px y[px][c] from its masked, bf16-rounded output tile while the tile is in LDS -- and then does NOT store y
   * (132 MB written and read back per network and step, by nobody else when d/dx of the network is not asked for).  y must still be a valid
   * view (shapes).  Needs dct_conv2d_workspace_bytes of workspace; DCT_ERR_UNSUPPORTED when the layer does not take the shared-halo
   * 64-channel tile (the caller then runs dct_conv2d and dct_conv_cin1_wgrad as before). */
  const float* stem_x;
  float* stem_dw;
  float* stem_db;
  int32_t stem_accumulate;
} dct_conv_desc;

size_t dct_conv2d_workspace_bytes(const dct_view* x, const dct_view* y, const dct_conv_desc* d, int dtype);
int dct_conv2d(const dct_view* x, const void* w_packed, const float* bias, const dct_view* mask,
               const dct_view* y, const dct_conv_desc* d, int dtype,
               void* workspace, size_t workspace_bytes, dct_stream stream);

/* Weight gradient: dw[p][r][s][q] (+)= sum_m P[m][p] * Q[pixel(m)*stride + (r,s)*dil - pad][q]
 * (fp32 output, K-major like the packed weights).  Conv2d: P = dy, Q = x.  ConvTranspose2d k2 s2:
 * P = x, Q = dy, R=S=2, stride 2.   Replaces the weight half of conv backward (autograd of
 * cotraining_totalloss.py:247). */
size_t dct_conv2d_wgrad_workspace_bytes(const dct_view* p, const dct_view* q, const dct_conv_desc* d, int dtype);
int dct_conv2d_wgrad(const dct_view* p, const dct_view* q, float* dw, const dct_conv_desc* d, int dtype,
                     void* workspace, size_t workspace_bytes, dct_stream stream);
/* Same, and db[c] (+)= sum over pixels of p[.., c] in the same launch (the bias gradient of a Conv2d is the column
 * sum of the dy tiles the kernel already holds: one extra MFMA against a ones vector).  bf16 only; db nullable. */
int dct_conv2d_wgrad_bias(const dct_view* p, const dct_view* q, float* dw, float* db, const dct_conv_desc* d, int dtype,
                          void* workspace, size_t workspace_bytes, dct_stream stream);

/* db[c] (+)= sum over pixels of dy[.., c]  (bias half of conv backward). */
int dct_bias_grad(const dct_view* dy, float* db, int accumulate, int dtype,
                  void* workspace, size_t workspace_bytes, dct_stream stream);
size_t dct_bias_grad_workspace_bytes(const dct_view* dy);
/* n (<= 8) bias gradients in one launch pair: dbs[k][c] (+)= sum over pixels of dys[k][.., c]; per job the sums and their order are those of
 * dct_bias_grad.  (A UNet's four up-convolutions: nn.ConvTranspose2d's bias gradient is the column sum of the OTHER operand of its weight-gradient
 * GEMM, so it cannot ride along there; four launch pairs of ~5 us each sat on every model's backward chain.) */
int dct_bias_grad_batched(const dct_view* dys, float* const* dbs, int n, int accumulate, int dtype,
                          void* workspace, size_t workspace_bytes, dct_stream stream);
size_t dct_bias_grad_batched_workspace_bytes(const dct_view* dys, int n);

/* Repack fp32 master weights src[P][T][Q] (T taps) into `dtype`:
 *   transpose == 0: straight cast copy;
 *   transpose == 1: dst[Q][T'][P]  (conv dgrad pack; tap order reversed when flip_taps);
 *   transpose == 2: dst[T'][Q][P]  (ConvTranspose2d forward pack for the scatter2x2 mode). */
int dct_pack_weight(const float* src, void* dst, int P, int T, int Q, int transpose, int flip_taps,
                    int dtype, dct_stream stream);
/* All transposed packs of a network in one launch.  jobs_dev: device array of njobs records
 *   { const void* src; void* dst; int32 P, T, Q, flip; int64 dq, dt; int32 tile_begin, src_bf16; }  (56 bytes;
 *     src is fp32, or the bf16 image of the same tensor when src_bf16 != 0)
 * job j covers the 32 x 32 (p, q) tiles [tile_begin[j], tile_begin[j+1]) (P/32 * Q/32 * T of them; P, Q
 * multiples of 32) of dst[q*dq + t'*dt + p] = src[p][t][q]: (dq, dt) = (T*P, P) is dct_pack_weight's
 * transpose == 1, (P, Q*P) its transpose == 2.  total_tiles = tile_begin past the last job. */
int dct_pack_weights_batched(const void* jobs_dev, int njobs, int total_tiles, int dtype, dct_stream stream);
/* The same table for 16-bit (bf16 / f16) sources AND destinations, on 64 x 64 tiles with 16-byte accesses: every job has
 * src_bf16 != 0, P and Q multiples of 64, dq and dt multiples of 8, 16-byte aligned src / dst; tile_begin counts 64 x 64
 * tiles (P/64 * Q/64 * T per job).  This is the per-step re-pack of a bf16 UNet (arch/unet.py::_ensure_packs). */
int dct_pack_weights_batched64(const void* jobs_dev, int njobs, int total_tiles, dct_stream stream);

/* First layer, Cin = 1 (network.py:159 dec1 conv; enet.py:21 initial conv): direct conv.
 * x is fp32 [N,H,W,1]; w fp32 [Cout][R][S]; y in `dtype`. */
int dct_conv_cin1_fwd(const dct_view* x, const float* w, const float* bias, const dct_view* y,
                      const dct_conv_desc* d, int dtype, dct_stream stream);
/* dx (fp32) = full correlation of dy with w  (the d/dx FGSM needs: AEGenerator.py:27-28). */
int dct_conv_cin1_dgrad(const dct_view* dy, const float* w, const dct_view* dx,
                        const dct_conv_desc* d, int dtype, dct_stream stream);
size_t dct_conv_cin1_wgrad_workspace_bytes(const dct_view* dy, const dct_conv_desc* d);
int dct_conv_cin1_wgrad(const dct_view* x, const dct_view* dy, float* dw, float* db,
                        const dct_conv_desc* d, int accumulate, int dtype,
                        void* workspace, size_t workspace_bytes, dct_stream stream);

/* Classifier head: 1x1 conv to a few classes (network.py:223 `final`), Cout <= 8.
 * x in `dtype` [.., Cin]; w fp32 [Cout][Cin]; y fp32 [.., Cout]. */
int dct_conv1x1_head_fwd(const dct_view* x, const float* w, const float* bias, const dct_view* y,
                         int dtype, dct_stream stream);
size_t dct_conv1x1_head_bwd_workspace_bytes(const dct_view* x, int cout);
/* dx (dtype, optional) = dy*W masked by (x>0) when relu_mask; dw,db (fp32, optional) (+)=. */
int dct_conv1x1_head_bwd(const dct_view* x, const dct_view* dy, const float* w, const dct_view* dx,
                         float* dw, float* db, int relu_mask, int accumulate, int dtype,
                         void* workspace, size_t workspace_bytes, dct_stream stream);

/* ---- K4: max pooling 2x2 stride 2 (ceil mode) ------------------------------------------
 * Replaces nn.MaxPool2d(2, stride=2, ceil_mode=True) (network.py:166).  y.h = ceil(x.h/2).
 * bwd: dx = dy routed to the first max in scan order, then * (x > 0 ? scale : 0) when relu_mask
 * (fuses the ReLU / dropout backward that precedes the pool). */
int dct_maxpool2x2_fwd(const dct_view* x, const dct_view* y, int dtype, dct_stream stream);
int dct_maxpool2x2_bwd(const dct_view* x, const dct_view* dy, const dct_view* dx, int relu_mask,
                       float scale, int dtype, dct_stream stream);

/* The same pair with the routing kept from the forward pass instead of re-derived from x: codes (uint8, dense
 * [N][y.h][y.w][C], 8-byte aligned) receives per pooled element bits 0-1 = window position (2*dy+dx) of the first maximum,
 * bit 2 = "maximum > 0" (the ReLU / dropout gate), bit 3 = no maximum; the backward pass reads dy and codes only.
 * dct_maxpool2x2_bwd_codes also takes views off the 16-byte vector width (one element per thread; codes then need no alignment). */
int dct_maxpool2x2_fwd_codes(const dct_view* x, const dct_view* y, uint8_t* codes, int dtype, dct_stream stream);
int dct_maxpool2x2_bwd_codes(const uint8_t* codes, const dct_view* dy, const dct_view* dx, int relu_mask,
                             float scale, int dtype, dct_stream stream);
/* The same with the gradient of a second reader of the pooled tensor gathered on the way: `skip` is the gradient at a bilinearly resized
 * (align_corners) copy of it -- the UNet's skip connection, network.py:205-239 `F.upsample(dec_k, size, mode='bilinear')` -- and
 * dx = unpool(dy + bilinear_backward(skip)): what dct_bilinear_bwd into dy followed by dct_maxpool2x2_bwd_codes gives, with one write and
 * one read of dy less and the sum kept in fp32 until it is routed. */
int dct_maxpool2x2_bwd_codes_skip(const uint8_t* codes, const dct_view* dy, const dct_view* skip, const dct_view* dx, int relu_mask,
                                  float scale, int dtype, dct_stream stream);

/* ---- K5: bilinear resize, align_corners=True -------------------------------------------
 * Replaces F.upsample_bilinear (network.py:232-240).  Any in/out size.  y may be a channel
 * slice of a concat buffer.  in/out dtypes given separately (the final resize reads/writes f32).
 * bwd is a gather (deterministic): dx[src] (+)= sum of dy[dst]*weight. */
int dct_bilinear_fwd(const dct_view* x, const dct_view* y, int dtype_in, int dtype_out, dct_stream stream);
/* n (<= 8) resizes of one dtype in ONE launch: ys[k] = dct_bilinear_fwd(xs[k]), bit for bit.  DCT_ERR_UNSUPPORTED for views off the 16-byte
 * vector width (use one dct_bilinear_fwd per tensor).  (A UNet's four skip connections, network.py:216-223: every pooled tensor exists once the
 * encoder is through.) */
int dct_bilinear_fwd_batched(const dct_view* xs, const dct_view* ys, int n, int dtype, dct_stream stream);
int dct_bilinear_bwd(const dct_view* dy, const dct_view* dx, int dtype_dy, int dtype_dx, int accumulate,
                     dct_stream stream);

/* ---- K9: dropout ------------------------------------------------------------------------
 * Replaces nn.Dropout(.5) (network.py:165,210).  Philox4x32-10 keyed by (seed, offset + element
 * index); y = keep ? x/(1-p) : 0.  mask_out (uint8, nullable, dense NHWC) receives the keep mask. */
int dct_dropout_fwd(const dct_view* x, const dct_view* y, uint8_t* mask_out, float p,
                    uint64_t seed, uint64_t offset, int dtype, dct_stream stream);
/* Same, with the call counter in device memory: calls = TWO 64-bit words that successive launches use in turn.  The launch reads
 * calls[parity] = n, is call number n + 1 (offset = that << 40) and stores n + 1 to calls[parity ^ 1]; the caller alternates `parity` (0, 1, 0, ...)
 * from launch to launch, stream-ordered.  Nothing in the launch depends on a per-step host value, so a captured HIP graph of the training step
 * draws a fresh mask on every replay -- provided a replay holds an EVEN number of launches per counter (a UNet forward pass has two sites). */
int dct_dropout_fwd_dev(const dct_view* x, const dct_view* y, uint8_t* mask_out, float p,
                        uint64_t seed, uint64_t* calls, int parity, int dtype, dct_stream stream);
/* dct_dropout_fwd_dev followed by dct_maxpool2x2_fwd_codes in ONE pass: y = maxpool(dropout(x)) and its routing codes, bit for bit, without the
 * dropped full-resolution tensor (the backward pass routes by the codes and the 1 / (1 - p) scale).  The fourth encoder level of a UNet's training
 * pass (network.py:160-166: conv, ReLU, Dropout, MaxPool2d).  calls / parity as dct_dropout_fwd_dev. */
int dct_dropout_maxpool2x2_fwd_codes(const dct_view* x, const dct_view* y, uint8_t* codes, float p, uint64_t seed, uint64_t* calls,
                                     int parity, int dtype, dct_stream stream);
/* y = x * (mask_u8 ? 1/(1-p) : 0) with a caller-supplied dense mask (parity replay). */
int dct_dropout_apply(const dct_view* x, const dct_view* y, const uint8_t* mask, float p, int dtype,
                      dct_stream stream);

/* ---- K7: elementwise -------------------------------------------------------------------- */
/* y = g * (a > 0 ? scale : 0)   (ReLU backward where it cannot be fused). */
int dct_relu_bwd(const dct_view* g, const dct_view* a, const dct_view* y, float scale, int dtype,
                 dct_stream stream);
int dct_cast(const dct_view* x, const dct_view* y, int dtype_in, int dtype_out, dct_stream stream);

/* ---- K10: pixel-wise losses on fp32 NHWC logits [P pixels][C], 2 <= C <= 8 ----------------
 * CE     : loss/loss.py:12-25   (log_softmax + NLL, mean over targets != ignore_index)
 * softmax: models/segmentators.py:50
 * JSD    : loss/loss.py:183-196 + :70-84 ; fused from logits of S <= 4 models; *mean* over pixels
 * KL     : loss/loss.py:110-134 ; KL(y || p), y detached, mean over pixels
 * All reductions are two-stage and deterministic.  Scalars are written to device memory;
 * nothing synchronises with the host.
 */
size_t dct_loss_workspace_bytes(int64_t pixels);
/* out[0] = mean CE, out[1] = number of counted pixels.  targets int64. */
int dct_ce_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
               float* out2, void* workspace, size_t workspace_bytes, dct_stream stream);
/* dlogits (=|+=) gscale[0] * gmul * (softmax - onehot) / count ; gscale is a device scalar (nullable=1) */
int dct_ce_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
               const float* count, const float* gscale, float gmul, float* dlogits, int accumulate,
               dct_stream stream);
/* dct_ce_fwd + dct_ce_bwd of the same logits in two launches instead of three: the backward kernel folds the forward kernel's block partials
 * itself (every block, in the forward call's order: out2 and dlogits are bit for bit those of the two calls).  The co-training step's supervised
 * term (cotraining_totalloss.py:211-216 + the loss.backward() of :247). */
int dct_ce_step(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index, float* out2,
                const float* gscale, float gmul, float* dlogits, int accumulate, void* workspace, size_t workspace_bytes,
                dct_stream stream);
/* Class-weighted cross entropy with the reductions of torch's F.cross_entropy(weight=, ignore_index=, reduction=) (the weight / reduce /
 * size_average arguments of loss/loss.py:12-25).  weight: C fp32 values in device memory, nullable = all ones; the kernels pick w_t by an
 * unrolled select, never by weight[t].  Per pixel i:
 *   l_i = logsumexp(x_i) - x_i[t_i];   w_i = weight[t_i] (1 when weight is NULL);
 *   t_i == ignore_index: w_i = 0 and l_i = 0;  a target outside [0, C) that is not ignore_index is treated as ignored too (torch raises
 *   there; nothing is indexed with it).
 * reduction 0 (mean): out2[0] = sum w_i l_i / sum w_i, out2[1] = sum w_i (the denominator); NaN when sum w_i == 0, as in torch (the gradients
 *   are then unspecified).      reduction 1 (sum): out2[0] = sum w_i l_i, out2[1] = sum w_i; the gradient's denominator is 1.
 * Gradient: dlogits[i][c] (=|+=) (g * w_i) * (p_c - [t_i == c]) with g = gscale[0] * gmul / denom formed in this order (gscale nullable = 1;
 *   denom = out2 + 1 of the forward call under mean, not read under sum): all-ones weights under mean give dct_ce_bwd's result bit for bit.
 *   Ignored pixels get exactly 0 (exactly the old value under accumulate).
 * dct_ce_weighted_step: fwd + bwd in two launches like dct_ce_step (the backward kernel folds the forward kernel's block partials itself);
 *   out2 and dlogits are bit for bit those of dct_ce_weighted_fwd followed by dct_ce_weighted_bwd.
 * map (reduce=False): map[i] = w_i l_i;  backward: dlogits[i][c] (=|+=) (gmul * dmap[i] * w_i) * (p_c - [t_i == c]).
 * DCT_ERR_BAD_ARG: a null logits / targets / out pointer, pixels < 1, a reduction other than 0 or 1; DCT_ERR_UNSUPPORTED: C outside 2..8;
 * DCT_ERR_WORKSPACE: less than dct_loss_workspace_bytes of workspace. */
int dct_ce_weighted_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                        const float* weight /*nullable*/, int reduction, float* out2, void* workspace, size_t workspace_bytes,
                        dct_stream stream);
int dct_ce_weighted_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                        const float* weight, int reduction, const float* denom /*out2 + 1*/, const float* gscale, float gmul,
                        float* dlogits, int accumulate, dct_stream stream);
int dct_ce_weighted_step(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                         const float* weight, int reduction, float* out2, const float* gscale, float gmul, float* dlogits,
                         int accumulate, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_ce_map_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                   const float* weight /*nullable*/, float* map, dct_stream stream);
int dct_ce_map_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                   const float* weight, const float* dmap, float gmul, float* dlogits, int accumulate, dct_stream stream);
/* Focal loss (Lin et al., "Focal loss for dense object detection", ICCV 2017) in its softmax form: the cross entropy of a pixel scaled by
 * (1 - p_t)^gamma, so that the easy pixels stop carrying the sum.  logits fp32 [pixels][C], 2 <= C <= 8; targets int64; weight: C fp32
 * values in device memory, nullable = all ones, picked by an unrolled select, never by weight[t]; gamma: a host float, finite and >= 0.
 * A pixel is counted exactly as in dct_ce_weighted_*: t != ignore_index && 0 <= t < C.  Per counted pixel, with p = softmax(x), y the
 * one-hot of t and w = weight[t]:
 *   q = sum_{c != t} p_c, the probability mass off the target -- summed, never formed as 1 - p_t, so that its relative error stays a few
 *       units of roundoff at a confident pixel;
 *   l = -log p_t;
 *   m = q^gamma, with m = 1 when gamma == 0 whatever q is, and m = 0 when q == 0 && gamma > 0;
 *   f = w m l;
 *   k = m + gamma p_t l q^(gamma - 1): 1 when gamma == 0, 0 when q == 0 && gamma > 0;
 *   d f / d x_c = w k (p_c - y_c).
 *   No inf * 0 and no 0 / 0 arises for any finite logits.
 * reduction 0 (mean): out2[0] = sum f / sum w over the counted pixels, out2[1] = sum w (NaN when sum w == 0, as in dct_ce_weighted_fwd).
 *   With gamma == 0 this is F.cross_entropy(weight=, ignore_index=, reduction='mean'); with weight == NULL it is the mean over the counted
 *   pixels that most published focal-loss code uses.      reduction 1 (sum): out2[0] = sum f, out2[1] = sum w.
 * Gradient: dlogits[i][c] (=|+=) (g w k) (p_c - y_c) with g = gscale[0] * gmul (gscale nullable = 1), divided by sum w under the mean
 *   (denom = out2 + 1 of the forward call; not read under the sum).  Uncounted pixels get exactly 0 in the map and in the gradient
 *   (exactly the old value under accumulate).
 * dct_focal_step: fwd + bwd in two launches like dct_ce_weighted_step (the backward kernel folds the forward kernel's block partials in
 *   every block); out2 and dlogits are bit for bit those of dct_focal_fwd followed by dct_focal_bwd.
 * map: map[i] = f_i;  backward: dlogits[i][c] (=|+=) (gmul * dmap[i] * w k) (p_c - y_c).
 * All sums are folded in one fixed order without float atomics: bit-identical from run to run.  Workspace: dct_loss_workspace_bytes.
 * DCT_ERR_BAD_ARG: as for dct_ce_weighted_*, and a gamma that is negative, NaN or infinite; DCT_ERR_UNSUPPORTED: C outside 2..8;
 * DCT_ERR_WORKSPACE: less than dct_loss_workspace_bytes of workspace.
 * Out of scope: the sigmoid (binary) form, a per-pixel alpha map, focal + Dice in one launch, gamma in device memory, probabilities as
 * input. */
int dct_focal_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                  const float* weight /*nullable*/, float gamma, int reduction, float* out2, void* workspace, size_t workspace_bytes,
                  dct_stream stream);
int dct_focal_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                  const float* weight, float gamma, int reduction, const float* denom /*out2 + 1*/, const float* gscale, float gmul,
                  float* dlogits, int accumulate, dct_stream stream);
int dct_focal_step(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                   const float* weight, float gamma, int reduction, float* out2, const float* gscale, float gmul, float* dlogits,
                   int accumulate, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_focal_map_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                      const float* weight /*nullable*/, float gamma, float* map, dct_stream stream);
int dct_focal_map_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                      const float* weight, float gamma, const float* dmap, float gmul, float* dlogits, int accumulate, dct_stream stream);
/* Top-k cross entropy (nnU-Net's TopKLoss; online hard-example mining): the mean of the per-pixel class-weighted cross entropy over the
 * hardest k_percent of the counted pixels only.  logits, targets, weight and ignore_index are those of dct_ce_weighted_*; k_percent: a
 * host double, finite, 0 < k_percent <= 100.  A pixel is counted exactly as in dct_ce_weighted_*: t != ignore_index && 0 <= t < C.
 *   v_i = w_i l_i for a counted pixel, 0 for an uncounted one: bit for bit the map of dct_ce_map_fwd.  The forward call stores it in vmap
 *       (fp32 [pixels], provided by the caller), and every later comparison reads the stored value, never a recomputed one (a backward
 *       kernel whose recomputed v_i differed in the last bit would put the pixel on the wrong side of the threshold).
 *   N = the number of counted pixels;  K = min(N, max(1, (int64) floor((double) N * k_percent / 100.0))), formed on the device in IEEE
 *       double in this order (Python's int(N * k / 100), clamped).
 *   tau = the K-th largest v_i over the counted pixels, in the order of float comparison with -0 equal to +0.  Negative values are allowed
 *       (weights need not be >= 0).  A NaN orders above +inf: if any counted v_i is NaN the value is NaN and the gradient is unspecified.
 *   n_gt = #{counted i: v_i > tau}, n_eq = #{counted i: v_i == tau}, so n_gt < K <= n_gt + n_eq.
 * Value: out2[0] = (sum_{v_i > tau} v_i + (float)(K - n_gt) * tau) / (float) K, out2[1] = tau: the mean of torch.topk(v, K) whatever the
 *   ties are.  counts4 (int64 [4] on the device) = {K, N, n_gt, n_eq}.  N == 0: K = 0, the value is NaN, every gradient entry exactly 0
 *   (the old value under accumulate).  k_percent == 100 with weight == NULL is the plain mean cross entropy; with weights it is
 *   sum w l / N, not / sum w.
 * Gradient: dlogits[i][c] (=|+=) (g a_i w_i)(p_c - y_c) with g = gscale[0] * gmul / (float) K (gscale nullable = 1); a_i = 1 where
 *   v_i > tau, (float)(K - n_gt) / (float) n_eq where v_i == tau (the ties share what is left: a valid subgradient that depends on neither
 *   pixel order nor launch geometry), 0 below tau.  Uncounted pixels and counted pixels below tau get exactly 0 for finite logits (exactly
 *   the old value under accumulate).
 * tau is found by a most-significant-digit radix select (11 + 11 + 10 bits) over the order-preserving 32-bit keys of the stored map; the
 *   histograms use integer atomics only, the float sum is folded in one fixed order without float atomics: bit-identical from run to
 *   run.  Nothing synchronises with the host.  The entry point zeroes the histograms itself (a memset on the stream): the caller never
 *   clears the workspace.
 * dct_topk_ce_bwd: vmap, out2 and counts4 are those of the forward call under the same arguments.
 * dct_topk_ce_step: fwd + bwd of the same logits; out2, counts4, vmap and dlogits are bit for bit those of the two calls.
 * DCT_ERR_BAD_ARG: as for dct_ce_weighted_*, a null vmap / counts4, or a k_percent that is NaN, <= 0 or > 100; DCT_ERR_UNSUPPORTED: C
 * outside 2..8, or pixels > 2^31 - 1; DCT_ERR_WORKSPACE: less than dct_topk_ce_workspace_bytes(pixels) of workspace.
 * Out of scope: per-image top-k, top-k + Dice in one launch, k_percent in device memory, top-k of the focal map, probabilities as
 * input. */
size_t dct_topk_ce_workspace_bytes(int64_t pixels);
int dct_topk_ce_fwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                    const float* weight /*nullable*/, double k_percent, float* out2, int64_t* counts4, float* vmap, void* workspace,
                    size_t workspace_bytes, dct_stream stream);
int dct_topk_ce_bwd(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                    const float* weight, const float* vmap, const float* out2, const int64_t* counts4, const float* gscale, float gmul,
                    float* dlogits, int accumulate, dct_stream stream);
int dct_topk_ce_step(const float* logits, const int64_t* targets, int64_t pixels, int C, int ignore_index,
                     const float* weight, double k_percent, float* out2, int64_t* counts4, float* vmap, const float* gscale, float gmul,
                     float* dlogits, int accumulate, void* workspace, size_t workspace_bytes, dct_stream stream);
/* Soft Dice and CE + Dice as one supervised criterion (the reference's loss/dice.py, SURVEY 2 row 3, on logits).  logits: fp32 NHWC
 * [B][pixels_per_image][C]; targets: int64 [B * pixels_per_image]; weight: the C fp32 class weights of the CE term on the device, nullable
 * = all ones, exactly as in dct_ce_weighted_*; class_mask: bit c set = class c takes part in the Dice mean, K = the number of set bits
 * below C; smooth >= 0; per_image 0: one group over the whole batch (G = 1), 1: one group per image (G = B); ce_coef, dice_coef: host floats.
 * A pixel i is counted as in the weighted CE: t_i != ignore_index && 0 <= t_i < C.  Uncounted pixels take part in no sum and get a gradient
 * of exactly 0 (exactly the old value under accumulate).  With p = softmax(x_i) and y the one-hot of t_i, per group g and class c over the
 * counted pixels of g:
 *   I = sum p_c y_c,  S = sum p_c,  Y = sum y_c,  D_gc = (2 I + smooth) / (S + Y + smooth);
 *   a denominator of 0 (smooth = 0 and no counted pixel): D_gc = 1, and the class contributes no gradient.
 *   dice  = 1 - (1 / (G K)) sum_g sum_{c in mask} D_gc
 *   ce    = sum w_i l_i / sum w_i, the rule of dct_ce_weighted_fwd under reduction 0 (NaN when sum w_i == 0)
 *   total = ce_coef ce + dice_coef dice; a coefficient that is exactly 0 removes its term from the total and from the gradient (a NaN ce
 *           then does not reach total).
 * dct_ce_dice_fwd writes out4 = {total, ce, sum w_i, dice}, dice_gc [G][C] = D_gc of every class, masked in or not (for logging), and
 *   sums [G][C][3] = {I, S, Y}, which the backward call reads.
 * Gradient, with g = gscale[0] * gmul (gscale nullable = 1):
 *   dlogits[i][c] (=|+=) g (ce_coef (w_i / sum w)(p_c - y_c) + dice_coef p_c (q_c - sum_k p_k q_k)),
 *   q_c = -(m_c / (G K)) (alpha_gc y_c - beta_gc),  alpha = 2 / (S + Y + smooth),  beta = (2 I + smooth) / (S + Y + smooth)^2,
 *   m_c = 1 for the classes of the mask, else 0.
 * dct_ce_dice_bwd reads out4 (its sum w_i) and sums of the forward call.  dct_ce_dice_step: fwd + bwd in two launches like dct_ce_step
 *   (the backward kernel folds the forward kernel's block partials itself); out4, dice_gc, sums and dlogits are bit for bit those of
 *   dct_ce_dice_fwd followed by dct_ce_dice_bwd.  All sums are folded in one fixed order without float atomics: bit-identical from run to
 *   run, and under per_image a group's numbers depend on that image alone (a permutation of the images permutes the rows of dice_gc).
 * Workspace: dct_ce_dice_workspace_bytes(B, C, per_image) (more than dct_loss_workspace_bytes: 3 C + 2 sums per block); no clearing needed.
 * DCT_ERR_BAD_ARG: a null logits / targets / out4 / dice_gc / sums / dlogits pointer, pixels_per_image < 1, B < 1, smooth < 0 or not finite,
 *   a class_mask with no bit below C, per_image outside {0, 1}; DCT_ERR_UNSUPPORTED: C outside 2..8, B > 65535; DCT_ERR_WORKSPACE: too
 *   little workspace.
 * Out of scope: the squared-denominator (V-Net) form, generalized (volume-weighted) Dice, and probabilities as input. */
size_t dct_ce_dice_workspace_bytes(int B, int C, int per_image);
int dct_ce_dice_fwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C, int ignore_index,
                    const float* weight /*nullable*/, int class_mask, float smooth, int per_image, float ce_coef, float dice_coef,
                    float* out4, float* dice_gc, float* sums, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_ce_dice_bwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C, int ignore_index,
                    const float* weight, int class_mask, float smooth, int per_image, float ce_coef, float dice_coef,
                    const float* out4, const float* sums, const float* gscale, float gmul, float* dlogits, int accumulate,
                    dct_stream stream);
int dct_ce_dice_step(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C, int ignore_index,
                     const float* weight, int class_mask, float smooth, int per_image, float ce_coef, float dice_coef, float* out4,
                     float* dice_gc, float* sums, const float* gscale, float gmul, float* dlogits, int accumulate, void* workspace,
                     size_t workspace_bytes, dct_stream stream);
/* Tversky loss (Salehi et al. 2017) and focal Tversky loss (Abraham & Khan 2019), alone or beside the class-weighted cross entropy, as one
 * supervised criterion on logits.  logits, targets, weight, class_mask, K, smooth, per_image, G, the counted pixels (t_i != ignore_index
 * && 0 <= t_i < C), the sums I = sum p_c y_c, S = sum p_c, Y = sum y_c per group g and class c, ce and sum w_i are those of dct_ce_dice_*.
 * alpha >= 0 weighs the false positives S - I, beta >= 0 the false negatives Y - I (alpha + beta > 0); gamma > 0 is the focal parameter,
 * the exponent is 1 / gamma as in the paper; ce_coef, tversky_coef: host floats.
 *   Den_gc = (1 - alpha - beta) I + alpha S + beta Y + smooth,   N_gc = I + smooth,   T_gc = N / Den
 *            a denominator of 0: T_gc = 1, and the class contributes neither to the value nor to the gradient (Dice's empty denominator)
 *   u_gc   = max(1 - T, 0)
 *   term   = u when gamma == 1 (no power function is evaluated), else u^(1 / gamma); u == 0: term = 0 and no gradient
 *   tversky = (1 / (G K)) sum_g sum_{c in mask} term_gc
 *   total  = ce_coef ce + tversky_coef tversky; a coefficient that is exactly 0 removes its term from the total and from the gradient (a
 *            NaN ce then does not reach total).
 *   alpha = beta = 0.5 is the soft Dice loss with twice the smooth; alpha = beta = 1 is the Jaccard loss.
 * Gradient, with g = gscale[0] * gmul (gscale nullable = 1) and m_c = 1 for the classes of the mask, else 0:
 *   dlogits[i][c] (=|+=) g (ce_coef (w_i / sum w)(p_c - y_c) + tversky_coef p_c (q_c - sum_k p_k q_k)),   q_c = qb_gc - y_c qa_gc
 *   f_gc  = (m_c / (G K)) (1 / gamma) u^(1 / gamma - 1)      (gamma == 1: m_c / (G K);  u == 0 or Den == 0: 0)
 *   qa_gc = f (1 - (1 - alpha - beta) T) / Den,              qb_gc = f alpha T / Den
 * Arithmetic: the host forms c0 = 1 - alpha - beta and e = 1 / gamma once, in double from the fp32 arguments, and rounds each to fp32
 *   once; the kernels take e - 1 from the fp32 e.  Den = ((c0 I + alpha S) + beta Y) + smooth with one rounding per operation (no fused
 *   multiply-add), u^x = exp2f(x log2f(u)), f = ((m / (G K)) e) u^(e - 1), qa = (f (1 - c0 T)) / Den, qb = ((f alpha) T) / Den.
 * dct_ce_tversky_fwd writes out4 = {total, ce, sum w_i, tversky}, tversky_gc [G][C] = T_gc, the index itself, of every class, masked in or
 *   not (for logging), and sums [G][C][3] = {I, S, Y}, which the backward call reads.  dct_ce_tversky_bwd reads out4 (its sum w_i) and sums
 *   of the forward call.  dct_ce_tversky_step: fwd + bwd in two launches; out4, tversky_gc, sums and dlogits are bit for bit those of
 *   dct_ce_tversky_fwd followed by dct_ce_tversky_bwd.  The forward partial sums are dct_ce_dice_*'s kernel and fold order: no float
 *   atomics, bit-identical from run to run, and under per_image a permutation of the images permutes the rows of tversky_gc.
 * Workspace: dct_ce_tversky_workspace_bytes(B, C, per_image) (= dct_ce_dice_workspace_bytes); no clearing needed.
 * DCT_ERR_BAD_ARG: everything dct_ce_dice_* refuses with it (tversky_gc in place of dice_gc); alpha or beta negative or not finite;
 *   alpha + beta == 0 (the index is constantly 1); gamma not finite or <= 0.  DCT_ERR_UNSUPPORTED, DCT_ERR_WORKSPACE: as dct_ce_dice_*.
 * Out of scope: generalized Dice (the weight of an absent class needs a rule of its own), the squared-denominator form, probabilities as
 *   input, Tversky as a consistency term. */
size_t dct_ce_tversky_workspace_bytes(int B, int C, int per_image);
int dct_ce_tversky_fwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C, int ignore_index,
                       const float* weight /*nullable*/, int class_mask, float smooth, float alpha, float beta, float gamma, int per_image,
                       float ce_coef, float tversky_coef, float* out4, float* tversky_gc, float* sums, void* workspace,
                       size_t workspace_bytes, dct_stream stream);
int dct_ce_tversky_bwd(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C, int ignore_index,
                       const float* weight, int class_mask, float smooth, float alpha, float beta, float gamma, int per_image,
                       float ce_coef, float tversky_coef, const float* out4, const float* sums, const float* gscale, float gmul,
                       float* dlogits, int accumulate, dct_stream stream);
int dct_ce_tversky_step(const float* logits, const int64_t* targets, int B, int64_t pixels_per_image, int C, int ignore_index,
                        const float* weight, int class_mask, float smooth, float alpha, float beta, float gamma, int per_image,
                        float ce_coef, float tversky_coef, float* out4, float* tversky_gc, float* sums, const float* gscale, float gmul,
                        float* dlogits, int accumulate, void* workspace, size_t workspace_bytes, dct_stream stream);
/* Boundary loss (Kervadec et al., "Boundary loss for highly unbalanced segmentation"): the softmax weighted by the signed Euclidean
 * distance to the ground-truth contour, here on the device from the targets to the gradient.
 * Targets t [B][H][W] int64; classes 0..C-1, 2 <= C <= 8; spacing (sy, sx), both > 0 and finite; G_c = {t == c}.  A target outside [0, C)
 * is in no class: it is background for every c (that covers ignore_index; the rule of dct_hausdorff).
 * Distances are per image (2-D), centre to centre: d2(p, q) = (sy dy)^2 + (sx dx)^2.  The signed distance phi_c:
 *   p not in G_c:  phi_c(p) = + min_{q in G_c} sqrt(d2(p, q))
 *   p in G_c:      phi_c(p) = -(min_{q not in G_c} sqrt(d2(p, q)) - 1)
 *   The "- 1" is the one of Kervadec's one_hot2dist, kept literally, in units of the spacing.
 *   phi_c = 0 over the whole image when G_c is empty in that image or fills it (no contour inside the image: one_hot2dist writes zeros
 *   for an absent class, scipy's answer for a full mask is arbitrary), or when c is not in class_mask.
 * dct_signed_distance writes phi [B][H][W][C] fp32, the layout of the logits -- EVERY element, the zeros included: the caller clears
 *   nothing.  Exact separable transform (csrc/surface.hip): with unit spacing every squared distance is an integer below 2^24 and the
 *   root is the correctly rounded one, so phi is the float64 result rounded once; no float atomics, bit-identical from run to run.
 *   targets, phi and workspace 16-byte aligned.  dct_signed_distance_workspace_bytes returns 0 for a shape dct_signed_distance refuses.
 * The loss reads s = softmax(x_p) of logits [pixels][C] fp32.  A pixel is counted as in dct_ce_weighted_*: t != ignore_index &&
 * 0 <= t < C; N = the number of counted pixels; K = the number of bits of class_mask below C:
 *   L = (1 / (N K)) sum_{p counted} sum_{c in mask} s_c(p) phi_c(p);     N = 0: L = 0 and every gradient is exactly 0.
 *   (With nothing ignored: one_hot2dist followed by SurfaceLoss's .mean() over B x K x H x W.)
 * dct_boundary_fwd writes out2 = {L, N}; its workspace is dct_loss_workspace_bytes.
 * Gradient, with g = gscale[0] * gmul (gscale nullable = 1, as in dct_ce_bwd):
 *   q_c = m_c phi_c(p) / (N K),  m_c = 1 for the classes of the mask, else 0;
 *   dlogits[p][c] (=|+=) g s_c (q_c - sum_k s_k q_k).
 *   Uncounted pixels get exactly 0 (exactly the old value under accumulate).  All sums are folded in one fixed order: bit-identical from
 *   run to run.  logits, phi and dlogits 16-byte aligned (the kernels read them 16 bytes at a time).
 * DCT_ERR_BAD_ARG: a null pointer, a spacing that is not positive and finite, a class_mask with no bit below C, pixels < 1 or B / H / W < 1,
 *   a misaligned pointer; DCT_ERR_UNSUPPORTED: C outside 2..8, H or W > 1024, B > 65535; DCT_ERR_WORKSPACE: too little workspace.
 *   Every check runs before the first launch.
 * Out of scope: 3-D maps with the batch as a volume, a fused fwd + bwd step, probabilities as input. */
size_t dct_signed_distance_workspace_bytes(int B, int H, int W, int C);
int dct_signed_distance(const int64_t* targets /*[B][H][W]*/, int B, int H, int W, int C, int class_mask, float sy, float sx,
                        float* phi /*[B][H][W][C]*/, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_boundary_fwd(const float* logits, const int64_t* targets, const float* phi, int64_t pixels, int C, int ignore_index,
                     int class_mask, float* out2 /*{L, N}*/, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_boundary_bwd(const float* logits, const int64_t* targets, const float* phi, int64_t pixels, int C, int ignore_index,
                     int class_mask, const float* count /*out2 + 1*/, const float* gscale, float gmul, float* dlogits, int accumulate,
                     dct_stream stream);
int dct_softmax_fwd(const float* logits, float* probs, int64_t pixels, int C, dct_stream stream);
/* dlogits (=|+=) p * (dprobs - sum_c dprobs*p) */
int dct_softmax_bwd(const float* probs, const float* dprobs, float* dlogits, int64_t pixels, int C,
                    int accumulate, dct_stream stream);
/* map[pix] = -sum_c p*log(p+1e-16) */
int dct_entropy_fwd(const float* probs, float* map, int64_t pixels, int C, dct_stream stream);
/* dprobs[pix][c] = dmap[pix] * -(log(p+1e-16) + p/(p+1e-16)) */
int dct_entropy_bwd(const float* probs, const float* dmap, float* dprobs, int64_t pixels, int C, dct_stream stream);
/* probs-in variants keep the reference module API (JSD_2D()(list_of_probs) -> [B,H,W] map). */
int dct_jsd_map_fwd(const float* const* probs, int S, float* map, int64_t pixels, int C, dct_stream stream);
int dct_jsd_map_bwd(const float* const* probs, int S, const float* dmap, float* const* dprobs,
                    int64_t pixels, int C, dct_stream stream);
int dct_kl_map_fwd(const float* p, const float* y, float* map, int64_t pixels, int C, float eps,
                   dct_stream stream);
int dct_kl_map_bwd(const float* p, const float* y, const float* dmap, float* dp, int64_t pixels,
                   int C, float eps, dct_stream stream);
/* fused-from-logits fast path used by the step: out[0] = mean JSD over pixels */
int dct_jsd_logits_fwd(const float* const* logits, int S, int64_t pixels, int C, float* out1,
                       void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_jsd_logits_bwd(const float* const* logits, int S, int64_t pixels, int C, const float* gscale,
                       float gmul, float* const* dlogits, int accumulate, dct_stream stream);
/* The step's whole JSD section in one pass (round 5): out1[0] = mean JSD (dct_jsd_logits_fwd's value, bit for bit), probs[s] (nullable array /
 * entries) = softmax of logits[s] (dct_softmax_fwd), dlogits[s] (nullable array: no gradients) (=|+=) the gradient dct_jsd_logits_bwd writes.
 * Two launches instead of five between the join of the S forward passes and the fork of the S backward passes (cotraining_totalloss.py:219-227). */
int dct_jsd_logits_step(const float* const* logits, int S, int64_t pixels, int C, float* out1, float* const* probs,
                        const float* gscale, float gmul, float* const* dlogits, int accumulate,
                        void* workspace, size_t workspace_bytes, dct_stream stream);
/* ---- pseudo-label consistency: every view is trained on the hard pseudo-labels of the others ----
 * Per pixel: S views (1 <= S <= 8) with probabilities p_s[0..C), a confidence threshold tau >= 0 and eps > 0 (1e-10 as for KL).
 * Teachers are constants: no gradient flows through an argmax, a confidence or a mask.  All comparisons and the sums below are fp32.
 *
 * teacher = DCT_PL_CROSS (cross pseudo supervision, Chen et al. 2021), S >= 2
 *   k_j = first maximum of p_j (dct_argmax's rule: v[c] > v[best], starting at 0)       q_j = p_j[k_j]       m_j = (q_j >= tau)
 *   l_i = -(1 / (S - 1)) * sum_{j != i} m_j * log(p_i[k_j] + eps)                       map = (1 / S) * sum_i l_i
 * teacher = DCT_PL_ENSEMBLE (the voted pseudo-label), S >= 1
 *   sum[c] = ((p_0[c] + p_1[c]) + ...), added in view order        k = first maximum of sum (of the unscaled sums: scaling cannot create a tie)
 *   q = sum[k] * (1.f / (float)S)       m = (q >= tau)             l_i = -m * log(p_i[k] + eps)              map = (1 / S) * sum_i l_i
 * d map / d p_i[c]:   cross     -(1 / (S (S - 1))) * sum_{j != i, k_j == c} m_j / (p_i[c] + eps)
 *                     ensemble  -(1 / S) * m * [k == c] / (p_i[c] + eps)
 * The kernels evaluate both as  map = w * sum_i sum_c n_ic * -log(p_i[c] + eps)  and  d map / d p_i[c] = -(w * n_ic) / (p_i[c] + eps),  with n_ic the
 * number of kept teacher terms of class c that student i meets and w = 1 / (S (S - 1)) resp. 1 / S; where n_ic = 0 nothing is evaluated and the
 * entry is 0 exactly.
 * From logits: p_s = softmax(x_s) with dct_softmax_fwd's bits; d / d x_i[c] = g * p_i[c] * (d_i[c] - sum_c' d_i[c'] p_i[c']), g = gscale[0] * gmul / P
 * (gscale NULL: 1), the form of dct_jsd_logits_bwd.
 * The mean is over all P pixels, never over the kept ones: with everything masked the loss and every gradient are exactly 0 and no 0/0 arises.
 * kept = the fraction of teacher terms with m = 1: of the P * S terms (one per teacher view) for cross, of the P terms for ensemble; the kept
 * map holds that fraction per pixel (kept teachers of the pixel / S resp. / 1).
 * DCT_ERR_BAD_ARG: S outside the mode's range, an unknown mode, a negative or NaN tau, eps <= 0 (or NaN), null pointers, pixels < 1;
 * DCT_ERR_UNSUPPORTED: C outside 2..8; DCT_ERR_WORKSPACE as dct_jsd_logits_step. */
#define DCT_PL_CROSS 0
#define DCT_PL_ENSEMBLE 1
/* probs in (the module API: PseudoLabel_2D()(list_of_probs) -> [B,H,W] map); kept (nullable): the per-pixel kept map.  The backward
 * recomputes the teachers from the probabilities: dprobs[s] = dmap[pix] * d map / d p_s. */
int dct_pl_map_fwd(const float* const* probs, int S, int teacher, float tau, float eps, float* map, float* kept, int64_t pixels, int C,
                   dct_stream stream);
int dct_pl_map_bwd(const float* const* probs, int S, int teacher, float tau, float eps, const float* dmap, float* const* dprobs,
                   int64_t pixels, int C, dct_stream stream);
/* The step's consistency section in one pass over the logits + a finalize: out2 = (mean map value, kept fraction), probs[s] (nullable array /
 * entries) = softmax of logits[s], dlogits[s] (nullable array: no gradients) (=|+=) the logit gradient; accumulate rounds, then adds. */
int dct_pl_logits_step(const float* const* logits, int S, int teacher, float tau, float eps, int64_t pixels, int C, float* out2,
                       float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate,
                       void* workspace, size_t workspace_bytes, dct_stream stream);
/* ---- soft pseudo-label consistency: every view is trained on the SHARPENED soft predictions of the others (MixMatch's Sharpen(q, T)) ----
 * Per pixel: S views (1 <= S <= 8) with fp32 probabilities p_s[0..C), C in 2..8, a teacher mode (DCT_PL_CROSS, S >= 2, or DCT_PL_ENSEMBLE,
 * S >= 1), a confidence threshold tau >= 0, a temperature T > 0, finite, with r = 1.f / T formed in fp32, and eps > 0.
 * Teachers are constants: no gradient flows through a sharpened target, a confidence or a mask.  Everything below is fp32.
 *
 * The raw teacher vector q, its first maximum k and the mask m are dct_pl_*'s, bit for bit:
 *   cross     q_j = p_j,  k_j = first maximum of p_j,  m_j = (p_j[k_j] >= tau)
 *   ensemble  q = ((p_0 + p_1) + ...), added in view order,  k = first maximum of the unscaled sums,  m = (q[k] * (1.f / (float)S) >= tau)
 * The mask is taken on the raw confidence, before sharpening.
 * Sharpening is scale-free, so it is taken from q as it stands (for the ensemble: the unscaled sums):
 *   u[c] = exp2f(r * (log2f(q[c]) - log2f(q[k]))),   u[c] = 0 where q[c] == 0,   u[k] = 1 exactly,
 *   t[c] = u[c] / (u[0] + ... + u[C-1]), added in class order.
 * Student i, class c:   cross     n_ic = sum over j != i, in ascending j, of m_j * t_j[c]
 *                       ensemble  n_ic = m * t[c]
 *   n_ic is formed as that sum, never as a total minus the student's own share: with S = 2, (t_0 + t_1) - t_0 is not t_1, and the error
 *   would be divided by p + eps afterwards.
 * Value and gradient, in dct_pl_*'s form with real-valued n:
 *   map = w * sum_i sum_c n_ic * -log(p_i[c] + eps),   d map / d p_i[c] = -(w * n_ic) / (p_i[c] + eps),   w = 1 / (S (S - 1)) resp. 1 / S;
 *   where n_ic == 0 nothing is evaluated and the entry is 0 exactly.
 * From logits: p_s = softmax(x_s) with dct_softmax_fwd's bits; d / d x_i[c] = g * p_i[c] * (d_i[c] - sum_c' d_i[c'] p_i[c']), g = gscale[0] * gmul / P
 * (gscale NULL: 1); accumulate rounds, then adds.
 * The mean is over all P pixels, never over the kept ones.  kept is dct_pl_*'s kept fraction and kept map, unchanged in meaning.
 * Three consequences:
 *   - T = 1 with the cross teacher is the mean cross entropy of every view against every other view's probabilities (t_j = p_j / sum_c p_j[c]);
 *   - where every teacher's second-largest entry is at most half its largest and T = 2^-10 (r = 1024), every u[c != k] is exp2f of at most
 *     about -1024, which is 0 in fp32: t is exactly one-hot and the rule is the hard pseudo-label's (dct_pl_*);
 *   - with everything masked, the value and every gradient are exactly 0.
 * Status codes are dct_pl_*'s, plus DCT_ERR_BAD_ARG for a temperature that is not finite and > 0, or whose 1.f / T is not finite and > 0 in fp32. */
int dct_spl_map_fwd(const float* const* probs, int S, int teacher, float tau, float temperature, float eps, float* map, float* kept,
                    int64_t pixels, int C, dct_stream stream);
int dct_spl_map_bwd(const float* const* probs, int S, int teacher, float tau, float temperature, float eps, const float* dmap,
                    float* const* dprobs, int64_t pixels, int C, dct_stream stream);
/* dct_pl_logits_step's contract (workspace, out2, probs, dlogits, two launches) with the sharpened teachers */
int dct_spl_logits_step(const float* const* logits, int S, int teacher, float tau, float temperature, float eps, int64_t pixels, int C,
                        float* out2, float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate,
                        void* workspace, size_t workspace_bytes, dct_stream stream);
/* ---- softmax-MSE consistency: every view is pulled towards the other views' (or the mean) prediction by the squared distance ----
 * Per pixel: S views (1 <= S <= 8) with fp32 probabilities p_s[0..C), C in 2..8, a teacher mode (DCT_PL_CROSS, S >= 2, or DCT_PL_ENSEMBLE,
 * S >= 1) and a confidence threshold tau >= 0.  There is no eps: nothing is divided and no logarithm is taken.
 * Teachers are constants: no gradient flows through a teacher vector, a confidence or a mask.  Everything below is fp32.
 *
 * The first maximum k, the confidence and the mask m are dct_pl_*'s, bit for bit:
 *   cross     teacher j is p_j,  k_j = first maximum of p_j,  m_j = (p_j[k_j] >= tau)
 *   ensemble  sum = ((p_0 + p_1) + ...), added in view order,  k = first maximum of the unscaled sums,
 *             q[c] = sum[c] * (1.f / (float)S),  m = (q[k] >= tau);  the student's own share inside q is held constant too.
 * Student i:  cross     e_ij[c] = p_i[c] - p_j[c],   a_i = sum over j != i, in ascending j, of m_j * (e_ij[0]^2 + ... + e_ij[C-1]^2)
 *                       d map / d p_i[c] = 2 w * sum over j != i, in ascending j, of m_j * e_ij[c],         w = 1.f / (float)(C S (S - 1))
 *             ensemble  e_i[c] = p_i[c] - q[c],      a_i = m * (e_i[0]^2 + ... + e_i[C-1]^2)
 *                       d map / d p_i[c] = 2 w * m * e_i[c],                                                w = 1.f / (float)(C S)
 *   map = w * (a_0 + a_1 + ...), added in view order.
 *   Every e is formed as the difference of two probabilities, never as a total minus the student's own share: (t_0 + t_1) - t_0 is not
 *   t_1 (see dct_spl_*), and views that agree bit for bit must give a value and every gradient of exactly 0.
 *   Contraction: every square is a ROUNDED product, added in class order; the sums over j and i are chains of rounded adds, each starting
 *   from 0; 2 w is exact and its product with the sum of differences is rounded once.  No multiply of this rule folds into an add.
 * From logits: p_s = softmax(x_s) with dct_softmax_fwd's bits; d / d x_i[c] = g * p_i[c] * (d_i[c] - sum_c' d_i[c'] p_i[c']), g = gscale[0] * gmul / P
 * (gscale NULL: 1); accumulate rounds, then adds.
 * The mean is over all P pixels, never over the kept ones.  kept is dct_pl_*'s kept fraction and kept map, unchanged in meaning.
 * Consequences:
 *   - every pixel's map value lies in [0, 2 / C]: two points of the simplex are at most sqrt(2) apart, and w counts the terms;
 *   - two one-hot views of different classes give exactly 2 / C under the cross teacher with S = 2 (4 w, a power of two times w);
 *   - views that agree bit for bit give a value and every gradient of exactly 0: under the cross teacher at any S, under the ensemble
 *     teacher at S = 1 and 2, where sum and q are exact (from three views on the fp32 mean of equal numbers may differ from them in the
 *     last bit);
 *   - with everything masked, the value and every gradient are exactly 0;
 *   - S = 1 with the ensemble teacher is exactly 0 (q = p * 1.f).
 * Status codes are dct_pl_*'s without the eps cases: DCT_ERR_BAD_ARG for S outside the mode's range, an unknown mode, a negative or NaN
 * tau, a null pointer (an entry of a pointer array included), pixels < 1; DCT_ERR_UNSUPPORTED for C outside 2..8; DCT_ERR_WORKSPACE as
 * dct_jsd_logits_step. */
int dct_mse_map_fwd(const float* const* probs, int S, int teacher, float tau, float* map, float* kept, int64_t pixels, int C,
                    dct_stream stream);
int dct_mse_map_bwd(const float* const* probs, int S, int teacher, float tau, const float* dmap, float* const* dprobs, int64_t pixels,
                    int C, dct_stream stream);
/* dct_pl_logits_step's contract (workspace, out2, probs, dlogits, two launches) with the squared distances */
int dct_mse_logits_step(const float* const* logits, int S, int teacher, float tau, int64_t pixels, int C, float* out2,
                        float* const* probs, const float* gscale, float gmul, float* const* dlogits, int accumulate,
                        void* workspace, size_t workspace_bytes, dct_stream stream);
/* out[0] = mean_pix sum_c y*(log(y+eps)-log(p+eps)), p = softmax(p_logits), y = softmax(y_logits) */
int dct_kl_logits_fwd(const float* p_logits, const float* y_logits, int64_t pixels, int C, float eps,
                      float* out1, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_kl_logits_bwd(const float* p_logits, const float* y_logits, int64_t pixels, int C, float eps,
                      const float* gscale, float gmul, float* dp_logits, int accumulate, dct_stream stream);
/* cls[pix] = argmax_c x[pix][c] (first max), int64  (AEGenerator.py:25 pseudo-labels; Dice one-hot) */
int dct_argmax(const float* x, int64_t* cls, int64_t pixels, int C, dct_stream stream);

/* ---- K11: FGSM tail  x_adv = x + eps*sign(g), noise = eps*sign(g) (AEGenerator.py:35-51) ---- */
int dct_fgsm_step(const float* x, const float* g, float eps, float* x_adv, float* noise, int64_t n,
                  dct_stream stream);

/* ---- VAT: virtual adversarial examples (Miyato et al., "Virtual Adversarial Training"; the reference's VATGenerator,
 * generalframework/utils/AEGenerator.py:54-119, which is broken as written -- SURVEY row 4 -- so the rule is restated here) ----
 * The label-free generator of the adversarial term: the direction in which the prediction itself moves fastest, measured by the
 * KL(clean || perturbed) the adversarial term already uses, scaled to an L2 ball per image.
 *
 * x: fp32 [N, Cin, H, W], per = Cin * H * W, f: a network that returns logits, xi > 0, eps > 0, ip >= 1.
 *   1. l = f(x), the clean logits, held constant; softmax(l) is the target of every KL below and is returned too.
 *   2. d = a direction the caller supplies, or else Gaussian noise: flat element e of the [N * per] tensor takes word e & 3 of
 *      philox4x32_10(seed, (call << 40) + (e >> 2)) (the dropout kernels' generator).  Words (r0, r1) and (r2, r3) give two normals
 *      each by Box-Muller: u1 = ((ra >> 8) + 1) * 2^-24 in (0, 1], u2 = (rb >> 8) * 2^-24 in [0, 1), rho = sqrtf(-2 logf(u1)),
 *      even element rho * cosf(2 pi u2), odd element rho * sinf(2 pi u2); the precise functions, never the fast intrinsics.
 *   3. ip times:  u = d / ||d||_n;  l^ = f(x + xi * u);  d = dD / d(x + xi * u), D = the mean over pixels of
 *      KL(softmax(l) || softmax(l^)): dct_kl_logits_fwd / dct_kl_logits_bwd with p = l^, y = l.
 *   4. r = eps * d / ||d||_n,  x_adv = x + r.  The result is (x_adv, r, softmax(l)).
 * ||d||_n is the L2 norm of sample n over its per elements; the sum of squares is taken in float64 in an order fixed by (N, per) alone.
 * There is NO additive epsilon: at xi = 1e-6 a three-channel toy net gave gradient norms of 5e-9, which the usual + 1e-8 would shrink
 * threefold.  A sample whose norm is 0 or not finite gets a zero perturbation: x_adv = x exactly, r = 0.
 * Only the direction of d is used in step 3, so the KL logit gradient there carries the step's loss scale and never lambda_adv (which
 * may be 0).
 * Every forward pass of the generator is an ordinary training-mode pass of f, as FGSM's is: dropout draws a fresh mask, BatchNorm uses
 * the batch statistics and updates the running statistics.
 *
 * The launches.  A sample is cut into dct_vat_workspace_bytes(N, per) / (8 N) blocks, a function of per alone (at most 64); the
 * workspace holds one float64 partial sum of squares per block.  Thread, lane, wave and block order are fixed, so the same tensor gives
 * the same bits, and dct_vat_noise leaves the partials dct_vat_sumsq would leave for the d it wrote.  16-byte accesses where a sample's
 * first element is 16-byte aligned (an odd per misaligns every second sample), scalar ones there and on the tail.
 *   dct_vat_noise:   d = the noise of rule 2 and its partials in one pass.  call = calls ? calls[0] + 1 : offset; the launch only READS
 *                    calls[0] (a 64-bit word on the device), so a captured step draws fresh noise on every replay once the word moves.
 *   dct_vat_sumsq:   the partials of g (the input gradient of step 3).
 *   dct_vat_perturb: every block folds its sample's partials in the one fixed order -- all blocks of a sample get the same scale bit
 *                    for bit, no finalize launch between -- and writes x_out = x + s * d, r_out = s * d (nullable), s =
 *                    (float)(radius / norm), product and sum rounded separately; norms_out (nullable): float64 [N].  calls_advance
 *                    (nullable): thread 0 of block 0 stores calls_advance[0] + 1; no block of this launch reads that word.  Pass it to
 *                    the first perturb launch behind a noise launch only.  (The dropout counter's two-word scheme needs an even number
 *                    of launches per captured step; a step holds ONE noise launch.)
 * DCT_ERR_BAD_ARG: a null d / g / x / x_out / workspace, N or per < 1, more than 2^42 elements, a pointer off its type's alignment, a
 * radius that is not positive and finite; DCT_ERR_WORKSPACE: less than dct_vat_workspace_bytes(N, per) (0 for a shape out of range). */
size_t dct_vat_workspace_bytes(int64_t N, int64_t per);
int dct_vat_noise(float* d, int64_t N, int64_t per, uint64_t seed, const uint64_t* calls, uint64_t offset, void* workspace,
                  size_t workspace_bytes, dct_stream stream);
int dct_vat_sumsq(const float* g, int64_t N, int64_t per, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_vat_perturb(const float* x, const float* d, double radius, int64_t N, int64_t per, const void* workspace,
                    size_t workspace_bytes, float* x_out, float* r_out, double* norms_out, uint64_t* calls_advance,
                    dct_stream stream);

/* ---- K12: Adam over one flat fp32 buffer (torch.optim.Adam, segmentators.py:41; step :248) --
 * g' = grad_scale*g + wd*p; m = m + (g'-m)*(1-b1); v = v*b2 + (1-b2)*g'^2;   (grad_scale: 1, or the inverse of the
 * power-of-two loss-gradient scale of an fp16 step)
 * p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)     (host passes step_size = lr/bc1, bc2_sqrt;
 * betas are doubles so that 1-beta is formed in double and then rounded, as torch does)
 * bf16_shadow (nullable): also writes the updated p rounded to bf16 at the same index. */
int dct_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float step_size,
                  float bc2_sqrt, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                  void* bf16_shadow, dct_stream stream);
/* Same update with the step-dependent scalars in device memory: state = {step count t, learning rate,
 * table base, table length} (four doubles), table (nullable) = {1 - beta1^t, sqrt(1 - beta2^t)} double pairs the
 * host computed for steps t = base+1 .. base+length.  Stream-ordered: t += 1, then the pair for step t is read from
 * the table (bit-identical to dct_adam_flat with the same host scalars); outside the table it is formed on
 * the device in double: step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t).  No per-step host
 * scalar, so the launch can be replayed from a captured HIP graph (torch.optim.Adam's `capturable` mode is
 * the reference-side analogue). */
int dct_adam_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, double* state,
                      const double* table, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                      void* bf16_shadow, dct_stream stream);

/* The guard in front of the update: gradient-norm clipping (torch.nn.utils.clip_grad_norm_) and the skipped step of a non-finite
 * gradient (torch.cuda.amp.GradScaler), decided and consumed on the device so that the step stays one replayable graph.
 *
 * dct_grad_sumsq: workspace[b] = the sum of g[i]^2 over block b's elements, squared and added in DOUBLE (a finite fp32 squared is exact
 * and cannot overflow there: the sum is non-finite iff some g[i] is inf or NaN; 1e30 is a large gradient, not an overflow).  The number
 * of blocks, dct_grad_sumsq_workspace_bytes(n) / 8 = clamp(ceil(floor(n / 4) / 256), 1, 2048), depends on n alone and every fold has a
 * fixed order (no float atomics): the same buffer gives the same bits on every run, eager or replayed.  g and workspace as below.
 *
 * dct_adam_flat_dev_guarded: three stream-ordered launches.  (1) dct_grad_sumsq into `workspace`.  (2) One block folds the partials in
 * double (thread t of 256 adds partials t, t + 256, ... in ascending order, a halving tree folds the 256 sums) and writes `guard`:
 *     norm = |grad_scale| * sqrt(sum)     the norm of the gradient the update sees (of the averaged one when grad_scale carries 1 / world)
 *     skip = skip_nonfinite && !isfinite(sum);   skipped += skip
 *     coef = 1 when clip == 0 or skip, else (float)min(1, max_norm / (norm + 1e-6)) formed in double, with max_norm READ FROM THE RECORD
 *            (a schedule of it is one async fill, never a recapture); a NaN quotient stays NaN and an infinite norm gives 0, as in torch;
 *            clipped += the quotient is not >= 1
 *     state[0] += 1 unless skip           (torch does not count a skipped step)
 * (3) The update of dct_adam_flat_dev with grad_scale * coef (one fp32 multiply) in grad_scale's place -- weight decay is added after
 * the clip, as in torch -- or, when skip, nothing: p, m, v and the shadow keep every bit.  With clip == 0 and skip_nonfinite == 0, or
 * with a max_norm that is never reached, p, m, v, the shadow and state[0] are bit-identical to dct_adam_flat_dev's.
 * The caller zeroes the record once, sets max_norm and leaves the rest to the device.
 * DCT_ERR_BAD_ARG: a null pointer (bf16_shadow and table may be null), n < 1; DCT_ERR_UNSUPPORTED: p, g, m, v not 16-byte aligned,
 * state, workspace or guard not 8-byte aligned; DCT_ERR_WORKSPACE: less than dct_grad_sumsq_workspace_bytes(n). */
typedef struct dct_adam_guard {
  double   norm;      /* out: gradient norm of the last step */
  double   max_norm;  /* in:  clipping threshold (read when clip != 0) */
  float    coef;      /* out: the factor the last step put on its gradients */
  uint32_t skip;      /* out: 1 when the last step was skipped */
  uint64_t skipped;   /* running totals since the caller zeroed the record */
  uint64_t clipped;
} dct_adam_guard;     /* 40 bytes */
size_t dct_grad_sumsq_workspace_bytes(int64_t n);
int dct_grad_sumsq(const float* g, int64_t n, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_adam_flat_dev_guarded(float* p, const float* g, float* m, float* v, int64_t n, double* state,
                              const double* table, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                              void* bf16_shadow, void* workspace, size_t workspace_bytes, dct_adam_guard* guard,
                              int skip_nonfinite, int clip, dct_stream stream);

/* ---- K2/K3/K4/K6/K7/K8: Enet layers (arch/enet.py:8-243) -------------------------------------
 * Enet's widths are 1..128 channels (internal 3/16/32): HBM- and launch-bound, so these are direct
 * fused kernels, not GEMMs.  Every consumer reads its input through the producer's BatchNorm +
 * activation ("normalise on load"): in = act(scale[c]*raw + shift[c]); mode 0 none, 1 affine,
 * 2 affine+PReLU(slope[c]), 3 affine+ReLU.  All per-channel vectors are fp32 device arrays. */
typedef struct dct_enet_tf {
  const float* scale; const float* shift; const float* slope;
  int32_t mode;
} dct_enet_tf;

/* Every Enet entry point takes `dtype` (the storage type T of the bf16/f32 activations) and an
 * `f32_mask`: bit k set = the k-th dct_view argument of that call (in declaration order) is stored
 * in fp32 regardless of `dtype`.  In bf16 mode the RAW conv outputs stay fp32 (BatchNorm subtracts
 * their mean, which would cancel most of bf16's 8 mantissa bits); block outputs and gradients are T. */

/* Generic small-channel convolution (<= 128 channels each side).  Replaces nn.Conv2d /
 * nn.ConvTranspose2d of enet.py:21,52-109 and both of their data gradients:
 *   direct:      y[oy,ox,o] = sum W(o,r,s,i) * in[oy*stride - pad + r*dil, ..., i]
 *   transposed:  y[oy,ox,o] = sum W(o,r,s,i) * in[(oy + pad - r*dil)/stride, ..., i]   (where divisible)
 * with W(o,r,s,i) = w[o*ws_out + (r*S+s)*ws_tap + i*ws_in] (fp32 master weights, any role).
 * Epilogue: + bias[o] -> + resid_grad*[resid_mask > 0] (residual-branch gradient of a bottleneck)
 * -> (+= y when d->accumulate).  f32_mask bits: 0 x, 1 y, 2 resid_grad, 3 resid_mask. */
int dct_enet_conv(const dct_view* x, const float* w, const float* bias, const dct_enet_tf* tf,
                  const dct_view* y, const dct_conv_desc* d, int transposed,
                  int ws_out, int ws_tap, int ws_in,
                  const dct_view* resid_grad, const dct_view* resid_mask,
                  int f32_mask, int dtype, dct_stream stream);
/* The same convolution (no residual gate) with the consumer BatchNorm's batch statistics riding along: where the MFMA form is
 * taken (bf16 / f16, >= 16 input channels) and the output has <= stats_capacity_rows tiles of 32 pixels, every tile writes
 * its per-channel {sum, sum of squares, 0} as doubles to stats_partial[tile][y.c][3] and *stats_rows = the tile count;
 * dct_enet_bn_fwd_stats_rows(..., workspace = stats_partial, partial_rows = *stats_rows) then only folds them.  Otherwise
 * *stats_rows = 0 and the statistics need the usual reduction. */
int dct_enet_conv_stats(const dct_view* x, const float* w, const float* bias, const dct_enet_tf* tf,
                        const dct_view* y, const dct_conv_desc* d, int transposed,
                        int ws_out, int ws_tap, int ws_in, int f32_mask, int dtype,
                        double* stats_partial, int stats_capacity_rows, int* stats_rows, dct_stream stream);

/* nn.BatchNorm2d bookkeeping for all layers of a network in one launch: layer k (record k of records_dev)
 *   { float* running_mean; float* running_var; int64* num_batches_tracked (nullable); int32 c, mean_off, var_off, pad; }  (40 bytes)
 * gets r <- (1 - momentum) r + momentum * stats[off + i] for both running statistics (stats: the flat buffer a forward pass
 * left its batch means / UNBIASED variances in) and num_batches_tracked += 1 -- what F.batch_norm does per call in the
 * reference (arch/enet.py:22,55-122).  Replaces four torch._foreach launches per forward pass. */
int dct_bn_running_update(const void* records_dev, int n_layers, const float* stats, float momentum, dct_stream stream);
/* out = a + b (+ c if non-NULL) over n floats (n % 4 == 0, 16-byte aligned): the per-pass flat gradient buffers of one model,
 * added in pass order -- ((labeled + unlabeled) + adversarial), bit for bit the in-place accumulation of sequential passes. */
int dct_flat_sum(float* out, const float* a, const float* b, const float* c, long long n, dct_stream stream);
/* x *= scale over n floats (any 4-byte aligned pointer, any n >= 1): the 1/world of a gradient average after a SUM all-reduce
 * (ddp.py::FlatGradSync, for models whose optimizer does not fold the factor into its update). */
int dct_flat_scale(float* x, float scale, long long n, dct_stream stream);

size_t dct_enet_reduce_workspace_bytes(int channels);
/* nn.BatchNorm2d(eps 1e-3, momentum 0.1) forward statistics of a raw conv output (enet.py:22,55-122):
 * training: batch mean / biased var (double accumulation, fixed-order fold), running stats updated
 * with the unbiased var; eval: running stats.  Writes scale = gamma*invstd, shift = beta - mean*scale
 * (what consumers apply on load) and save_mean / save_invstd for the backward.  f32_mask bit 0: raw.
 * Deferred running statistics: with running_mean = running_var = NULL in training mode nothing is updated and save_var
 * (nullable) receives the batch's UNBIASED variance, so that the caller can apply r = (1 - momentum) r + momentum b for
 * several forward passes later, in the reference's order (the passes themselves may then run concurrently). */
int dct_enet_bn_fwd_stats(const dct_view* raw, const float* gamma, const float* beta, float eps, float momentum,
                          float* running_mean, float* running_var, int training,
                          float* scale, float* shift, float* save_mean, float* save_invstd, float* save_var,
                          int f32_mask, int dtype, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_enet_bn_fwd_stats_rows(const dct_view* raw, const float* gamma, const float* beta, float eps, float momentum,
                               float* running_mean, float* running_var, int training,
                               float* scale, float* shift, float* save_mean, float* save_invstd, float* save_var,
                               int f32_mask, int dtype, void* workspace, size_t workspace_bytes, int partial_rows, dct_stream stream);
/* Backward of act(BN(raw)) given g = grad wrt the activation output (optionally gated by
 * g_mask > 0, the ReLU of the bottleneck sum): dgamma/dbeta/dslope += ..., and
 * draw = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) (training; eval mode: gamma*invstd*dz with the
 * running statistics).  c1c2: 2*C floats of scratch.  f32_mask bits: 0 raw, 1 g, 2 g_mask, 3 draw. */
int dct_enet_bn_bwd(const dct_view* raw, const dct_view* g, const dct_view* g_mask,
                    const float* scale, const float* shift, const float* slope, int act,
                    const float* mean, const float* invstd,
                    float* dgamma, float* dbeta, float* dslope, float* c1c2, int training,
                    const dct_view* draw, int f32_mask, int dtype, void* workspace, size_t workspace_bytes,
                    dct_stream stream);
int dct_enet_bn_bwd_rows(const dct_view* raw, const dct_view* g, const dct_view* g_mask,
                         const float* scale, const float* shift, const float* slope, int act,
                         const float* mean, const float* invstd,
                         float* dgamma, float* dbeta, float* dslope, float* c1c2, int training,
                         const dct_view* draw, int f32_mask, int dtype, void* workspace, size_t workspace_bytes,
                         int partial_rows, dct_stream stream);
/* The data-gradient convolution y = dgrad(x) whose output is the gradient wrt act(BN(bn_raw)) of the producing layer, with that
 * BatchNorm's backward sums riding along (MFMA form only, as dct_enet_conv_stats): every tile of 32 pixels writes
 * {sum dz, sum dz xhat, sum g z [z<0]} per channel to stats_partial[tile][y.c][3]; dct_enet_bn_bwd_rows(..., workspace =
 * stats_partial, partial_rows = *stats_rows) then skips its reduction launch.  *stats_rows = 0: nothing written. */
int dct_enet_conv_bnbwd_stats(const dct_view* x, const float* w, const dct_view* y, const dct_conv_desc* d, int transposed,
                              int ws_out, int ws_tap, int ws_in, int f32_mask, int dtype,
                              const dct_view* bn_raw, const float* bn_scale, const float* bn_shift, const float* bn_slope, int bn_act,
                              const float* bn_mean, const float* bn_invstd,
                              double* stats_partial, int stats_capacity_rows, int* stats_rows, dct_stream stream);
/* out[c] += sum over pixels of x[.., c]   (bias gradients).  f32_mask bit 0: x. */
int dct_enet_channel_sum(const dct_view* x, float* out, int f32_mask, int dtype, void* workspace, size_t workspace_bytes,
                         dct_stream stream);
/* Bottleneck tail out = relu(main + act(bn(raw))) (enet.py:132-149), mode:
 *   0 regular: main = main_in;   1 down: main = maxpool2x2(main_in) zero-padded to out.c channels,
 *   argmax codes written to idx [N,h,w,idx_channels];   2 up: main = max_unpool(bn(rawm)) by idx;
 *   3 initial block (enet.py:26-30): out = cat(prelu(bn(raw)), maxpool2x2(main_in = the image)).
 * f32_mask bits: 0 raw, 1 main_in, 2 rawm, 3 out. */
int dct_enet_tail_fwd(const dct_view* raw, const dct_enet_tf* tf, const dct_view* main_in,
                      const dct_view* rawm, const dct_enet_tf* tfm, uint8_t* idx, int idx_channels,
                      int mode, const dct_view* out, int f32_mask, int dtype, dct_stream stream);
/* Main-branch gradient of those tails: 1 down -> dst = routed grad at double resolution;
 * 2 up -> dst = grad of bn(rawm) (gather); 3 initial -> dst (image grad) (+)= pooled-channel grad
 * (out_mask = the input image).  f32_mask bits: 0 dout, 1 out_mask, 2 dst. */
int dct_enet_tail_bwd(const dct_view* dout, const dct_view* out_mask, const uint8_t* idx, int idx_channels,
                      int mode, int accumulate, const dct_view* dst, int f32_mask, int dtype, dct_stream stream);
/* dw[a.c][R][S][b.c] += sum_pixels tfa(a[p]) (x) tfb(b[p*stride - pad + tap*dil]).
 * Conv2d: a = draw, b = layer input; ConvTranspose2d: a = layer input, b = dy.  f32_mask bits: 0 a, 1 b. */
size_t dct_enet_wgrad_workspace_bytes(const dct_view* a, const dct_view* b, const dct_conv_desc* d);
int dct_enet_wgrad(const dct_view* a, const dct_enet_tf* tfa, const dct_view* b, const dct_enet_tf* tfb,
                   float* dw, const dct_conv_desc* d, int f32_mask, int dtype,
                   void* workspace, size_t workspace_bytes, dct_stream stream);

/* ---- K6 for the BatchNorm'd UNet: nn.BatchNorm2d(C) + ReLU (arch/network.py:138-146,181-183,243-290) -------------------
 * C a power of two, 8 <= C <= 2048; dense-channel NHWC views with 16-byte aligned rows.  Forward: batch statistics of `raw`
 * (training; double accumulation, fixed-order fold; running statistics updated with the unbiased variance) or the running
 * statistics (eval) -> scale = gamma * invstd, shift = beta - mean * scale, save_mean / save_invstd (nullable), and
 * y = relu?(scale * raw + shift) when y != NULL.  Backward: g = gradient wrt y;
 * dgamma / dbeta (= | +=, nullable) and draw = scale * (dz - mean(dz) - xhat * mean(dz * xhat)), dz = g * [y > 0] when relu
 * (eval mode: draw = scale * dz).  c1c2: 2 * C floats of scratch. */
size_t dct_bn_workspace_bytes(int channels);
int dct_bn_fwd(const dct_view* raw, const float* gamma, const float* beta, float eps, float momentum,
               float* running_mean, float* running_var, int training,
               float* scale, float* shift, float* save_mean, float* save_invstd,
               const dct_view* y, int relu, int dtype, void* workspace, size_t workspace_bytes, dct_stream stream);
int dct_bn_bwd(const dct_view* raw, const dct_view* g, const float* scale, const float* shift,
               const float* mean, const float* invstd, float* dgamma, float* dbeta, int accumulate,
               float* c1c2, int training, int relu, const dct_view* draw, int dtype,
               void* workspace, size_t workspace_bytes, dct_stream stream);

/* ---- Dice accumulation on device (metrics/dice_meter.py:12-83) ----------------------------
 * inter[b][c], psum[b][c], gsum[b][c] (int32, zeroed by caller) from logits argmax vs gt. */
int dct_dice_counts(const float* logits, const int64_t* gt, int B, int64_t pixels_per_image, int C,
                    int32_t* inter, int32_t* psum, int32_t* gsum, dct_stream stream);

/* Dice rows of one DiceMeter.add from those counts (2-D: one row per slice; 3-D: one row for the batch) and the meter's
 * running sums in the same launch: dice[rows][C] fp32; acc (double [2][C+1], caller-zeroed once) += value, value^2 per class and,
 * in column C, for the row mean over the report axes (bit c of axes_mask).  B <= 64, C <= 8. */
int dct_dice_update(const int32_t* inter, const int32_t* psum, const int32_t* gsum, int B, int C, int method3d,
                    uint32_t axes_mask, float smooth, float* dice, double* acc, dct_stream stream);

/* ---- Hausdorff distance on device (the HD column of the result tables of Summary.py:70-252) -------------------
 * The reference takes it from the external `deepclustering` package; the rule here is medpy's metric.binary.hd, per class c and
 * per "row" (2-D: one slice; method3d: the whole batch as a volume):
 *   P = pixels whose argmax is c (first maximum, as dct_argmax / dct_dice_counts); G = pixels with gt == c.  A gt value outside
 *   [0, C) belongs to no class.
 *   Surface of a mask = its pixels with a background neighbour among the 4 in-plane (2-D) / 6 (3-D) neighbours; everything outside
 *   the array is background (a mask that fills the image has its frame as surface).
 *   d2(p, q) = (sz dz)^2 + (sy dy)^2 + (sx dx)^2 (2-D ignores sz);  hd2 = max( max_{p in dP} min_{q in dG} d2, max_{q in dG} min_{p in dP} d2 ).
 * hd2[rows][C] (rows = method3d ? 1 : B) receives the SQUARED distance, NaN where P or G is empty (medpy raises there).
 * Exact separable distance transform (csrc/surface.hip): the cost does not depend on the masks.  fp32 on squared distances: with
 * unit spacing every intermediate is an integer below 2^24 and the result is exact; it is bit-identical from run to run.
 * logits, gt and workspace 16-byte aligned; the workspace needs no clearing by the caller.  DCT_ERR_BAD_ARG: null pointer, size < 1,
 * spacing <= 0; DCT_ERR_UNSUPPORTED: C > 8, H or W > 1024, B > 256 in 3-D (B > 65535 in 2-D); DCT_ERR_WORKSPACE: workspace too
 * small.  dct_hausdorff_workspace_bytes returns 0 for a shape dct_hausdorff refuses. */
size_t dct_hausdorff_workspace_bytes(int B, int H, int W, int C, int method3d);
int dct_hausdorff(const float* logits /*[B][H][W][C]*/, const int64_t* gt /*[B][H][W]*/,
                  int B, int H, int W, int C, int method3d, float sz, float sy, float sx,
                  float* hd2 /*[rows][C]*/, void* workspace, size_t workspace_bytes, dct_stream stream);

/* ---- Largest connected component on device (the cleaning every ACDC-style pipeline applies before it scores: Hausdorff distance
 * is a maximum, and one stray island far from the organ sets it) -------------------
 * Row: one slice (2-D), or the whole batch taken as a volume with z = batch index (method3d) -- the convention of dct_hausdorff.
 * Class of a pixel: the argmax of its logits, first maximum, exactly as dct_argmax / dct_dice_counts / dct_hausdorff.
 * Connected: two pixels of the same class in the same row that are neighbours.  full = 0: face neighbours (4 in a plane, 6 in a
 *   volume); full = 1: all neighbours that share a face, an edge or a corner (8 / 26).  Nothing outside the array is a neighbour.  (A
 *   volume's 18-neighbourhood is not offered.)
 * Component: a maximal connected set of pixels of one class.
 * Kept: for every row and every class c with bit c set in class_mask, the component with the most pixels; ties go to the component
 *   whose first pixel in raster order (z, y, x) comes first -- what np.argmax over the sizes of scipy.ndimage.label's labels gives,
 *   scipy numbering components in that order.  Every pixel of class c outside the kept component becomes class `background`; pixels
 *   of classes outside class_mask are left alone.  `background` itself may not be in class_mask.
 * Outputs: onehot[B][H][W][C] (nullable) = 1.0 at the cleaned class, 0.0 elsewhere (the form every meter takes: for them only the
 *   argmax matters); cls[B][H][W] (nullable) = the cleaned class map; stats[rows][C][3] (nullable, rows = method3d ? 1 : B) =
 *   {components of class c before cleaning, size of the largest, pixels of class c before cleaning}, for every class, in class_mask
 *   or not; 0, 0, 0 for an absent class.
 * Union-find over pixels with 32-bit labels (csrc/components.hip); integer sums, maxima and minima only: exact, and bit-identical
 * from run to run.  Everything runs on the caller's stream, nothing waits for the device; the workspace needs no clearing by the
 * caller.  logits, onehot and workspace 16-byte aligned, cls 8-byte, stats 4-byte.
 * DCT_ERR_BAD_ARG: a null logits or workspace, onehot and cls both null, a size < 1, full not 0 or 1, background outside [0, C),
 * class_mask with a bit at background or at C and above, a misaligned pointer; DCT_ERR_UNSUPPORTED: C > 8, a row of 2^31 pixels or
 * more (labels are 32-bit pixel indices), B >= 2^27; DCT_ERR_WORKSPACE: workspace too small.  dct_components_workspace_bytes returns 0
 * for a shape dct_largest_component refuses. */
size_t dct_components_workspace_bytes(int B, int H, int W, int C, int method3d);
int dct_largest_component(const float* logits /*[B][H][W][C]*/, int B, int H, int W, int C, int method3d, int full,
                          uint32_t class_mask, int background,
                          float* onehot /*[B][H][W][C], nullable*/, int64_t* cls /*[B][H][W], nullable*/,
                          int32_t* stats /*[rows][C][3], nullable*/, void* workspace, size_t workspace_bytes, dct_stream stream);

/* ---- Agreement between raters on device: pairwise confusion matrices (the kappa table of Summary.py:70-252, which takes
 * cohen_kappa_score from scikit-learn; the same counts give the reference's ConfusionMatrix and IoU meters) -------------------
 * Raters: the S predictions are raters 0..S-1; the class of a pixel is the argmax of its logits, first maximum, exactly as
 *   dct_argmax / dct_dice_counts.  When gt != NULL, gt is rater S.  R = S + (gt ? 1 : 0).
 * Pairs: (i, j) with i < j in lexicographic order: p = i (2R - i - 1) / 2 + (j - i - 1); P = R (R - 1) / 2.
 * Counts: counts[b][p][a][c] (int32) += the number of pixels of image b where rater i says class a and rater j says class c.  A
 *   pixel whose gt value is outside [0, C) (255, negative, >= C) is counted in no pair that contains gt, and still in every
 *   prediction-against-prediction pair.
 * Derived quantities are host arithmetic in float64 on a matrix M with n = sum M, both unweighted:
 *   kappa = (po - pe) / (1 - pe), po = tr M / n, pe = sum_k row_k col_k / n^2; NaN when n = 0 or pe = 1 (scikit-learn's
 *   cohen_kappa_score gives NaN in the same cases).
 *   IoU_c = M[c][c] / (row_c + col_c - M[c][c]), NaN where that denominator is 0.
 *   kappa restricted to the pixels whose SECOND rater lies in a class set = kappa of M with the other columns zeroed (the
 *   reference's considered_classes on the target): the kernel needs no mask argument.
 * One launch reads every pixel of every rater once ((4 C S + 8) bytes per pixel); integer sums: bit-identical from run to run.
 * logits: S host-side entries, each a device [B][pixels][C] fp32 tensor aligned to its pixel (16 bytes at C = 4, 8 at C = 2, else
 * 4); counts is zeroed by the caller (or holds earlier counts: the call adds).  No workspace.
 * DCT_ERR_BAD_ARG: a null logits / entry / counts, a misaligned pointer, S < 1, B < 1, pixels < 1, R < 2 (S = 1 without gt);
 * DCT_ERR_UNSUPPORTED: S > 8, C < 1 or C > 8, pixels_per_image >= 2^31 (a per-image count must fit int32), B > 65535. */
int dct_confusion_counts(const float* const* logits, int S, const int64_t* gt /*[B][pixels], nullable*/,
                         int B, int64_t pixels_per_image, int C, int32_t* counts /*[B][P][C][C]*/, dct_stream stream);

/* ---- Calibration on device: reliability tables, and the sums behind the Brier score and the negative log-likelihood ----------
 * Inputs: S tensors probs[s] = [B][pixels][C] in fp32, 1 <= S <= 8, 1 <= C <= 8; gt as int64.  With from_logits each view first
 *   becomes p = softmax(x) in fp32: m = max_c x_c, e_c = expf(x_c - m), p_c = e_c / sum_c e_c (the sum in class order).  Everything
 *   below is a function of the fp32 p only; without from_logits the inputs are taken to be probabilities (in [0, 1]) as they are.
 * Raters: the S views in order.  With with_ensemble one more rater follows: p_ens = (p_0 + p_1 + ...) / S, summed in view order in
 *   fp32, one fp32 division (exact when S is a power of two).  R = S + with_ensemble.
 * Which pixels count: those with 0 <= gt < C and bit gt of class_mask set (bits at C and above mean nothing) -- the "second rater
 *   lies in this class set" convention of kappa above; 255, negative and >= C never count.
 * Per counted pixel and rater: conf = max_c p_c; pred = the first maximum, exactly as dct_argmax / dct_confusion_counts;
 *   correct = (pred == gt); bin = min(n_bins - 1, (int)(conf * (float)n_bins)), one fp32 multiply, 1 <= n_bins <= 32 (a negative
 *   or NaN conf goes to bin 0); brier = sum_c (p_c - [c == gt])^2; nll = -logf(p_gt + 1e-10f).
 * What is stored, all integers, so that the sums are order-independent and bit-identical from run to run:
 *   bins[b][r][k][3] (int64) += {pixels, correct pixels, sum of (uint32)(conf * 2^24)} of bin k;
 *   scores[b][r][2] (int64) += {sum of (int64)(brier * 2^24), sum of (int64)(nll * 2^24)}.
 *   The truncation loses less than 2^-24 per pixel; for conf >= 0.5 the scaling is exact.  For probabilities every word fits 32 bits
 *   (brier <= 2, nll <= -log(1e-10) = 23.03) and is converted as such: an input outside [0, 1] saturates there, a NaN gives 0.
 * Derived, on the host, in float64, for a row (an image, a batch, everything pooled) with N counted pixels and per bin n_k pixels:
 *   acc_k = correct_k / n_k, conf_k = confsum_k / (2^24 n_k); ECE = sum_k (n_k / N) |acc_k - conf_k|; MCE = the maximum of
 *   |acc_k - conf_k| over the non-empty bins; Brier and NLL = the means over the counted pixels; N = 0 gives NaN everywhere.
 *   Coverage and accuracy at a bin's lower edge k / n_bins: the share of the counted pixels in bins >= k, and their accuracy.
 * One launch reads every pixel of every view once ((4 C S + 8) bytes per pixel).  probs: S host-side entries, each a device tensor
 * aligned to its pixel (16 bytes at C = 4, 8 at C = 2, else 4); gt, bins and scores 8-byte aligned; bins and scores are zeroed by
 * the caller (or hold earlier sums: the call adds).  No workspace; nothing waits for the device.
 * DCT_ERR_BAD_ARG: a null probs / entry / gt / bins / scores, a misaligned pointer, S < 1, B < 1, pixels < 1, with_ensemble or
 * from_logits not 0 or 1; DCT_ERR_UNSUPPORTED: S > 8, C < 1 or C > 8, n_bins < 1 or n_bins > 32, B > 65535, pixels_per_image >= 2^31.
 * Both are decided before anything is launched. */
int dct_calibration_counts(const float* const* probs, int S, const int64_t* gt /*[B][pixels]*/, int B, int64_t pixels_per_image,
                           int C, int n_bins, uint32_t class_mask, int with_ensemble, int from_logits,
                           int64_t* bins /*[B][R][n_bins][3]*/, int64_t* scores /*[B][R][2]*/, dct_stream stream);

/* ---- Temperature scaling on device: the sums behind the fit of one temperature per rater, and the scaled probabilities --------
 * Raters: S tensors logits[s] = [B][pixels][C] in fp32, 1 <= S <= 8, 1 <= C <= 8, the views' logits z.  With with_ensemble one more
 *   rater follows whose "logits" are u_c = logf(p_ens_c + 1e-10f), p_ens being exactly the mean of the calibration rule above: each
 *   view's fp32 softmax at temperature 1, summed in view order, one fp32 division by S.  The ensemble is formed first and scaled
 *   afterwards: it is the ensemble rater of dct_calibration_counts.  R = S + with_ensemble.
 * Which pixels count: as above, 0 <= gt < C and bit gt of class_mask set.
 * Candidates: betas[R][K], fp32 on the device, 1 <= K <= 16: inverse temperatures beta = 1 / T, a row per rater.
 * Per counted pixel, rater r and candidate k, with z the rater's logits, y = gt, beta = betas[r][k], everything in fp32:
 *   x_c = beta * z_c (a rounded product); m = max_c x_c; e_c = expf(x_c - m); s = sum_c e_c in class order;
 *   nll = logf(s) - (x_y - m); g = (sum_c e_c * z_c) / s - z_y.
 *   g is d nll / d beta, and its sum over the pixels is non-decreasing in beta (the NLL is convex in beta): the fit is a root
 *   search on a monotone function.  (2 z, beta / 2) gives the same x, hence the same nll words, as (z, beta), and twice the g.
 * What is stored, all integers, so that the sums are order-independent and bit-identical from run to run:
 *   sums[r][k][0] (int64) += rint(min(nll, 4095) * 2^20); sums[r][k][1] += rint(clamp(g, -2047, 2047) * 2^20), signed;
 *   counted[0] (int64) += the number of counted pixels.  rint rounds to nearest, ties to even; a NaN contributes 0.
 * One launch per batch reads every logit once from HBM ((4 C S + 8) bytes per pixel) and evaluates all R K candidates.
 * logits: S host-side entries, each a device tensor aligned to its pixel (16 bytes at C = 4, 8 at C = 2, else 4); gt, sums and counted
 * 8-byte aligned, betas 4-byte; sums and counted are zeroed by the caller (or hold earlier sums: the call adds).  No workspace;
 * nothing waits for the device.
 * dct_temperature_apply writes R fp32 tensors out[r] = [B][pixels][C] (host-side entries, aligned as the logits): for a view the
 *   softmax above (the calibration rule's: max-subtracted, the sum in class order, a true division) of beta_r * z, for the ensemble
 *   the same softmax of beta_R * u.  beta: R floats on the HOST.  At beta = 1 a view's output is the p of dct_calibration_counts'
 *   from_logits, bit for bit.
 * DCT_ERR_BAD_ARG: a null logits / entry / gt / betas / sums / counted / beta / out, a misaligned pointer, S < 1, B < 1, pixels < 1,
 * with_ensemble not 0 or 1; DCT_ERR_UNSUPPORTED: S > 8, C < 1 or C > 8, K < 1 or K > 16, B > 65535, pixels_per_image >= 2^31.
 * Both are decided before anything is launched. */
int dct_temperature_sums(const float* const* logits, int S, const int64_t* gt /*[B][pixels]*/, int B, int64_t pixels_per_image,
                         int C, uint32_t class_mask, int with_ensemble, const float* betas /*[R][K], device*/, int K,
                         int64_t* sums /*[R][K][2]*/, int64_t* counted /*[1]*/, dct_stream stream);
int dct_temperature_apply(const float* const* logits, int S, int B, int64_t pixels_per_image, int C, const float* beta /*[R], host*/,
                          int with_ensemble, float* const* out /*R entries*/, dct_stream stream);

/* ---- per-kernel-class timing (bench.py roofline leg) --------------------------------------
 * When enabled every launch made through this library is bracketed by hipEvents on its stream;
 * dct_prof_read synchronises and returns accumulated milliseconds and launch counts per class. */
enum { DCT_PROF_IGEMM = 0, DCT_PROF_WGRAD = 1, DCT_PROF_POINTWISE = 2, DCT_PROF_LOSS = 3,
       DCT_PROF_ADAM = 4, DCT_PROF_OTHER = 5, DCT_PROF_NCLASS = 6 };
int dct_prof_enable(int on);
/* Process-wide tuning / A-B knobs for benchmarking (never needed for correctness; defaults are the
 * shipped configuration). */
enum { DCT_TUNE_IGEMM_SPLIT = 1,   /* >= 1: force the split-K factor; -1 (default): planner's choice */
       DCT_TUNE_WGRAD_CHUNKS = 3,  /* >= 1: force the number of pixel chunks (split-K) of wgrad */
       DCT_TUNE_IGEMM_HALO = 7,    /* 1 (default): shared-halo kernel for 3x3 stride-1 layers on large images; 0: per-tap kernel everywhere
                                      (the reference path of the bit-level cross-checks in tests/test_kernels_gpu.py) */
       DCT_TUNE_WGRAD_ROWS = 8,    /* 1 (default): filter-row weight-gradient kernel (three taps share the x strip); 0: per-tap kernel */
       DCT_TUNE_WGRAD_ROWS_FILL = 9,   /* percent (default 70): minimum fill of the filter-row kernel's 64-pixel K-steps */
       DCT_TUNE_IGEMM_PACKED = 10,     /* 1 (default): packed-rows shared-halo kernel for 3x3 stride-1 layers on small images; 0: per-tap kernel */
       DCT_TUNE_ENET_WGRAD_BLOCKS = 12,/* 1..1024 (default 1024): cap on the pixel chunks (blocks) of dct_enet_wgrad */
       DCT_TUNE_WGRAD_TARGET = 14,     /* >= 64 (default: see wgrad.hip): block target of the per-tap weight-gradient kernel */
       DCT_TUNE_WGRAD3_TARGET = 15,    /* >= 64: block target (4-wave units) of the filter-row weight-gradient kernel */
       DCT_TUNE_IGEMM_SPLIT_TARGET = 16, /* >= 64 (default 450): block target of a split-K conv layer */
       DCT_TUNE_IGEMM_HALO_MIN_BLOCKS = 19,  /* default 400: fewest blocks for which the shared-halo patch kernel is taken */
       DCT_TUNE_IGEMM_HALO_COVER = 20,       /* percent (default 75): least image cover of its 8 x 16 patches */
       DCT_TUNE_IGEMM_PACKED_SPLIT = 23,     /* default 160: packed-rows kernel splits layers with fewer blocks over channel slices */
       DCT_TUNE_IGEMM_PACKED_FILL = 24,      /* percent (default 50; 76 until round 5): least fill of the packed-rows kernel's 128-pixel tiles */
       DCT_TUNE_ENET_MFMA = 26,              /* bf16 / f16 Enet: bit 0 = MFMA form of the convolutions with >= 16 input channels,
                                                bit 1 = of the weight gradients; 3 (default), 0 = the fp32 VALU kernels */
       DCT_TUNE_ENET_MWGRAD_WAVES = 28,      /* >= 64 (default 2048): waves an MFMA weight-gradient launch aims for */
       DCT_TUNE_IGEMM_XCD = 39,              /* 1 (default): the per-tap and packed-rows conv kernels deal the blocks of a weights-heavy layer XCD by XCD
                                                (each weight is fetched into ONE L2 slice); 0: natural 3-D grids; 2: on every layer */
       DCT_TUNE_IGEMM_HALO_TALL = 40,        /* 16 x 16 patches on one halo stage in the shared-halo kernel (two blocks per CU, 32 MFMAs per wave and barrier
                                                round; bit-identical to the 8 x 16 patches): 0 = never, 1 (default) = planner's choice, 2 = every layer the form can run */
       DCT_TUNE_IGEMM_PACKED_RING = 41,      /* lean loop of the packed-rows kernel on one halo stage and a three-slot weight ring (72 KiB; a weight stage is issued two
                                                barrier rounds ahead behind a counted vmcnt; bit-identical): 0 = two halo and two weight stages, 1 (default) =
                                                every packed-rows launch */
       DCT_TUNE_LEAN = 38 };                 /* bit mask (default 31: all set) of the instruction-lean loop forms, each bit-identical to
                                                the plain form it replaces (0 = the plain forms, the tests' reference): bit 0 = filter-row weight gradient,
                                                bit 1 = packed-rows conv kernel, bit 2 = per-tap weight gradient, bit 3 = per-tap conv kernel, bit 4 (with bit 0, round 5) =
                                                the filter-row loop skips the 16-row sub-steps of a K-step that hold no dy pixel (exact zeros) */
/* (Knob numbers are stable across rounds; the gaps are A/B switches of variants that were measured slower and removed with their
 *  kernels -- DESIGN.md 4.1 / 4.2: register-staged bf16 kernels, 4-wave tiles, scattered epilogue stores, the 32x32x16 shared-halo
 *  form, XCD-aware tile orders, the weight-ring and four-fat-wave shared-halo tiles, one / four wave groups and per-tap reads in the
 *  filter-row weight gradient, the scalar Enet reductions, the channel-owner BatchNorm, the vector BatchNorm-backward apply, the Enet finalizes riding in their
 *  producers' last blocks (34), the one-block-per-CU ping-pong conv tile (35, 37) -- and planner constants whose
 *  sweeps are on file: profiles/r03_knob_sweeps.txt.) */
int dct_tune_set(int knob, int value);
int dct_prof_read(double* ms_per_class, int64_t* launches_per_class, int reset);
/* Shader-clock probe: ONE wave on `stream` that sleeps until ref_ticks ticks of the constant 100 MHz reference counter have passed
 * and leaves out2[0] = shader-clock cycles (s_memtime), out2[1] = reference ticks (s_memrealtime) of its life: the clock the chip
 * held meanwhile is 0.1 GHz * out2[0] / out2[1].  Launched on a stream of its own beside the captured step, it samples the clock
 * UNDER that load (bench.py `roofline.shader_clock_ghz_during_the_step`).  out2: two device uint64.  ref_ticks <= 1e8 (one second). */
int dct_clock_probe(unsigned long long* out2, unsigned long long ref_ticks, dct_stream stream);
/* Phase stamp: a one-thread launch on `stream` that appends the 100 MHz reference counter (s_memrealtime) to a ring: slot[0] counts the site's
 * stamps, slot[1 + n % ring] holds the n-th (device uint64[1 + ring], zeroed by the caller).  Diagnostic: queued between the phases of a step, it
 * dates them in the real, pipelined schedule of the replayed graph (CoTrainer.phase_stamps, tools/phase_stamps.py). */
int dct_stamp(unsigned long long* slot, unsigned ring, dct_stream stream);

/* "De-normalise on load": a data-gradient convolution whose input is the BatchNorm-backward result of the layer in front of it
 * computes that result where it would load it -- raw = that layer's fp32 output, tf = its scale / shift / slope (mode != 0),
 * bin = {gradient wrt its activation g, optional ReLU mask of g, saved mean / invstd, c1c2 from dct_enet_bn_bwd_sums} -- so the
 * elementwise apply launch is no longer on the chain between the sums and this convolution (arch/enet.py: it is only launched,
 * as a leaf, where a weight gradient needs the tensor).  Same arithmetic as the apply kernel (one shared definition), rounded to
 * the compute type as the stored tensor would be.  Optional residual gate / accumulate as dct_enet_conv; optional output-side
 * BatchNorm-backward sums as dct_enet_conv_bnbwd_stats (bn_raw != NULL).  MFMA form only (bf16 / f16, >= 16 channels, 16-byte
 * aligned views): DCT_ERR_UNSUPPORTED otherwise -- the caller then materialises the tensor (dct_enet_bn_bwd_apply) and calls
 * dct_enet_conv. */
typedef struct dct_enet_bwd_in {
  const dct_view* g; const dct_view* g_mask;
  const float* mean; const float* invstd; const float* c1c2;
} dct_enet_bwd_in;
int dct_enet_conv_bwd_in(const dct_view* raw, const float* w, const dct_enet_tf* tf, const dct_enet_bwd_in* bin,
                         const dct_view* y, const dct_conv_desc* d, int transposed, int ws_out, int ws_tap, int ws_in,
                         const dct_view* resid_grad, const dct_view* resid_mask, int f32_mask, int dtype,
                         const dct_view* bn_raw, const float* bn_scale, const float* bn_shift, const float* bn_slope, int bn_act,
                         const float* bn_mean, const float* bn_invstd,
                         double* stats_partial, int stats_capacity_rows, int* stats_rows, dct_stream stream);
/* The two halves of dct_enet_bn_bwd[_rows] on their own: the sums (reduction, or the rows a convolution's epilogue wrote, + finalize:
 * parameter gradients and c1c2) and the elementwise apply (draw from raw, g, c1c2).  leaf != 0: the apply's result is only read by
 * weight gradients, so under dct_leaves_begin it is held back with them. */
int dct_enet_bn_bwd_sums(const dct_view* raw, const dct_view* g, const dct_view* g_mask,
                         const float* scale, const float* shift, const float* slope, int act,
                         const float* mean, const float* invstd,
                         float* dgamma, float* dbeta, float* dslope, float* c1c2, int training,
                         int f32_mask, int dtype, void* workspace, size_t workspace_bytes, int partial_rows, dct_stream stream);
int dct_enet_bn_bwd_apply(const dct_view* raw, const dct_view* g, const dct_view* g_mask,
                          const float* scale, const float* shift, const float* slope, int act,
                          const float* mean, const float* invstd, const float* c1c2,
                          const dct_view* draw, int f32_mask, int dtype, int leaf, dct_stream stream);

/* ---- grouped passes -------------------------------------------------------------------------------------------
 * Independent passes with identical shapes (the 2S forward, then the 2S backward passes of a co-training step:
 * cotraining_totalloss.py:208-227,247) as ONE chain of launches: between dct_group_begin(members) and dct_group_end the
 * dct_enet_* entry points record their launches for the member selected by dct_group_member(m) instead of issuing them
 * (every other entry point still launches at once: do not call them inside a group); dct_group_end(stream, ...) issues
 * entry k of all members as one launch (blockIdx.z = member) where kernel, grid, block and LDS bytes agree, else member by
 * member.  Same kernel bodies on the same operands: bit-identical to the passes launched one after the other.  The
 * operands of every recorded launch must stay allocated until dct_group_end returns.  members <= dct_group_max(). */
int dct_group_begin(int members);
int dct_group_member(int member);
int dct_group_max(void);
int dct_group_abort(void);
int dct_group_end(dct_stream stream, int* grouped_launches, int* single_launches);
/* Leaves of a backward pass on another queue: from dct_leaves_begin on, the launches of dct_enet_wgrad and dct_enet_channel_sum
 * (weight / bias gradients: nothing later in the pass reads them) are held back while all other entry points launch as usual;
 * dct_leaves_flush(stream, &n) issues what is held so far on `stream` and keeps recording; dct_leaves_end issues the rest.
 * The caller orders `stream` after the producing chain (an event before the flush) and joins it before the gradients are read;
 * operands stay allocated until then.  Not nestable with a group. */
int dct_leaves_begin(void);
int dct_leaves_flush(dct_stream stream, int* launches);
int dct_leaves_end(dct_stream stream, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* DCT_H_ */
