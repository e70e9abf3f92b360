"""The Enet convolution kernels of csrc/enet.hip at training scale, against float64 references: the MFMA convolution (``MconvK<T, NT>``,
NT = 1 / 2 / 4, direct and gather forms, the fused BatchNorm-backward-on-load and statistics-rows forms), the VALU convolution (``ConvK``),
the MFMA weight gradient and its fold (``MwgradK``, ``WgradRedK``), the VALU weight gradient (``WgradK<T, SL>``) and the bottleneck tails
(``TailFwdK``, ``TailBwdK``) -- ``K.enet_conv*``, ``K.enet_wgrad``, ``K.enet_channel_sum``, ``K.enet_tail_*``.

References are computed in float64 on the device, as one shifted-view GEMM per filter tap on NHWC tensors (`conv_ref`, its transposed /
gather form `convT_ref`, `wgrad_ref` for both pairings of the weight gradient, `pool_first_ref` for the 2x2 pooling with the FIRST maximum
in scan order); `test_reference_helpers_match_torch` checks them against torch.nn.functional on the CPU.

Exact-integer data (the main tool).  Activations, gradients and weights are small integers; producer transforms have integer scale and
shift and slopes from {0.25, 0.5}, so every transformed operand is a multiple of 0.25 that bf16 and f16 hold exactly; biases, residual
gradients and pre-filled accumulators are integers.  The ranges keep 4 x (sum of |terms|) of every output below 2^24 (`assert_exact_range`,
per case; a weight gradient called twice counts both calls and the pre-fill), so every partial sum -- in any order, K-split, pixel slice or
fold -- is a multiple of 0.25 below 2^22 and fp32 accumulation is exact.  The data have non-zero means, so the partial sums are mostly far
above 2^11.  The kernel then equals the float64 reference BIT FOR BIT: exactly for fp32 outputs, after one round-to-nearest-even for bf16 /
f16 outputs.  Outputs are pre-filled with NaN, or with known integers where the kernel adds; inputs that are channel slices of wider
buffers have NaN around them, and the bytes of an output view's buffer outside the view must keep their bits.

Gaussian data (`test_gaussian_*`, one per family).  With U = 2^-24 and |x| (*) |w| the float64 reference on absolute values, a chain of n
fp32 additions is off by at most  n U (|x| (*) |w|)  (first order).  n is what the planned kernel runs: MFMA convolution -- K / 16 steps
split over 4 waves, + the 4-way fold, + 3 (bias, residual, accumulate); VALU forms -- one addition per product (+ 3); weight gradients --
the pixels of one slice / block + the fold over the slices (+ 2; WgradK: + its SL in-block slices), against an |x| (*) |w| that
counts both "+=" calls and the pre-fill.  A bf16 store adds 2^-8 |ref|.  The reference applies the producer
transform as the kernel does: z = fl32(scale x + shift) from the float64 product and sum, rounded once; the negative side fl32(z slope);
then the rounding to the compute dtype where the MFMA forms round their operands.  Largest err / bound per family, as printed on an MI355X
(the two convolution figures come from bf16 stores, whose half ulp reaches 2^-8 |ref| just above a power of two; the largest with an
fp32 store are 0.27 and 0.26):

    family    err / bound   worst case
    MconvK    0.996         16 -> 64 2x2 stride-2 data gradient, NT = 2, bf16 store, n = 8
    ConvK     0.971         24 -> 40 3x3, bf16 store, n = 219
    MwgradK   0.0196        ConvTranspose2d pairing 16 x 144, 113 slices, n = 179
    WgradK    0.0142        16 x 64, SL = 4, 2 blocks, n = 72

Planner mirrors (`mconv_plan`, `convk_plan`, `mwgrad_plan`, `wgradk_plan`) predict the note that enet_conv_impl / dct_enet_wgrad leave in
dct_debug_last_plan, and every edge case asserts the note it was built for: NT thresholds at 1,024 / 2,048 pixel tiles, the weight-gradient
fold's eight-slab round from 113 slices on, the 1,024-slice / 1,024-block caps.  Knobs are set through `knobs`, which restores the shipped
values (ENET_MFMA 3, ENET_MWGRAD_WAVES 2048, ENET_WGRAD_BLOCKS 1024) also when a case fails.

Every Enet conv-family call of one eager training forward and backward of get_arch("enet") is recorded (views, strides, keywords) at
cfg5's geometry (320^2, C = 2, B = 20, bf16) and in the fp32 parity mode (200^2, B = 2), de-duplicated by signature and replayed on fresh
exact-integer data of the same geometry (`test_recorded_calls`), each replay under the plan note the mirrors predict for it.  On an MI355X
the recording holds 299 calls at cfg5 (32 distinct enet_conv, 11 enet_conv_stats, 8 enet_conv_bnbwd_stats, 27 enet_wgrad, 1
enet_channel_sum, 9 + 4 tails) and 301 in the fp32 mode (52, 27, 1, 9 + 5).  No eager pass issues enet_conv_bwd_in, and the fp32 mode
none of the statistics-rows forms (`ISSUED`; a recording that differs fails); `test_fused_bwd_in_at_nt` holds enet_conv_bwd_in to the
separate path at NT = 2 and 4."""
import math

import pytest
import torch
import torch.nn.functional as F

# shared with the UNet file: the helpers that are the same for both (the references below differ: they also take outputs past the
# input's padded extent, which the transposed forms need)
from test_conv_kernels_scale_gpu import cdiv, desc_of, gen, ints, plan_note, same_bits

gpu = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
UB = 2.0 ** -8
EXACT = 2.0 ** 24
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# dct_tune_set knobs (include/dct.h) and their shipped values
ENET_WGRAD_BLOCKS, ENET_MFMA, ENET_MWGRAD_WAVES = 12, 26, 28
DEFAULTS = {ENET_WGRAD_BLOCKS: 1024, ENET_MFMA: 3, ENET_MWGRAD_WAVES: 2048}


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


class knobs(object):
    """Planner knobs for one case, restored to the shipped values afterwards (also when the case fails)."""

    def __init__(self, **kv):
        self.kv = {globals()[k]: v for k, v in kv.items()}

    def __enter__(self):
        from dct_amd import _lib
        self.lib = _lib.load()
        for k, v in self.kv.items():
            assert self.lib.dct_tune_set(k, v) == 0, (k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            self.lib.dct_tune_set(k, DEFAULTS[k])
        return False


# ================================================================================================ references (float64, any device)
def conv_ref(x, w, R, S, stride=1, dil=1, pad_h=0, pad_w=0, Ho=None, Wo=None):
    """x [n, H, W, Cin], w [N, R, S, Cin] -> [n, Ho, Wo, N] = sum over taps of x[shifted] @ w[:, r, s].T, in x's dtype."""
    n, H, W, _ = x.shape
    if Ho is None:
        Ho = (H + 2 * pad_h - dil * (R - 1) - 1) // stride + 1
        Wo = (W + 2 * pad_w - dil * (S - 1) - 1) // stride + 1
    eh = max(0, dil * (R - 1) + (Ho - 1) * stride + 1 - (H + 2 * pad_h))       # (an output past the input's padded extent reads zeros)
    ew = max(0, dil * (S - 1) + (Wo - 1) * stride + 1 - (W + 2 * pad_w))
    xp = F.pad(x, (0, 0, pad_w, pad_w + ew, pad_h, pad_h + eh))
    out = torch.zeros(n, Ho, Wo, w.shape[0], dtype=x.dtype, device=x.device)
    for r in range(R):
        for s in range(S):
            v = xp[:, r * dil: r * dil + (Ho - 1) * stride + 1: stride, s * dil: s * dil + (Wo - 1) * stride + 1: stride, :]
            out += v @ w[:, r, s, :].T
    return out


def convT_ref(x, w, R, S, stride, dil, pad_h, pad_w, Ho, Wo):
    """The transposed (gather) form: y[n, oy, ox, o] = sum over taps (r, s) and inputs i of x[n, iy, ix, i] w[o, r, s, i] where
    iy stride = oy + pad_h - r dil (and so for x) -- the transpose of a strided convolution: a data gradient, or a ConvTranspose2d
    forward.  x [n, H, W, Cin], w [N, R, S, Cin] -> [n, Ho, Wo, N]; computed as the scatter of every input pixel."""
    n, H, W, _ = x.shape
    Hb = max((H - 1) * stride + dil * (R - 1) + 1, pad_h + Ho)
    Wb = max((W - 1) * stride + dil * (S - 1) + 1, pad_w + Wo)
    big = torch.zeros(n, Hb, Wb, w.shape[0], dtype=x.dtype, device=x.device)
    for r in range(R):
        for s in range(S):
            big[:, r * dil: r * dil + (H - 1) * stride + 1: stride, s * dil: s * dil + (W - 1) * stride + 1: stride, :] += x @ w[:, r, s, :].T
    return big[:, pad_h: pad_h + Ho, pad_w: pad_w + Wo, :].contiguous()


def wgrad_ref(a, b, R, S, stride=1, dil=1, pad_h=0, pad_w=0):
    """dw[ac, r, s, bc] = sum over the pixels m of ``a`` of a[m, ac] b[m stride - pad + (r, s) dil, bc], zeros outside ``b``.
    Convolution: a = dy (at the output), b = the layer input -> [Cout][R][S][Cin].  Transposed convolution: a = the layer INPUT,
    b = dy (at the up-sampled output) -> [Cin][R][S][Cout]."""
    n, Ha, Wa, Ca = a.shape
    _, Hb, Wb, Cb = b.shape
    eh = max(0, dil * (R - 1) + (Ha - 1) * stride + 1 - (Hb + 2 * pad_h))
    ew = max(0, dil * (S - 1) + (Wa - 1) * stride + 1 - (Wb + 2 * pad_w))
    bp = F.pad(b, (0, 0, pad_w, pad_w + ew, pad_h, pad_h + eh))
    af = a.reshape(-1, Ca)
    dw = torch.empty(Ca, R, S, Cb, dtype=a.dtype, device=a.device)
    for r in range(R):
        for s in range(S):
            v = bp[:, r * dil: r * dil + (Ha - 1) * stride + 1: stride, s * dil: s * dil + (Wa - 1) * stride + 1: stride, :]
            dw[:, r, s, :] = af.T @ v.reshape(-1, Cb)
    return dw


def pool_first_ref(x):
    """2x2 stride-2 max pooling of x [n, 2h, 2w, C] -> (max, code): code = the window position 2 dy + dx of the FIRST maximum in scan
    order (a later value replaces the best only when strictly greater) -- csrc/enet.hip pool4, ATen's max_pool2d."""
    n, H, W, C = x.shape
    best = torch.full((n, H // 2, W // 2, C), float("-inf"), dtype=x.dtype, device=x.device)
    code = torch.zeros((n, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
    for k in range(4):
        v = x[:, (k >> 1): 2 * (H // 2): 2, (k & 1): 2 * (W // 2): 2, :]
        gt = v > best
        best = torch.where(gt, v, best)
        code = torch.where(gt, torch.full_like(code, k), code)
    return best, code


def tf_ref(x, tfv, mode, round_to=None):
    """The producer transform as the kernels apply it on load, from the stored values x: z = fl32(scale x + shift) (one rounding: fmaf),
    the negative side fl32(z slope) (PReLU) or 0 (ReLU), then the rounding to the MFMA forms' operand type.  -> float64."""
    if mode:
        scale, shift, slope = tfv
        z = (scale.double() * x.double() + shift.double()).float()
        if mode == 2:
            z = torch.where(z > 0, z, (z.double() * slope.double()).float())
        elif mode == 3:
            z = torch.where(z > 0, z, torch.zeros_like(z))
    else:
        z = x
    if round_to is not None:
        z = z.float().to(round_to)
    return z.double()


def test_reference_helpers_match_torch():
    """The tap-GEMM references against torch.nn.functional in float64 on the CPU: conv2d and its two gradients by autograd (`convT_ref` is
    the data gradient), conv_transpose2d forward (`convT_ref`), its data gradient (`conv_ref`) and weight gradient (`wgrad_ref` with the
    layer input first); the pooling codes against max_pool2d's indices on tie-free data and by hand on ties; the planner mirrors on the
    counts the module's cases are built on."""
    g = torch.Generator().manual_seed(0)
    for (n, H, W, Ci, Co, R, S, st, dil, ph, pw) in [(2, 9, 11, 5, 7, 3, 3, 1, 1, 0, 0), (1, 10, 8, 3, 4, 3, 3, 1, 1, 1, 1),
                                                     (2, 12, 10, 4, 6, 2, 2, 2, 1, 0, 0), (1, 13, 13, 3, 2, 3, 3, 1, 4, 4, 4),
                                                     (1, 7, 9, 2, 3, 1, 1, 1, 1, 0, 0), (2, 11, 9, 3, 5, 3, 3, 2, 1, 1, 1),
                                                     (2, 12, 7, 3, 5, 5, 1, 1, 1, 2, 0), (2, 11, 13, 3, 4, 2, 2, 2, 1, 0, 0)]:
        x = torch.randn(n, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, R, S, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, w, stride=st, dilation=dil, padding=(ph, pw))
        wk = w.detach().permute(0, 2, 3, 1)                             # [co][r][s][ci]
        got = conv_ref(x.detach().permute(0, 2, 3, 1), wk, R, S, st, dil, ph, pw)
        assert torch.allclose(got.permute(0, 3, 1, 2), y, rtol=1e-12, atol=1e-12)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        dyk = dy.permute(0, 2, 3, 1)
        dw = wgrad_ref(dyk, x.detach().permute(0, 2, 3, 1), R, S, st, dil, ph, pw)
        assert torch.allclose(dw.permute(0, 3, 1, 2), w.grad, rtol=1e-12, atol=1e-12)
        dx = convT_ref(dyk, wk.permute(3, 1, 2, 0), R, S, st, dil, ph, pw, H, W)      # W(o = ci, tap, i = co)
        assert torch.allclose(dx.permute(0, 3, 1, 2), x.grad, rtol=1e-12, atol=1e-12)
    for (n, H, W, Ci, Co, k, pad, opad) in [(2, 9, 7, 5, 4, 3, 1, 1), (1, 6, 8, 3, 3, 3, 1, 0), (2, 5, 6, 4, 2, 2, 0, 0)]:
        x = torch.randn(n, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Ci, Co, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(x, w, stride=2, padding=pad, output_padding=opad)
        Ho, Wo = y.shape[2], y.shape[3]
        wk = w.detach().permute(0, 2, 3, 1)                             # [ci][r][s][co]
        xk = x.detach().permute(0, 2, 3, 1)
        got = convT_ref(xk, wk.permute(3, 1, 2, 0), k, k, 2, 1, pad, pad, Ho, Wo)
        assert torch.allclose(got.permute(0, 3, 1, 2), y, rtol=1e-12, atol=1e-12)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(dy)
        dyk = dy.permute(0, 2, 3, 1)
        dx = conv_ref(dyk, wk, k, k, 2, 1, pad, pad, H, W)              # data gradient: a strided direct convolution of dy
        assert torch.allclose(dx.permute(0, 3, 1, 2), x.grad, rtol=1e-12, atol=1e-12)
        dw = wgrad_ref(xk, dyk, k, k, 2, 1, pad, pad)                   # [ci][r][s][co]: the layer input comes first
        assert torch.allclose(dw.permute(0, 3, 1, 2), w.grad, rtol=1e-12, atol=1e-12)
    x = torch.randn(2, 5, 10, 14, generator=g, dtype=torch.float64)
    m, idx = F.max_pool2d(x, 2, stride=2, return_indices=True)
    pm, pc = pool_first_ref(x.permute(0, 2, 3, 1))
    oy = torch.arange(5).view(1, 1, 5, 1)
    ox = torch.arange(7).view(1, 1, 1, 7)
    code = (idx // 14 - 2 * oy) * 2 + (idx % 14 - 2 * ox)
    assert torch.equal(pm.permute(0, 3, 1, 2), m) and torch.equal(pc.permute(0, 3, 1, 2).long(), code)
    ties = torch.tensor([[1., 1.], [1., 1.]]).view(1, 2, 2, 1)
    assert pool_first_ref(ties)[1].item() == 0
    assert pool_first_ref(torch.tensor([[0., 2.], [2., 1.]]).view(1, 2, 2, 1))[1].item() == 1
    assert pool_first_ref(torch.tensor([[0., 1.], [2., 2.]]).view(1, 2, 2, 1))[1].item() == 2
    xi = torch.randint(-2, 3, (2, 6, 8, 3), generator=g).double()
    m2, idx2 = F.max_pool2d(xi.permute(0, 3, 1, 2), 2, stride=2, return_indices=True)
    pm2, pc2 = pool_first_ref(xi)
    code2 = (idx2 // 8 - 2 * torch.arange(3).view(1, 1, 3, 1)) * 2 + (idx2 % 8 - 2 * torch.arange(4).view(1, 1, 1, 4))
    assert torch.equal(pm2.permute(0, 3, 1, 2), m2) and torch.equal(pc2.permute(0, 3, 1, 2).long(), code2)
    # the transform: exact on quarter multiples, the negative side, the operand rounding
    tfv = (torch.tensor([2.0]), torch.tensor([-1.0]), torch.tensor([0.25]))
    xs = torch.tensor([-3.0, 0.0, 0.5, 3.0]).view(1, 1, 4, 1)
    assert tf_ref(xs, tfv, 2).flatten().tolist() == [-1.75, -0.25, 0.0, 5.0]
    assert tf_ref(xs, tfv, 3).flatten().tolist() == [0.0, 0.0, 0.0, 5.0]
    assert tf_ref(xs, tfv, 1).flatten().tolist() == [-7.0, -1.0, 0.0, 5.0]
    assert tf_ref(torch.tensor([1.0 + 2.0 ** -9]), None, 0, BF16).item() == 1.0
    # the planner mirrors on the counts the cases name
    assert mconv_plan(128, 1 * 181 * 180)[:3] == (1019, 1, 4) and mconv_plan(128, 1 * 181 * 181)[:3] == (1024, 2, 2)
    assert mconv_plan(128, 3 * 149 * 146)[:3] == (2040, 2, 2) and mconv_plan(128, 3 * 149 * 147)[:3] == (2054, 4, 1)
    assert mconv_plan(64, 3 * 149 * 146)[:3] == (2040, 1, 2) and mconv_plan(64, 3 * 149 * 147)[:3] == (2054, 2, 1)
    assert mconv_plan(96, 181 * 181)[:3] == (1024, 2, 2) and mconv_plan(40, 3 * 149 * 147)[:3] == (2054, 2, 1)
    assert mconv_plan(64, 20 * 80 * 80)[:3] == (4000, 2, 1) and mconv_plan(32, 3 * 149 * 147)[:3] == (2054, 1, 1)
    assert mwgrad_plan(13, 9, 246) == (1, 1, 64, 4) and mwgrad_plan(16, 16, 3 * 149 * 147) == (1, 1, 128, 514)
    assert mwgrad_plan(13, 9, 65526) == (1, 1, 64, 1024) and mwgrad_plan(13, 9, 20 * 160 * 160) == (1, 1, 512, 1000)
    assert mwgrad_plan(128, 288, 65526, waves=36864) == (4, 9, 64, 1024) and mwgrad_plan(128, 288, 65526) == (4, 9, 1216, 54)
    assert wgradk_plan(16, 64, 100) == (4, 64, 2) and wgradk_plan(16, 144, 7182) == (2, 64, 113)
    assert wgradk_plan(32, 288, 15309) == (1, 64, 240) and wgradk_plan(13, 9, 65541) == (4, 96, 683)
    assert convk_plan(1, 13, 9, 2 * 100 * 100) == (2, 157, 576) and convk_plan(64, 64, 9, 100)[2] > 64 * 1024
    # the case tables reach what they name
    for c in MCONV_CASES:
        ys = conv_geom(*c[:5])[1]
        assert mconv_plan(c[2], ys[0] * ys[1] * ys[2])[1] == c[-1], c
    for c in MWGRAD_CASES:
        ad, _, kw = wgrad_geom(*c[:5])
        assert mwgrad_plan(c[1], kw["R"] * kw["S"] * c[2], ad[0] * ad[1] * ad[2], c[-2])[3] == c[-1], c
    for c in WGRADK_CASES:
        ad, _, kw = wgrad_geom(*c[:5])
        pl = wgradk_plan(c[1], kw["R"] * kw["S"] * c[2], ad[0] * ad[1] * ad[2], c[-2])
        assert (pl[0], pl[2]) == c[-1], c


# ================================================================================================ planner mirrors (csrc/enet.hip)
def takes_mfma(compute, cin, cout, mfma_knob=3):
    """enet_conv_impl's host check for the MFMA form, for 16-byte aligned dense or channel-slice views (p.vec) and residual views stored
    in the compute dtype: low-precision mode and at least 16 input channels in whole groups of 16."""
    return bool(mfma_knob & 1) and compute != F32 and cin >= 16 and cin % 16 == 0 and cout <= 128


def mconv_plan(cout, P):
    """-> (ptiles, NT, ngroups, grid): one block per 32 pixels x 32 NT channels; NT > 1 only where the pixel tiles alone fill the chip."""
    ptiles, ntiles = cdiv(P, 32), cdiv(cout, 32)
    nt = 1
    if ntiles >= 4 and ptiles >= 2048:
        nt = 4
    elif ntiles >= 2 and ptiles * ((ntiles + 1) // 2) >= 2048:
        nt = 2
    ngroups = cdiv(ntiles, nt)
    return ptiles, nt, ngroups, ptiles * ngroups


def mconv_note(cout, P, form, wvec, stats=0):
    _, nt, ngroups, grid = mconv_plan(cout, P)
    return f"enet mconv {form} NT {nt}: {ngroups} groups, grid {grid}, wvec {wvec}, stats rows {stats}"


def convk_plan(cin, cout, taps, P):
    """-> (G, grid, LDS bytes): one thread per pixel x 8 channels, G = channel groups of 8 rounded up to a power of two."""
    G = 1
    while G < cdiv(cout, 8):
        G <<= 1
    return G, cdiv(P, 256 // G), taps * cin * G * 8 * 4


def convk_note(cin, cout, taps, P):
    G, grid, lds = convk_plan(cin, cout, taps, P)
    return f"enet conv valu G {G}: grid {grid}, lds {lds}"


def mwgrad_plan(Ca, kb, P, waves=2048):
    """-> (mtiles, ntiles, pixels per slice, slices): ~waves waves, >= 4 MFMA steps (64 pixels) per slice, <= 1024 slices."""
    mtiles, ntiles = cdiv(Ca, 32), cdiv(kb, 32)
    steps = cdiv(P, 16)
    ks = max(waves // (mtiles * ntiles), 1)
    sps = max(cdiv(steps, ks), 4)
    if cdiv(steps, sps) > 1024:
        sps = cdiv(steps, 1024)
    sps = cdiv(sps, 4) * 4
    return mtiles, ntiles, 16 * sps, cdiv(P, 16 * sps)


def mwgrad_note(Ca, kb, P, waves=2048):
    return "enet mwgrad %d x %d tiles: pps %d, %d slices" % mwgrad_plan(Ca, kb, P, waves)


def wgradk_plan(Ca, kb, P, max_blocks=1024):
    """-> (SL, pixels per block, blocks); None where the gradient has more than 512 register tiles of 4 x 8."""
    tiles = cdiv(Ca, 4) * cdiv(kb, 8)
    if tiles > 512:
        return None
    SL = 4 if tiles <= 64 else 2 if tiles <= 128 else 1
    blocks = max(min(cdiv(P, 64), max_blocks), 1)
    ppb = cdiv(cdiv(P, blocks), 32) * 32
    return SL, ppb, cdiv(P, ppb)


def wgradk_note(Ca, kb, P, max_blocks=1024):
    return "enet wgrad valu SL %d: ppb %d, %d blocks" % wgradk_plan(Ca, kb, P, max_blocks)


# ================================================================================================ data and checks
def assert_exact_range(abs_ref, what):
    """4 x (sum of |terms|) < 2^24: every partial sum of quarter multiples is then exact in fp32."""
    m = 4.0 * float(abs_ref.max()) if abs_ref.numel() else 0.0
    assert m < EXACT, f"{what}: 4 x sum |terms| reaches {m:.3g}: the exact-integer premise does not hold"


def nan_fill(span, dtype):
    if dtype.is_floating_point:
        return torch.full((span,), float("nan"), dtype=dtype, device=DEV)
    return torch.full((span,), 0xA5, dtype=dtype, device=DEV)


def dense(shape, dtype):
    st, s = [], 1
    for d in reversed(shape):
        st.append(s)
        s *= d
    return (tuple(shape), tuple(reversed(st)), 0, dtype)


def wide(shape, dtype, lo, hi):
    """A channel slice [lo, lo + C) of a buffer lo + C + hi channels wide."""
    n, h, w, c = shape
    Wd = lo + c + hi
    return ((n, h, w, c), (h * w * Wd, w * Wd, Wd, 1), lo, dtype)


class Buf(object):
    """A tensor view (shape, strides, offset modulo 64 elements, dtype) on a fresh NaN-filled buffer of its own.  `set` gives the view
    its data; `check_out` holds the view to the expected bits and the rest of the buffer to what it was."""

    def __init__(self, desc, data=None):
        shape, stride, off, dtype = desc
        off %= 64
        span = off + 1 + sum((a - 1) * b for a, b in zip(shape, stride)) if all(shape) else off
        self.base = nan_fill(span, dtype)
        self.t = self.base.as_strided(shape, stride, off)
        self.desc = (tuple(shape), tuple(stride), off, dtype)
        if data is not None:
            self.t.copy_(data)
        self.before = self.base.clone()

    def old(self):
        return self.before.as_strided(*self.desc[:3])

    def check_out(self, want, what):
        exp = self.before.clone()
        exp.as_strided(*self.desc[:3]).copy_(want)
        same_bits(self.base, exp, what)

    def check_untouched(self, what):
        same_bits(self.base, self.before, what)


class Data(object):
    """Value ranges of one case: exact integers (mode "int") or Gaussian (mode "gauss").  ``small`` narrows the integer ranges for the
    cases whose sums run over several hundred thousand pixels."""

    def __init__(self, mode, seed, small=False):
        self.mode, self.g, self.small = mode, gen(seed), small
        self.exact = mode == "int"

    def act(self, shape, dtype):          # stored activations / images: non-negative integers (mean 1.5) / |N(0, 1)|
        if self.exact:
            return ints(self.g, shape, 0, 2 if self.small else 3, dtype)
        return torch.randn(tuple(shape), generator=self.g, device=DEV).abs().to(dtype)

    def raw(self, shape, dtype):          # raw convolution outputs ahead of a transform: both signs, mean 0.5 / N(1, 2)
        if self.exact:
            return ints(self.g, shape, -1 if self.small else -2, 2 if self.small else 3, dtype)
        return (torch.randn(tuple(shape), generator=self.g, device=DEV) * 2 + 1).to(dtype)

    def grad(self, shape, dtype):         # gradients and weights: integers in [-1, 2] (mean 0.5) / N(0, 1)
        if self.exact:
            return ints(self.g, shape, -1, 1 if self.small else 2, dtype)
        return torch.randn(tuple(shape), generator=self.g, device=DEV).to(dtype)

    def seed_out(self, shape, dtype):     # what an accumulating kernel adds to
        if self.exact:
            return ints(self.g, shape, -8, 8, dtype)
        return torch.randn(tuple(shape), generator=self.g, device=DEV).to(dtype)

    def tf(self, K, C, mode):
        """-> (K.Tf | None, (scale, shift, slope) | None): integer scale and shift, slopes from {0.25, 0.5} / as a BatchNorm gives them."""
        if not mode:
            return None, None
        if self.exact:
            scale = ints(self.g, (C,), 1, 1 if self.small else 2, F32)
            shift = ints(self.g, (C,), -1 if self.small else -2, 1 if self.small else 2, F32)
            slope = ints(self.g, (C,), 1, 2, F32) * 0.25
        else:
            scale = torch.rand(C, generator=self.g, device=DEV) + 0.5
            shift = torch.randn(C, generator=self.g, device=DEV) * 0.3
            slope = torch.rand(C, generator=self.g, device=DEV) * 0.5
        return K.Tf(scale, shift, slope if mode == 2 else None, mode), (scale, shift, slope)


class Stats(object):
    worst = {}

    @classmethod
    def note(cls, family, ratio):
        cls.worst[family] = max(cls.worst.get(family, 0.0), ratio)


def compare(buf, ref, absref, n_chain, what, family, exact):
    """Exact: the view equals ref rounded once to its dtype.  Gaussian: |got - ref| <= n U absref (+ half a bf16 ulp of ref)."""
    dtype = buf.desc[3]
    if exact:
        buf.check_out(ref.to(F32).to(dtype), what)
        return
    got = buf.t.double()
    assert dtype in (F32, BF16), dtype
    bound = n_chain * U * absref + (UB * ref.abs() if dtype == BF16 else 0) + 2.0 ** -126
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    print(f"  {what}: err / bound {ratio:.3g} (n = {n_chain})")
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3g} (max err {float(err.max()):.3g})"
    Stats.note(family, ratio)
    exp = buf.before.clone()
    exp.as_strided(*buf.desc[:3]).copy_(buf.t)
    same_bits(buf.base, exp, f"{what}: bytes outside the view")


# ================================================================================================ one convolution call
ROWS_CHECKED = {"sum": 0, "squares": 0}      # how many statistics-rows comparisons ran (the squares' depends on the range)


def conv_call(K, D, xd, yd, kw, tfmode=0, has_bias=False, rgd=None, rmd=None, compute=BF16, what="", stats=False, expect=None):
    """One K.enet_conv on fresh data of the given views, against float64.  ``stats`` = "fwd": K.enet_conv_stats, whose rows are
    checked too; ``stats`` = ("bnbwd", raw view, transform mode, mean view, invstd view): K.enet_conv_bnbwd_stats (y against float64
    and the row count; the rows' values belong to the BatchNorm file).  ``kw``: R, S, stride, dil, pad_h, pad_w, transposed, ws,
    accumulate.  ``expect``: the plan note the call must leave.  -> the plan note."""
    kw = dict(kw)
    (n, H, W, cin), xdt = xd[0], xd[3]
    (_, Ho, Wo, cout), ydt = yd[0], yd[3]
    R, S, stride, dil = kw["R"], kw["S"], kw.get("stride", 1), kw.get("dil", 1)
    ph, pw, gather, acc = kw.get("pad_h", 0), kw.get("pad_w", 0), kw.get("transposed", False), kw.get("accumulate", False)
    taps, ws = R * S, kw["ws"]
    wn = 1 + (cout - 1) * ws[0] + (taps - 1) * ws[1] + (cin - 1) * ws[2]
    assert wn == cout * taps * cin, (ws, cout, taps, cin)
    wbuf = D.grad((wn,), F32) if D.exact else D.grad((wn,), F32) / math.sqrt(taps * cin)
    Wd = wbuf.as_strided((cout, R, S, cin), (ws[0], S * ws[1], ws[1], ws[2]))
    tf, tfv = D.tf(K, cin, tfmode)
    x = Buf(xd, D.raw((n, H, W, cin), xdt) if tfmode else (D.grad if gather else D.act)((n, H, W, cin), xdt))
    bias = (ints(D.g, (cout,), -64, 64, F32) if D.exact else torch.randn(cout, generator=D.g, device=DEV)) if has_bias else None
    y = Buf(yd, D.seed_out((n, Ho, Wo, cout), ydt) if acc else None)
    rg = rm = None
    if rgd is not None:
        rg = Buf(rgd, D.seed_out(rgd[0], rgd[3]))
        rm = Buf(rmd, D.raw(rmd[0], rmd[3]))
    bn = stats if isinstance(stats, tuple) else None
    if stats:
        tiles = cdiv(n * Ho * Wo, 32)
        st = torch.full((tiles * cout * 3,), float("nan"), dtype=torch.float64, device=DEV)
        kws = {k: v for k, v in kw.items() if k != "accumulate"}
        if bn:
            _, rrawd, rmode, meand, invd = bn
            rec_raw = Buf(rrawd, D.raw(rrawd[0], rrawd[3]))
            rec_tf, _ = D.tf(K, cout, rmode)
            mean, invstd = Buf(meand, D.raw(meand[0], meand[3])), Buf(invd, D.act(invd[0], invd[3]) + 1)
            rows = K.enet_conv_bnbwd_stats(x.t, wbuf, y.t, st, rec_raw.t, rec_tf, mean.t, invstd.t, compute=compute, **kws)
        else:
            rows = K.enet_conv_stats(x.t, wbuf, bias, tf, y.t, st, compute=compute, **kws)
    else:
        K.enet_conv(x.t, wbuf, bias, tf, y.t, resid_grad=rg.t if rg else None, resid_mask=rm.t if rm else None, compute=compute, **kw)
    note = plan_note()
    torch.cuda.synchronize()
    what = f"{what} [{note}]"
    if expect is not None:
        assert note == expect, (what, expect)
    mfma = note.startswith("enet mconv")
    low = compute if compute != F32 else (xdt if xdt != F32 else F32)
    assert mfma == takes_mfma(low, cin, cout, D.mfma_knob if hasattr(D, "mfma_knob") else 3), what
    rt = low if mfma else None                                # the MFMA form rounds both operands to the compute dtype
    xv = tf_ref(x.t, tfv, tfmode, rt)
    wv = tf_ref(Wd, None, 0, rt)
    fn = (lambda a, b: convT_ref(a, b, R, S, stride, dil, ph, pw, Ho, Wo)) if gather else \
         (lambda a, b: conv_ref(a, b, R, S, stride, dil, ph, pw, Ho, Wo))
    ref, absr = fn(xv, wv), fn(xv.abs(), wv.abs())
    if bias is not None:
        ref, absr = ref + bias.double(), absr + bias.double().abs()
    if rg is not None:
        gate = rm.t.double() > 0
        ref = ref + torch.where(gate, rg.t.double(), torch.zeros_like(ref))
        absr = absr + rg.t.double().abs()
    if acc:
        ref, absr = ref + y.old().double(), absr + y.old().double().abs()
    if D.exact:
        assert_exact_range(absr, what)
    K16 = taps * cin // 16
    n_chain = (cdiv(K16, 4) + 4 + 3) if mfma else (taps * cin + 3)
    compare(y, ref, absr, n_chain, what + ": y", "MconvK" if mfma else "ConvK", D.exact)
    x.check_untouched(what + ": x")
    if stats:
        tiles = cdiv(n * Ho * Wo, 32)
        if not mfma:
            assert rows == 0, what
        elif bn:
            assert rows == tiles and note.endswith("stats rows 2"), (what, rows, tiles)
            assert bool(torch.isfinite(st).all()), what + ": rows"
            rec_raw.check_untouched(what + ": the producer's raw output")
        else:
            assert rows == tiles and note.endswith("stats rows 1"), (what, rows, tiles)
            if D.exact:
                # the rows carry the fp32 outputs ahead of the storage rounding: per tile of 32 pixels {sum, sum of squares, 0}
                out = ref.reshape(-1, cout)
                pad = tiles * 32 - out.shape[0]
                o3 = F.pad(out, (0, 0, 0, pad)).view(tiles, 32, cout)
                got = st.view(tiles, cout, 3)
                same_bits(got[:, :, 0].contiguous(), o3.sum(1), what + ": rows, sum")
                ROWS_CHECKED["sum"] += 1
                same_bits(got[:, :, 2].contiguous(), torch.zeros_like(got[:, :, 2]), what + ": rows, third sum")
                sq = (o3 * o3).sum(1)
                if 16.0 * float(sq.max()) < EXACT:          # (squares of quarter multiples are multiples of 1/16)
                    same_bits(got[:, :, 1].contiguous(), sq, what + ": rows, sum of squares")
                    ROWS_CHECKED["squares"] += 1
    return note


def _ids(table):
    """Readable case ids: the case tuple with dtypes and shapes spelled short."""
    def one(v):
        if isinstance(v, torch.dtype):
            return {F32: "f32", BF16: "bf16", F16: "f16"}[v]
        if isinstance(v, tuple):
            return "x".join(map(str, v))
        return str(v).replace(",", "+") or "plain"
    return [f"{i}-" + "-".join(one(v) for v in c) for i, c in enumerate(table)]


FILTERS = {            # R, S, stride, dil, pad_h, pad_w
    "1x1": (1, 1, 1, 1, 0, 0), "3x3": (3, 3, 1, 1, 1, 1), "3x3d4": (3, 3, 1, 4, 4, 4), "5x1": (5, 1, 1, 1, 2, 0),
    "3x3s2": (3, 3, 2, 1, 1, 1), "2x2s2": (2, 2, 2, 1, 0, 0),
}


def conv_geom(out_px, cin, cout, filt, form):
    """Input shape, output shape and keywords of a convolution with ``out_px`` = (n, Ho, Wo) output pixels.  Forms: "direct"
    (weights [cout][tap][cin]), "gather" = the data gradient of a direct convolution cout -> cin (weights [fwd cout = cin here][tap][cout
    here], ``ws=(1, cout, taps cout)``: wvec = 0), "convT" = a stride-2 ConvTranspose2d forward (weights [cin][tap][cout], gather)."""
    R, S, stride, dil, ph, pw = FILTERS[filt]
    n, Ho, Wo = out_px
    taps = R * S
    kw = dict(R=R, S=S, stride=stride, dil=dil, pad_h=ph, pad_w=pw)
    if form == "direct":
        H = (Ho - 1) * stride + dil * (R - 1) + 1 - 2 * ph + (stride - 1)
        W = (Wo - 1) * stride + dil * (S - 1) + 1 - 2 * pw + (stride - 1)
        kw.update(ws=(taps * cin, cin, 1))
    else:
        if form == "convT":        # ConvTranspose2d(stride 2): the output is twice the input (+ output_padding on even sizes)
            H, W = cdiv(Ho, 2), cdiv(Wo, 2)
        else:
            H = (Ho + 2 * ph - dil * (R - 1) - 1) // stride + 1
            W = (Wo + 2 * pw - dil * (S - 1) - 1) // stride + 1
        kw.update(transposed=True, ws=(1, cout, taps * cout))
    return (n, H, W, cin), (n, Ho, Wo, cout), kw


# ================================================================================================ 1. MconvK across the NT thresholds
A0, A1 = (1, 181, 180), (1, 181, 181)        # 1,019 / 1,024 pixel tiles (the last one of A1: 25 pixels)
B0, B1 = (3, 149, 146), (3, 149, 147)        # 2,040 / 2,054 pixel tiles (the last one of B1: 13 pixels)

MCONV_CASES = [
    # out pixels, cin, cout, filter, form, x dtype, transform mode, y dtype, compute, options, NT
    (A0, 32, 128, "1x1", "direct", F32, 2, F32, BF16, "bias", 1),             # 4 column tiles below 1,024 pixel tiles: one group each
    (A1, 32, 128, "1x1", "direct", F32, 2, F32, BF16, "bias", 2),             # ... at 1,024: two groups of two
    (A1, 32, 128, "1x1", "direct", F32, 2, F32, F16, "bias", 2),
    (B0, 32, 128, "1x1", "direct", F32, 3, F32, BF16, "bias", 2),             # 2,040 tiles: still NT = 2
    (B1, 32, 128, "1x1", "direct", F32, 3, F32, BF16, "bias,views", 4),       # 2,054 tiles: NT = 4, one group
    (B1, 32, 128, "1x1", "direct", F32, 3, F32, F16, "bias", 4),
    (A0, 32, 96, "3x3", "direct", F32, 1, F32, BF16, "bias", 1),
    (A1, 32, 96, "3x3", "direct", F32, 1, F32, BF16, "bias", 2),              # three column tiles: the second group half empty
    (A1, 32, 96, "3x3", "direct", F32, 1, F32, F16, "bias", 2),
    (A0, 32, 72, "3x3d4", "direct", BF16, 0, BF16, BF16, "", 1),
    (A1, 32, 72, "3x3d4", "direct", BF16, 0, BF16, BF16, "views", 2),         # a partly filled third column tile
    (B0, 16, 64, "1x1", "direct", F32, 2, F32, BF16, "bias", 1),              # two column tiles below 2,048 pixel tiles
    (B1, 16, 64, "1x1", "direct", F32, 2, F32, BF16, "bias", 2),              # cfg5's stage-1 16 -> 64
    (B1, 16, 64, "1x1", "direct", F32, 2, F32, F16, "bias", 2),
    (B0, 16, 40, "5x1", "direct", F32, 3, F32, BF16, "bias", 1),
    (B1, 16, 40, "5x1", "direct", F32, 3, F32, BF16, "bias", 2),              # a partly filled second column tile
    (B1, 128, 32, "3x3", "direct", BF16, 0, F32, BF16, "bias", 1),            # long K: 8 steps per tap, 72 in all
    (B1, 16, 64, "3x3s2", "direct", F32, 2, F32, BF16, "bias", 2),
    (B1, 32, 128, "2x2s2", "direct", BF16, 0, BF16, BF16, "", 4),             # the down-sampling form
    (B1, 32, 128, "3x3s2", "direct", BF16, 0, BF16, BF16, "", 4),             # the data gradient of a stride-2 ConvTranspose2d
    (B1, 64, 64, "3x3s2", "direct", BF16, 0, F32, BF16, "acc", 2),
    # data gradients (gather form, wvec = 0)
    (B0, 16, 64, "1x1", "gather", BF16, 0, BF16, BF16, "resid", 1),
    (B1, 16, 64, "1x1", "gather", BF16, 0, BF16, BF16, "resid,views", 2),     # cfg5's 64-wide data gradient
    (B1, 64, 64, "1x1", "gather", BF16, 0, BF16, BF16, "", 2),                # (the baseline of the fused forms below)
    (B1, 32, 128, "1x1", "gather", BF16, 0, BF16, BF16, "", 4),
    (B1, 32, 128, "3x3", "gather", BF16, 0, F32, BF16, "acc", 4),
    (B1, 32, 128, "3x3", "gather", F16, 0, F16, F16, "resid", 4),
    (A1, 32, 96, "3x3d4", "gather", BF16, 0, BF16, BF16, "acc", 2),
    (B1, 16, 40, "5x1", "gather", BF16, 0, BF16, BF16, "", 2),
    (A1, 32, 72, "3x3s2", "gather", BF16, 0, BF16, BF16, "", 2),
    (B0, 16, 64, "2x2s2", "gather", BF16, 0, BF16, BF16, "", 1),
    (B1, 16, 64, "2x2s2", "gather", BF16, 0, BF16, BF16, "acc,resid", 2),
    (A1, 128, 32, "1x1", "gather", BF16, 0, BF16, BF16, "", 1),
    (B1, 128, 32, "3x3", "gather", F16, 0, F16, F16, "", 1),
    # the stride-2 ConvTranspose2d forward
    (B1, 16, 64, "3x3s2", "convT", F32, 3, F32, BF16, "bias", 2),
    (B1, 32, 128, "3x3s2", "convT", F32, 2, F32, F16, "bias", 4),
]


@gpu
@pytest.mark.parametrize("case", range(len(MCONV_CASES)), ids=_ids(MCONV_CASES))
def test_mconv_nt_edges(K, case):
    """MconvK<T, NT> just below and at the NT thresholds, ragged last pixel tiles, partly filled column tiles and groups: exact-integer
    data, bit for bit against float64, and the plan note says which NT ran."""
    out_px, cin, cout, filt, form, xdt, mode, ydt, compute, opts, nt = MCONV_CASES[case]
    xs, ys, kw = conv_geom(out_px, cin, cout, filt, form)
    P = ys[0] * ys[1] * ys[2]
    assert mconv_plan(cout, P)[1] == nt, (mconv_plan(cout, P), nt)
    views = "views" in opts
    xd = wide(xs, xdt, 8, 8) if views else dense(xs, xdt)
    yd = wide(ys, ydt, 3, 5) if views else dense(ys, ydt)
    rgd = rmd = None
    if "resid" in opts:
        rgd = wide(ys, compute, 2, 6) if views else dense(ys, compute)
        rmd = wide(ys, compute, 5, 1) if views else dense(ys, compute)
    kw["accumulate"] = "acc" in opts
    what = f"mconv {out_px} {cin}->{cout} {filt} {form} {opts}"
    note = conv_call(K, Data("int", 100 + case), xd, yd, kw, mode, "bias" in opts, rgd, rmd, compute, what)
    assert note == mconv_note(cout, P, "direct" if form == "direct" else "gather", 1 if form == "direct" else 0), note


# ================================================================================================ 2. ConvK
S3 = (2, 25, 25)                    # a stage-3 tensor of the fp32 parity mode: 1,250 pixels
CONVK_CASES = [
    # out pixels, cin, cout, filter, form, x dtype, transform mode, y dtype, compute, options, ENET_MFMA knob
    (S3, 14, 3, "1x1", "direct", F32, 3, F32, F32, "bias", 3),                # G = 1: 256 pixels per block, 4.9 blocks
    (S3, 13, 13, "3x3", "direct", F32, 2, F32, F32, "bias", 3),               # G = 2: 128 per block
    (S3, 3, 14, "1x1", "direct", F32, 3, F32, BF16, "bias", 3),               # the last up-sampling bottleneck's widths, bf16 mode
    (S3, 24, 40, "3x3", "direct", BF16, 0, F32, BF16, "bias,views", 3),       # 24 channels: not whole groups of 16 -> VALU; G = 8
    (S3, 40, 24, "5x1", "direct", BF16, 0, BF16, BF16, "", 3),                # G = 4
    (S3, 40, 128, "1x1", "direct", BF16, 0, F32, BF16, "bias", 3),            # G = 16: 16 pixels per block, 78.1 blocks
    (S3, 24, 40, "2x2s2", "direct", BF16, 0, BF16, BF16, "", 3),              # 24 channels, 2 x 2 taps: K = 96 is whole steps, still VALU
    (S3, 14, 16, "2x2s2", "direct", BF16, 0, F32, BF16, "bias", 3),           # the down-sampling 2x2
    (S3, 32, 32, "3x3d4", "direct", F32, 2, F32, BF16, "bias", 0),            # knob 26 = 0: the MFMA shape on the VALU kernel
    (S3, 16, 64, "3x3s2", "direct", F32, 2, F32, F32, "bias", 3),             # fp32 mode: G = 8
    (S3, 40, 24, "3x3", "gather", BF16, 0, BF16, BF16, "resid,acc", 3),       # data gradients
    (S3, 14, 24, "3x3d4", "gather", F32, 0, F32, F32, "resid", 3),
    (S3, 13, 1, "3x3s2", "gather", BF16, 0, F32, BF16, "acc", 3),             # the initial convolution's, onto the image gradient
    (S3, 16, 14, "2x2s2", "gather", F32, 0, F32, F32, "", 3),
    (S3, 24, 13, "5x1", "gather", BF16, 0, BF16, BF16, "views", 3),
    (S3, 3, 3, "3x3s2", "convT", F32, 3, F32, BF16, "bias", 3),               # ConvTranspose2d forward of the last bottleneck
    (S3, 16, 16, "3x3s2", "convT", F32, 2, F32, F32, "bias", 3),
    ((2, 100, 100), 1, 13, "3x3s2", "direct", F32, 0, F32, BF16, "bias", 3),  # the initial 1 -> 13 convolution on 2 x 200 x 200
    ((2, 100, 100), 1, 13, "3x3s2", "direct", F32, 0, F32, F32, "bias", 3),
]


@gpu
@pytest.mark.parametrize("case", range(len(CONVK_CASES)), ids=_ids(CONVK_CASES))
def test_convk_shapes(K, case):
    """ConvK (fp32 mode; bf16 mode with ragged channel counts or with ENET_MFMA bit 0 off) on the filters and widths of the model, with
    a ragged last block for every pixels-per-block count: exact-integer data, bit for bit."""
    out_px, cin, cout, filt, form, xdt, mode, ydt, compute, opts, knob = CONVK_CASES[case]
    xs, ys, kw = conv_geom(out_px, cin, cout, filt, form)
    P = ys[0] * ys[1] * ys[2]
    G, grid, _ = convk_plan(cin, cout, kw["R"] * kw["S"], P)
    assert P % (256 // G), "the last block is not ragged"
    views = "views" in opts
    xd = wide(xs, xdt, 8, 8) if views else dense(xs, xdt)
    yd = wide(ys, ydt, 3, 5) if views else dense(ys, ydt)
    rgd = rmd = None
    if "resid" in opts:
        rdt = compute if compute != F32 else F32
        rgd, rmd = dense(ys, rdt), wide(ys, rdt, 1, 2)
    kw["accumulate"] = "acc" in opts
    D = Data("int", 300 + case)
    D.mfma_knob = knob
    with knobs(ENET_MFMA=knob):
        note = conv_call(K, D, xd, yd, kw, mode, "bias" in opts, rgd, rmd, compute, f"convk {out_px} {cin}->{cout} {filt} {form} {opts}")
    assert note == convk_note(cin, cout, kw["R"] * kw["S"], P), note


@gpu
def test_convk_weights_past_lds_raise(K):
    """An fp32 3 x 3 convolution 64 -> 64 needs 144 KiB of weights in LDS: the call raises and y keeps its bits."""
    xs, ys, kw = conv_geom((1, 9, 7), 64, 64, "3x3", "direct")
    assert convk_plan(64, 64, 9, 63)[2] > 64 * 1024
    D = Data("int", 1)
    x, y = D.act(xs, F32), Buf(dense(ys, F32))
    w = D.grad((64 * 9 * 64,), F32)
    with pytest.raises(RuntimeError):
        K.enet_conv(x, w, None, None, y.t, compute=F32, **kw)
    torch.cuda.synchronize()
    y.check_untouched("y after the refused call")


# ================================================================================================ one weight-gradient call
def wgrad_call(K, D, ad, bd, kw, tfa_mode=0, tfb_mode=0, what="", expect=None, family=None):
    """K.enet_wgrad twice ("+=") into a pre-filled dw, against float64.  a / b as dct_enet_wgrad takes them: a pixel of ``a`` pairs with
    the pixel (stride ay - pad + r dil, ...) of ``b``; dw is [Ca][R][S][Cb].  -> the plan note."""
    (n, Ha, Wa, Ca), adt = ad[0], ad[3]
    (_, Hb, Wb, Cb), bdt = bd[0], bd[3]
    R, S, stride, dil, ph, pw = kw["R"], kw["S"], kw.get("stride", 1), kw.get("dil", 1), kw.get("pad_h", 0), kw.get("pad_w", 0)
    tfa, tfav = D.tf(K, Ca, tfa_mode)
    tfb, tfbv = D.tf(K, Cb, tfb_mode)
    a = Buf(ad, D.raw(ad[0], adt) if tfa_mode else D.grad(ad[0], adt))
    b = Buf(bd, D.raw(bd[0], bdt) if tfb_mode else D.act(bd[0], bdt))
    dw = D.seed_out((Ca * R * S * Cb,), F32)
    dw0 = dw.clone()
    K.enet_wgrad(a.t, tfa, b.t, tfb, dw, **kw)
    note = plan_note()
    K.enet_wgrad(a.t, tfa, b.t, tfb, dw, **kw)
    torch.cuda.synchronize()
    what = f"{what} [{note}]"
    if expect is not None:
        assert note == expect, (what, expect)
    mfma = note.startswith("enet mwgrad")
    low = [t for t in (adt, bdt) if t != F32]
    rt = low[0] if (mfma and low) else None                     # the MFMA form rounds both operands to the compute dtype
    assert mfma == bool(low and (getattr(D, "mfma_knob", 3) & 2)), what
    av, bv = tf_ref(a.t, tfav, tfa_mode, rt), tf_ref(b.t, tfbv, tfb_mode, rt)
    one = wgrad_ref(av, bv, R, S, stride, dil, ph, pw).reshape(-1)
    absr = wgrad_ref(av.abs(), bv.abs(), R, S, stride, dil, ph, pw).reshape(-1)
    ref = dw0.double() + 2 * one
    absr = dw0.double().abs() + 2 * absr
    P = n * Ha * Wa
    if D.exact:
        assert_exact_range(absr, what)
        same_bits(dw, ref.float(), what + ": dw")
    else:
        if mfma:
            _, _, pps, nsl = mwgrad_plan(Ca, R * S * Cb, P, getattr(D, "waves", 2048))
            n_chain = min(pps, P) + nsl + 2
        else:
            SL, ppb, nb = wgradk_plan(Ca, R * S * Cb, P, getattr(D, "max_blocks", 1024))
            n_chain = min(ppb, P) + nb + SL + 2
        bound = n_chain * U * absr + 2.0 ** -126
        ratio = float(((dw.double() - ref).abs() / bound).max())
        print(f"  {what}: err / bound {ratio:.3g} (n = {n_chain})")
        assert ratio <= 1.0, f"{what}: err / bound {ratio:.3g}"
        Stats.note(family or ("MwgradK" if mfma else "WgradK"), ratio)
    a.check_untouched(what + ": a")
    b.check_untouched(what + ": b")
    return note


def wgrad_geom(a_px, Ca, Cb, filt, pairing="conv"):
    """a (n, h, w) pixels; b's shape from the filter.  "conv": a = dy, b = the layer input; "convT": a = the layer input, b = dy of a
    stride-2 ConvTranspose2d (twice the size)."""
    R, S, stride, dil, ph, pw = FILTERS[filt]
    n, h, w = a_px
    if pairing == "convT":
        Hb, Wb = 2 * h, 2 * w
    else:
        Hb = (h - 1) * stride + dil * (R - 1) + 1 - 2 * ph + (stride - 1)
        Wb = (w - 1) * stride + dil * (S - 1) + 1 - 2 * pw + (stride - 1)
    return (n, h, w, Ca), (n, Hb, Wb, Cb), dict(R=R, S=S, stride=stride, dil=dil, pad_h=ph, pad_w=pw)


# ================================================================================================ 3. MwgradK and WgradRedK
MWGRAD_CASES = [
    # a pixels (n, h, w), Ca, Cb, filter, pairing, a dtype, tfa, b dtype, tfb, waves knob, slices
    ((41, 2, 3), 13, 1, "3x3s2", "conv", BF16, 0, F32, 0, 2048, 4),             # 13 x 9, 246 pixels: the 4-step floor gives 4 slices
    ((1190, 2, 3), 14, 14, "2x2s2", "conv", BF16, 0, BF16, 0, 2048, 112),       # 14 x 56: the last count without the fold's unrolled round
    ((3, 342, 7), 40, 24, "3x3", "conv", BF16, 0, F32, 2, 2048, 113),           # 40 x 216: the first count with it
    ((1205, 2, 3), 16, 16, "3x3s2", "convT", F32, 2, BF16, 0, 2048, 113),       # ConvTranspose2d: a = the layer input through tfa
    ((3, 391, 7), 64, 16, "1x1", "conv", BF16, 0, F32, 3, 2048, 129),           # 64 x 16: the unrolled round plus one slab
    ((3, 391, 7), 16, 16, "5x1", "conv", F16, 0, F32, 1, 2048, 129),            # f16; 16 x 80
    ((3, 729, 7), 32, 32, "1x1", "conv", BF16, 0, F32, 2, 2048, 240),           # one round and 7 x 16 slabs
    ((3, 729, 7), 32, 32, "3x3", "conv", BF16, 0, BF16, 0, 2048, 120),          # 32 x 288: 9 column tiles, 8 steps per slice
    ((3, 342, 7), 32, 32, "3x3d4", "conv", BF16, 0, F32, 3, 2048, 113),
    ((3, 342, 7), 128, 32, "1x1", "conv", BF16, 0, F32, 1, 2048, 113),          # 128 x 32: 4 row tiles
    ((10921, 2, 3), 13, 1, "3x3s2", "conv", BF16, 0, F32, 0, 2048, 1024),       # 65,526 pixels: exactly on the cap, 64 pixels per slice
    ((3, 149, 147), 16, 16, "1x1", "conv", BF16, 0, F32, 2, 2048, 514),         # 65,709: across it -- sps 5 -> 8
    ((10921, 2, 3), 128, 32, "3x3", "conv", BF16, 0, BF16, 0, 36864, 1024),     # 36 tiles x 1,024 slices through ENET_MWGRAD_WAVES
]


@gpu
@pytest.mark.parametrize("case", range(len(MWGRAD_CASES)), ids=_ids(MWGRAD_CASES))
def test_mwgrad_slices_and_fold(K, case):
    """MwgradK over the slice counts that change WgradRedK's path (4, 112 / 113, 129, 240, the 1,024 cap), pixel counts off the multiples
    of 16 and of a slice, images narrower than a lane's 8-pixel run (it wraps rows and images), ragged and full tiles."""
    a_px, Ca, Cb, filt, pairing, adt, tfa, bdt, tfb, waves, slices = MWGRAD_CASES[case]
    ad, bd, kw = wgrad_geom(a_px, Ca, Cb, filt, pairing)
    P, kb = ad[0] * ad[1] * ad[2], kw["R"] * kw["S"] * Cb
    mt, nt, pps, nsl = mwgrad_plan(Ca, kb, P, waves)
    assert nsl == slices and P % 16 and P % pps, (mwgrad_plan(Ca, kb, P, waves), P)
    D = Data("int", 500 + case, small=P > 60000)
    D.waves = waves
    with knobs(ENET_MWGRAD_WAVES=waves):
        wgrad_call(K, D, dense(ad, adt), dense(bd, bdt), kw, tfa, tfb, f"mwgrad {a_px} {Ca}x{kb} {filt} {pairing}",
                   expect=mwgrad_note(Ca, kb, P, waves))


@gpu
@pytest.mark.parametrize("below", [True, False])
def test_mwgrad_span_guard(K, below):
    """MwgradK addresses both operands with 32-bit element offsets; the host admits a view only while n sn + h sh + w sw + c < 2^31 - 1.
    ``a`` is a two-image view on an uninitialised buffer of ~2^30 elements with data in its two images only: just below the guard the
    result equals the reference, one image-stride step further the call raises and dw keeps its bits."""
    h, w, Ca, Cb = 9, 7, 32, 16
    img = h * w * Ca
    tail = h * (w * Ca) + w * Ca + Ca                      # h sh + w sw + c of the host's span
    sn = (0x7fffffff - 1 - tail) // 2 + (0 if below else 1)
    assert (2 * sn + tail < 0x7fffffff) == below
    D = Data("int", 900 + below)
    base = torch.empty(sn + img, dtype=BF16, device=DEV)
    a = base.as_strided((2, h, w, Ca), (sn, w * Ca, Ca, 1))
    for i in range(2):
        a[i] = D.grad((h, w, Ca), BF16)
    b = D.act((2, h, w, Cb), BF16)
    dw = D.seed_out((Ca * 9 * Cb,), F32)
    dw0 = dw.clone()
    kw = dict(R=3, S=3, pad_h=1, pad_w=1)
    if below:
        K.enet_wgrad(a, None, b, None, dw, **kw)
        note = plan_note()
        torch.cuda.synchronize()
        assert note == mwgrad_note(Ca, 9 * Cb, 2 * h * w), note
        ref = dw0.double() + wgrad_ref(a.double(), b.double(), 3, 3, 1, 1, 1, 1).reshape(-1)
        same_bits(dw, ref.float(), f"span just below 2^31 [{note}]")
    else:
        with pytest.raises(RuntimeError):
            K.enet_wgrad(a, None, b, None, dw, **kw)
        torch.cuda.synchronize()
        same_bits(dw, dw0, "dw after the refused call")
    del a, base
    torch.cuda.empty_cache()


# ================================================================================================ 4. WgradK<T, SL>
WGRADK_CASES = [
    # a pixels, Ca, Cb, filter, pairing, a dtype, tfa, b dtype, tfb, ENET_WGRAD_BLOCKS knob, (SL, blocks)
    ((5, 4, 5), 16, 64, "1x1", "conv", F32, 0, F32, 2, 1024, (4, 2)),           # 16 x 64: 32 register tiles -> 4 pixel slices per round
    ((3, 342, 7), 16, 16, "3x3", "conv", F32, 0, F32, 2, 1024, (2, 113)),       # 16 x 144: 72 tiles -> 2; the fold's unrolled round
    ((3, 729, 7), 32, 32, "3x3", "conv", BF16, 0, F32, 3, 1024, (1, 240)),      # 32 x 288: 288 tiles -> 1, two tiles per thread
    ((3, 391, 7), 16, 64, "1x1", "conv", BF16, 0, BF16, 0, 1024, (4, 129)),
    ((1205, 2, 3), 16, 16, "3x3s2", "convT", F32, 2, F32, 0, 1024, (2, 113)),
    ((3, 729, 7), 14, 14, "2x2s2", "conv", F32, 0, F32, 0, 113, (4, 96)),       # the knob's cap at 113: 160 pixels per block
    ((3, 149, 147), 24, 24, "5x1", "conv", BF16, 0, BF16, 0, 240, (2, 229)),    # ... at 240: 288 per block, the last one ragged
    ((3, 3121, 7), 13, 1, "3x3s2", "conv", F32, 0, F32, 0, 1024, (4, 683)),     # 65,541 pixels: across the 1,024 cap, 96 per block
    ((3, 3121, 7), 32, 32, "3x3d4", "conv", BF16, 0, F32, 1, 1024, (1, 683)),
]


@gpu
@pytest.mark.parametrize("case", range(len(WGRADK_CASES)), ids=_ids(WGRADK_CASES))
def test_wgradk_slices_and_blocks(K, case):
    """WgradK<T, SL> (fp32 mode; bf16 mode with ENET_MFMA bit 1 off) for SL = 4 / 2 / 1 and block counts on both sides of the fold's
    unrolled round and of the block cap, the last block ragged."""
    a_px, Ca, Cb, filt, pairing, adt, tfa, bdt, tfb, maxb, (SL, blocks) = WGRADK_CASES[case]
    ad, bd, kw = wgrad_geom(a_px, Ca, Cb, filt, pairing)
    P, kb = ad[0] * ad[1] * ad[2], kw["R"] * kw["S"] * Cb
    pl = wgradk_plan(Ca, kb, P, maxb)
    assert (pl[0], pl[2]) == (SL, blocks) and P % pl[1], (pl, P)
    D = Data("int", 700 + case, small=P > 60000)
    D.mfma_knob, D.max_blocks = 1, maxb
    with knobs(ENET_MFMA=1, ENET_WGRAD_BLOCKS=maxb):
        wgrad_call(K, D, dense(ad, adt), dense(bd, bdt), kw, tfa, tfb, f"wgradk {a_px} {Ca}x{kb} {filt} {pairing}",
                   expect=wgradk_note(Ca, kb, P, maxb))


@gpu
def test_wgradk_too_many_tiles_raise(K):
    """A 64 x 576 gradient has 1,152 register tiles (> 512): the fp32 call raises and dw keeps its bits."""
    assert wgradk_plan(64, 576, 63) is None
    D = Data("int", 2)
    a, b = D.grad((1, 9, 7, 64), F32), D.act((1, 9, 7, 64), F32)
    dw = D.seed_out((64 * 9 * 64,), F32)
    dw0 = dw.clone()
    with pytest.raises(RuntimeError):
        K.enet_wgrad(a, None, b, None, dw, R=3, S=3, pad_h=1, pad_w=1)
    torch.cuda.synchronize()
    same_bits(dw, dw0, "dw after the refused call")


# ================================================================================================ 5. fused forms at NT > 1
def fused_call(K, D, rawd, gd, md, yd, kw, act, bn_act=None, rgd=None, rmd=None, compute=BF16, what=""):
    """K.enet_conv_bwd_in (the BatchNorm backward of (raw, g [, mask]) computed while the data-gradient convolution loads) against
    K.enet_bn_bwd_apply followed by K.enet_conv / K.enet_conv_bnbwd_stats (``bn_act``: the output side's BatchNorm-backward rows are
    written as well): y bit for bit, the same row count, the same rows.  -> (note of the fused call, rows)."""
    n, H, W, C = rawd[0]
    _, Ho, Wo, Cx = yd[0]
    g = D.g
    vec = lambda c, lo=0.5: torch.rand(c, generator=g, device=DEV) + lo
    tf = K.Tf(vec(C), torch.randn(C, generator=g, device=DEV) * 0.3, vec(C, 0.0) * 0.5 if act == 2 else None, act)
    mean, invstd = torch.randn(C, generator=g, device=DEV), vec(C)
    c1c2 = torch.randn(2 * C, generator=g, device=DEV) * 0.1
    raw = Buf(rawd, torch.randn(rawd[0], generator=g, device=DEV) * 2 + 1)
    gy = Buf(gd, torch.randn(gd[0], generator=g, device=DEV).to(gd[3]))
    mask = Buf(md, torch.randn(md[0], generator=g, device=DEV).to(md[3])) if md is not None else None
    taps = kw["R"] * kw["S"]
    w = torch.randn(C * taps * Cx, generator=g, device=DEV) / math.sqrt(C * taps)
    acc = kw.get("accumulate", False)
    seed = torch.randn(yd[0], generator=g, device=DEV).to(yd[3]) if acc else None
    y1, y2 = Buf(yd, seed), Buf(yd, seed)
    rg = Buf(rgd, torch.randn(rgd[0], generator=g, device=DEV).to(rgd[3])) if rgd is not None else None
    rm = Buf(rmd, torch.randn(rmd[0], generator=g, device=DEV).to(rmd[3])) if rmd is not None else None
    draw = torch.full((n, H, W, C), float("nan"), dtype=gd[3], device=DEV)
    K.enet_bn_bwd_apply(raw.t, gy.t, mask.t if mask else None, tf, mean, invstd, c1c2, draw)
    tiles = cdiv(n * Ho * Wo, 32)
    bn = None
    rows1 = 0
    if bn_act is not None:
        rec_raw = torch.randn(yd[0], generator=g, device=DEV) * 2 + 1
        rec_tf = K.Tf(vec(Cx), torch.randn(Cx, generator=g, device=DEV) * 0.3, vec(Cx, 0.0) * 0.5 if bn_act == 2 else None, bn_act)
        rec_mean, rec_invstd = torch.randn(Cx, generator=g, device=DEV), vec(Cx)
        st1 = torch.full((tiles * Cx * 3,), float("nan"), dtype=torch.float64, device=DEV)
        st2 = st1.clone()
        kws = {k: v for k, v in kw.items() if k != "accumulate"}
        rows1 = K.enet_conv_bnbwd_stats(draw, w, y1.t, st1, rec_raw, rec_tf, rec_mean, rec_invstd, compute=compute, **kws)
        bn = (st2, rec_raw, rec_tf, rec_mean, rec_invstd)
    else:
        K.enet_conv(draw, w, None, None, y1.t, resid_grad=rg.t if rg else None, resid_mask=rm.t if rm else None, compute=compute, **kw)
    base_note = plan_note()
    rows2 = K.enet_conv_bwd_in(raw.t, w, tf, gy.t, mask.t if mask else None, mean, invstd, c1c2, y2.t,
                               resid_grad=rg.t if rg else None, resid_mask=rm.t if rm else None, compute=compute, bn=bn, **kw)
    note = plan_note()
    torch.cuda.synchronize()
    what = f"{what} [{note}]"
    assert rows2 is not None, what + ": no on-load form"
    assert rows1 == rows2 == (tiles if bn_act is not None else 0), (what, rows1, rows2, tiles)
    assert base_note.replace("gather", "*").replace("direct", "*") == note.replace("bwd-in", "*"), (base_note, note)
    assert bool(torch.isfinite(y1.t.float()).all()), what
    same_bits(y2.base, y1.base, what + ": y (and the bytes around it)")
    if bn_act is not None:
        same_bits(st2, st1, what + ": the BatchNorm-backward rows")
    return note, rows2


@gpu
@pytest.mark.parametrize("C,Cx,nt", [(64, 64, 2), (32, 128, 4)])
@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("bn_act", [None, 2])
def test_fused_bwd_in_at_nt(K, C, Cx, nt, use_mask, bn_act):
    """enet_conv_bwd_in at 3 x 149 x 147 pixels (2,054 tiles: NT = 2 for 64 outputs, NT = 4 for 128), with and without the mask and the
    BatchNorm-backward rows, against the separate path -- whose convolution `test_mconv_nt_edges` holds to float64 at these shapes."""
    xs, ys, kw = conv_geom(B1, C, Cx, "1x1", "gather")
    D = Data("gauss", 1100 + C + use_mask + (bn_act or 0))
    note, rows = fused_call(K, D, dense(xs, F32), dense(xs, BF16), dense(xs, BF16) if use_mask else None, dense(ys, BF16), kw,
                            act=2 if C == 64 else 3, bn_act=bn_act, what=f"bwd_in {C}->{Cx}")
    P = ys[0] * ys[1] * ys[2]
    assert note == mconv_note(Cx, P, "bwd-in", 0, 2 if bn_act else 0) and f"NT {nt}:" in note, note


# ================================================================================================ 6. tails
def tail_fwd_call(K, D, mode, rawd, outd, maind=None, rawmd=None, Cm=0, tfmode=2, tfm_mode=1, what=""):
    """K.enet_tail_fwd on exact-integer data.  -> (out Buf, idx) for the backward."""
    n, h, w, C = outd[0]
    tf, tfv = D.tf(K, rawd[0][3], tfmode)
    raw = Buf(rawd, D.raw(rawd[0], rawd[3]))
    ext = tf_ref(raw.t, tfv, tfmode)
    out = Buf(outd)
    idx = None
    if mode == 0:
        main = Buf(maind, D.raw(maind[0], maind[3]))
        K.enet_tail_fwd(raw.t, tf, main.t, None, None, None, 0, 0, out.t)
        ref = (main.t.double() + ext).clamp_min(0)
    elif mode == 1:
        main = Buf(maind, D.raw(maind[0], maind[3]))
        idx = torch.full((n, h, w, Cm), 0xA5, dtype=torch.uint8, device=DEV)
        K.enet_tail_fwd(raw.t, tf, main.t, None, None, idx, Cm, 1, out.t)
        pm, pc = pool_first_ref(main.t.double())
        ref = (F.pad(pm, (0, C - Cm)) + ext).clamp_min(0)
        torch.cuda.synchronize()
        same_bits(idx, pc, what + ": pooling codes")
    elif mode == 2:
        tfm, tfmv = D.tf(K, C, tfm_mode)
        rawm = Buf(rawmd, D.raw(rawmd[0], rawmd[3]))
        idx = torch.randint(0, 4, (n, h // 2, w // 2, C), generator=D.g, device=DEV, dtype=torch.int32).to(torch.uint8)
        K.enet_tail_fwd(raw.t, tf, None, rawm.t, tfm, idx, C, 2, out.t)
        zm = tf_ref(rawm.t, tfmv, tfm_mode)
        up = torch.zeros(n, h, w, C, dtype=torch.float64, device=DEV)
        for k in range(4):
            up[:, (k >> 1)::2, (k & 1)::2, :] = torch.where(idx == k, zm, torch.zeros_like(zm))
        ref = (up + ext).clamp_min(0)
    else:
        main = Buf(maind, D.act(maind[0], maind[3]))
        K.enet_tail_fwd(raw.t, tf, main.t, None, None, None, rawd[0][3], 3, out.t)
        ref = torch.cat([ext, pool_first_ref(main.t.double())[0]], 3)
    torch.cuda.synchronize()
    out.check_out(ref.float().to(outd[3]), what + ": out")
    return out, idx


def tail_bwd_call(K, D, mode, doutd, maskd, dstd, Cm, acc, idx=None, what=""):
    """K.enet_tail_bwd on exact-integer data: mode 1 routes dout (gated by out > 0) to the argmax position at double resolution, mode 2
    gathers it at half resolution, mode 3 routes channel Cm of dout to the image's argmax (no gate)."""
    n, H, W, C = dstd[0]
    dout = Buf(doutd, D.grad(doutd[0], doutd[3]))
    if mode == 3:
        mask = Buf(maskd, D.act(maskd[0], maskd[3]))                 # the input image
    else:
        mask = Buf(maskd, D.raw(maskd[0], maskd[3]).clamp_min(0))     # a block output: about a third zeros
    dst = Buf(dstd, D.seed_out(dstd[0], dstd[3]) if acc else None)
    if idx is None and mode != 3:
        ish = doutd[0][:3] if mode == 1 else dstd[0][:3]
        idx = torch.randint(0, 4, (*ish, Cm), generator=D.g, device=DEV, dtype=torch.int32).to(torch.uint8)
    K.enet_tail_bwd(dout.t, mask.t, idx, Cm, mode, dst.t, accumulate=acc)
    torch.cuda.synchronize()
    d64 = dout.t.double()
    if mode == 3:
        code = pool_first_ref(mask.t.double())[1]
        gz = d64[..., Cm:Cm + 1]
    else:
        code = idx
        gz = torch.where(mask.t.double() > 0, d64, torch.zeros_like(d64))
    ref = torch.zeros(dstd[0], dtype=torch.float64, device=DEV)
    if mode == 2:
        for k in range(4):
            ref += torch.where(code == k, gz[:, (k >> 1)::2, (k & 1)::2, :], torch.zeros_like(ref))
    else:
        gz = gz[..., :Cm] if mode == 1 else gz
        for k in range(4):
            ref[:, (k >> 1)::2, (k & 1)::2, :C] = torch.where(code == k, gz, torch.zeros_like(gz))
    if acc:
        ref = ref + dst.old().double()
    dst.check_out(ref.float().to(dstd[3]), what + ": dst")


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_tails_stage_shapes(K, dt, mode):
    """The bottleneck tails at stage shapes with odd halves (25 x 25 <-> 50 x 50, 14 and 64 channels): integer data tie constantly, so
    the uint8 argmax codes are a test of the first-maximum rule; forward (modes 0-3) and backward (modes 1-3, also accumulating)."""
    D = Data("int", 1300 + mode)
    B = 3
    what = f"tail mode {mode} {dt}"
    if mode == 0:
        for C in (14, 64):
            tail_fwd_call(K, D, 0, dense((B, 25, 25, C), F32), wide((B, 25, 25, C), dt, 2, 1), wide((B, 25, 25, C), dt, 1, 3), what=what)
        return
    if mode == 1:
        out, idx = tail_fwd_call(K, D, 1, dense((B, 25, 25, 64), F32), dense((B, 25, 25, 64), dt), dense((B, 50, 50, 14), dt), Cm=14,
                                 what=what)
        for acc in (False, True):
            tail_bwd_call(K, D, 1, dense((B, 25, 25, 64), dt), dense((B, 25, 25, 64), dt), wide((B, 50, 50, 14), dt, 1, 1), 14, acc, idx,
                          what + f" bwd acc={acc}")
        return
    if mode == 2:
        for C in (14, 64):
            tail_fwd_call(K, D, 2, dense((B, 50, 50, C), F32), dense((B, 50, 50, C), dt), rawmd=dense((B, 25, 25, C), F32), what=what)
            for acc in (False, True):
                tail_bwd_call(K, D, 2, dense((B, 50, 50, C), dt), dense((B, 50, 50, C), dt), dense((B, 25, 25, C), dt), C, acc,
                              what=what + f" bwd acc={acc}")
        return
    tail_fwd_call(K, D, 3, dense((B, 25, 25, 13), F32), dense((B, 25, 25, 14), dt), dense((B, 50, 50, 1), F32), what=what)
    for acc in (False, True):
        tail_bwd_call(K, D, 3, dense((B, 25, 25, 14), dt), dense((B, 50, 50, 1), F32), dense((B, 50, 50, 1), F32), 13, acc,
                      what=what + f" bwd acc={acc}")


# ================================================================================================ Gaussian data
def _report(family):
    print(f"largest err / bound: {family} {Stats.worst.get(family, float('nan')):.3g}")
    assert family in Stats.worst


@gpu
def test_gaussian_mconv(K):
    """MconvK on Gaussian data within the bound of the module docstring: NT = 1, 2 and 4, direct and gather, fp32 and bf16 stores."""
    Stats.worst.pop("MconvK", None)
    for i, (px, cin, cout, filt, form, xdt, mode, ydt, opts) in enumerate([
            (A0, 32, 128, "1x1", "direct", F32, 2, F32, "bias"), (B1, 32, 128, "3x3", "direct", F32, 3, F32, "bias"),
            (B1, 16, 64, "1x1", "direct", F32, 2, F32, "bias"), (A1, 128, 32, "3x3", "direct", BF16, 0, BF16, ""),
            (B1, 32, 128, "3x3", "gather", BF16, 0, F32, "acc"), (B1, 16, 64, "2x2s2", "gather", BF16, 0, BF16, "resid"),
            (B1, 16, 64, "3x3s2", "convT", F32, 3, F32, "bias")]):
        xs, ys, kw = conv_geom(px, cin, cout, filt, form)
        kw["accumulate"] = "acc" in opts
        r = dense(ys, BF16) if "resid" in opts else None
        conv_call(K, Data("gauss", 2000 + i), dense(xs, xdt), dense(ys, ydt), kw, mode, "bias" in opts, r, r, BF16,
                  f"gaussian mconv {cin}->{cout} {filt} {form}")
    _report("MconvK")


@gpu
def test_gaussian_convk(K):
    """ConvK on Gaussian data: fp32 mode and the bf16 mode's ragged widths."""
    Stats.worst.pop("ConvK", None)
    for i, (px, cin, cout, filt, form, xdt, mode, ydt, compute, opts) in enumerate([
            (S3, 13, 13, "3x3", "direct", F32, 2, F32, F32, "bias"), (S3, 16, 64, "3x3s2", "direct", F32, 2, F32, F32, "bias"),
            (S3, 24, 40, "3x3", "direct", BF16, 0, BF16, BF16, ""), (S3, 40, 24, "3x3", "gather", BF16, 0, BF16, BF16, "resid,acc"),
            ((2, 100, 100), 1, 13, "3x3s2", "direct", F32, 0, F32, BF16, "bias")]):
        xs, ys, kw = conv_geom(px, cin, cout, filt, form)
        kw["accumulate"] = "acc" in opts
        r = dense(ys, compute) if "resid" in opts else None
        conv_call(K, Data("gauss", 2100 + i), dense(xs, xdt), dense(ys, ydt), kw, mode, "bias" in opts, r, r, compute,
                  f"gaussian convk {cin}->{cout} {filt} {form}")
    _report("ConvK")


@gpu
def test_gaussian_mwgrad(K):
    """MwgradK + WgradRedK on Gaussian data: 113, 514 and 1,024 slices."""
    Stats.worst.pop("MwgradK", None)
    for i, (a_px, Ca, Cb, filt, pairing, adt, tfa, bdt, tfb) in enumerate([
            ((3, 342, 7), 40, 24, "3x3", "conv", BF16, 0, F32, 2), ((3, 149, 147), 16, 16, "1x1", "conv", BF16, 0, F32, 3),
            ((10921, 2, 3), 13, 1, "3x3s2", "conv", BF16, 0, F32, 0), ((1205, 2, 3), 16, 16, "3x3s2", "convT", F32, 2, BF16, 0)]):
        ad, bd, kw = wgrad_geom(a_px, Ca, Cb, filt, pairing)
        wgrad_call(K, Data("gauss", 2200 + i), dense(ad, adt), dense(bd, bdt), kw, tfa, tfb, f"gaussian mwgrad {a_px} {Ca}x{Cb} {filt}")
    _report("MwgradK")


@gpu
def test_gaussian_wgradk(K):
    """WgradK + WgradRedK on Gaussian data: SL = 4, 2 and 1; 2, 113, 240 and 683 blocks."""
    Stats.worst.pop("WgradK", None)
    for i, (a_px, Ca, Cb, filt, adt, bdt, tfb) in enumerate([
            ((5, 4, 5), 16, 64, "1x1", F32, F32, 2), ((3, 342, 7), 16, 16, "3x3", F32, F32, 2),
            ((3, 729, 7), 32, 32, "3x3", F32, F32, 3), ((3, 3121, 7), 13, 1, "3x3s2", F32, F32, 0)]):
        ad, bd, kw = wgrad_geom(a_px, Ca, Cb, filt)
        wgrad_call(K, Data("gauss", 2300 + i), dense(ad, adt), dense(bd, bdt), kw, 0, tfb, f"gaussian wgradk {a_px} {Ca}x{Cb} {filt}")
    _report("WgradK")


# ================================================================================================ 7. replay of the model's own calls
REC_FNS = ("enet_conv", "enet_conv_stats", "enet_conv_bwd_in", "enet_conv_bnbwd_stats", "enet_wgrad", "enet_channel_sum",
           "enet_tail_fwd", "enet_tail_bwd")
CONFIGS = {   # name -> (H, C, B, compute dtype, with d/dx)
    "cfg5": (320, 2, 20, BF16, False),
    "fp32": (200, 2, 2, F32, True),
}


def _desc(v):
    if isinstance(v, torch.Tensor):
        return ("T", desc_of(v))
    if isinstance(v, (list, tuple)):
        return type(v)(_desc(e) for e in v)
    if type(v).__name__ == "Tf":
        return ("Tf", int(v.mode), v.slope is not None)
    return v


def _sig(v):
    """The signature that de-duplicates: offsets only modulo 64 elements (the alignment)."""
    if isinstance(v, tuple) and len(v) == 2 and v[0] == "T":
        s, st, off, dt = v[1]
        return ("T", s, st, off % 64, str(dt))
    if isinstance(v, (list, tuple)):
        return tuple(_sig(e) for e in v)
    if isinstance(v, dict):
        return tuple(sorted((k, _sig(e)) for k, e in v.items()))
    return str(v) if isinstance(v, torch.dtype) else v


_RECORDED = {}


def recorded(K, cfg):
    """The distinct Enet conv-family calls of one eager training forward + backward of get_arch("enet") for ``cfg``:
    {fn: [(args, kwargs), ...]} with tensors replaced by ("T", (shape, stride, offset, dtype)) and transforms by ("Tf", mode, slope?)."""
    if cfg in _RECORDED:
        return _RECORDED[cfg]
    from dct_amd.arch import get_arch
    H, C, B, dt, need_dx = CONFIGS[cfg]
    torch.manual_seed(5)
    net = get_arch("enet", {"num_classes": C, "compute_dtype": dt}).to(DEV).train()
    calls, depth = [], [0]
    orig = {f: getattr(K, f) for f in REC_FNS}

    def wrap(name):
        def fn(*a, **kw):
            if depth[0] == 0:
                calls.append((name, _desc(a), {k: _desc(v) for k, v in kw.items()}))
            depth[0] += 1
            try:
                return orig[name](*a, **kw)
            finally:
                depth[0] -= 1
        return fn
    for f in REC_FNS:
        setattr(K, f, wrap(f))
    try:
        x = torch.rand(B, 1, H, H, generator=gen(1), device=DEV).requires_grad_(need_dx)
        out = net(x)
        out.backward(torch.randn(out.shape, generator=gen(2), device=DEV))
    finally:
        for f in REC_FNS:
            setattr(K, f, orig[f])
    torch.cuda.synchronize()
    del net, out, x
    torch.cuda.empty_cache()
    distinct, seen = {f: [] for f in REC_FNS}, set()
    for name, a, kw in calls:
        s = (name, _sig(a), _sig(kw))
        if s not in seen:
            seen.add(s)
            distinct[name].append((a, kw))
    _RECORDED[cfg] = (len(calls), distinct)
    return _RECORDED[cfg]


def _T(d):
    assert isinstance(d, tuple) and d[0] == "T", d
    return d[1]


def _To(d):
    return _T(d) if d is not None else None


def _mode(d):
    return d[1] if d is not None else 0


def _pixels(d):
    s = _T(d)[0]
    return s[0] * s[1] * s[2]


def _conv_kw(kw):
    return {k: v for k, v in kw.items() if k in ("R", "S", "stride", "dil", "pad_h", "pad_w", "transposed", "ws", "accumulate")}


def conv_expect(xd, yd, kw, compute, stats_code):
    """The note the planner mirrors predict for a recorded convolution."""
    (cin, xdt), (cout, P) = (xd[0][3], xd[3]), (yd[0][3], yd[0][0] * yd[0][1] * yd[0][2])
    low = compute if compute != F32 else xdt
    if takes_mfma(low, cin, cout):
        ws = kw["ws"]
        wvec = int(ws[2] == 1 and ws[0] % 4 == 0 and ws[1] % 4 == 0)
        return mconv_note(cout, P, "gather" if kw.get("transposed") else "direct", wvec, stats_code)
    return convk_note(cin, cout, kw["R"] * kw["S"], P)


def replay_conv(K, cfg, i, fn, a, kw):
    compute = kw.get("compute") or F32
    ckw = _conv_kw(kw)
    if fn == "enet_conv_bnbwd_stats":
        xd, wd, yd, std, rrawd, rtfd, rmeand, rinvd = a
        stats, code, tfd, bd = ("bnbwd", _T(rrawd), rtfd[1], _T(rmeand), _T(rinvd)), 2, None, None
    elif fn == "enet_conv_stats":
        xd, wd, bd, tfd, yd, std = a
        stats, code = "fwd", 1
    else:
        xd, wd, bd, tfd, yd = a
        stats, code = False, 0
    D = Data("int", 3000 + i, small=bool(stats))       # (narrow data keep a tile's sum of squares within the exact range)
    what = f"{cfg} {fn}[{i}] {_T(xd)[0]} -> {_T(yd)[0]}"
    return conv_call(K, D, _T(xd), _T(yd), ckw, _mode(tfd), bd is not None, _To(kw.get("resid_grad")), _To(kw.get("resid_mask")),
                     compute, what, stats=stats, expect=conv_expect(_T(xd), _T(yd), ckw, compute, code))


def replay_wgrad(K, cfg, i, a, kw):
    ad, tfa, bd, tfb, dwd = a
    P = _pixels(ad)
    Ca, kb = _T(ad)[0][3], kw["R"] * kw["S"] * _T(bd)[0][3]
    low = _T(ad)[3] != F32 or _T(bd)[3] != F32             # a bf16 / f16 operand: the MFMA form
    D = Data("int", 4000 + i, small=P > 60000)
    return wgrad_call(K, D, _T(ad), _T(bd), dict(kw), _mode(tfa), _mode(tfb), f"{cfg} enet_wgrad[{i}] {_T(ad)[0]} x {_T(bd)[0]}",
                      expect=mwgrad_note(Ca, kb, P) if low else wgradk_note(Ca, kb, P))


def replay_channel_sum(K, cfg, i, a, kw):
    xd, od = a
    P = _pixels(xd)
    D = Data("int", 6000 + i, small=P > 60000)
    x = Buf(_T(xd), D.grad(_T(xd)[0], _T(xd)[3]))
    out = D.seed_out(_T(od)[0], F32)
    out0 = out.clone()
    K.enet_channel_sum(x.t, out)
    torch.cuda.synchronize()
    assert_exact_range(x.t.double().abs().sum((0, 1, 2)) + 8, "channel sum")
    same_bits(out, (out0.double() + x.t.double().sum((0, 1, 2))).float(), f"{cfg} enet_channel_sum[{i}] {_T(xd)[0]}")


def replay_tail(K, cfg, i, name, a, kw):
    D = Data("int", 7000 + i)
    if name == "enet_tail_fwd":
        rawd, tfd, maind, rawmd, tfmd, idxd, Cm, mode, outd = a
        tail_fwd_call(K, D, mode, _T(rawd), _T(outd), _To(maind), _To(rawmd), Cm if mode == 1 else 0, _mode(tfd), _mode(tfmd) or 1,
                      what=f"{cfg} enet_tail_fwd[{i}] mode {mode} {_T(outd)[0]}")
    else:
        doutd, maskd, idxd, Cm, mode, dstd = a
        tail_bwd_call(K, D, mode, _T(doutd), _T(maskd), _T(dstd), Cm, kw.get("accumulate", False),
                      what=f"{cfg} enet_tail_bwd[{i}] mode {mode} {_T(dstd)[0]}")


# what each configuration's eager step issues (fp32 mode has no fused statistics; no eager step computes the BatchNorm backward on load)
ISSUED = {"cfg5": ("enet_conv", "enet_conv_stats", "enet_conv_bnbwd_stats", "enet_wgrad", "enet_channel_sum", "enet_tail_fwd", "enet_tail_bwd"),
          "fp32": ("enet_conv", "enet_wgrad", "enet_channel_sum", "enet_tail_fwd", "enet_tail_bwd")}


@gpu
@pytest.mark.parametrize("cfg,fn", [(c, f) for c in CONFIGS for f in ISSUED[c]])
def test_recorded_calls(K, cfg, fn):
    """The distinct calls of ``fn`` in one eager training step of the model, replayed on fresh exact-integer data of the same geometry
    (views, strides and keywords kept): the convolutions (their statistics-rows forms included), weight gradients, bias sums and tails
    bit for bit against float64, each under the plan note the mirrors predict for it."""
    total, distinct = recorded(K, cfg)
    for f in REC_FNS:
        assert bool(distinct[f]) == (f in ISSUED[cfg]), f"{cfg}: {f} has {len(distinct[f])} recorded calls: ISSUED and the replays must follow"
    notes = []
    checked = dict(ROWS_CHECKED)
    for i, (a, kw) in enumerate(distinct[fn]):
        if fn in ("enet_conv", "enet_conv_stats", "enet_conv_bnbwd_stats"):
            notes.append(replay_conv(K, cfg, i, fn, a, kw))
        elif fn == "enet_wgrad":
            notes.append(replay_wgrad(K, cfg, i, a, kw))
        elif fn == "enet_channel_sum":
            replay_channel_sum(K, cfg, i, a, kw)
        else:
            replay_tail(K, cfg, i, fn, a, kw)
    print(f"{cfg}: {total} recorded calls; {fn}: {len(distinct[fn])} distinct; plans: {sorted(set(notes))}")
    if fn == "enet_conv_stats":
        sums, squares = (ROWS_CHECKED[k] - checked[k] for k in ("sum", "squares"))
        print(f"{cfg}: statistics rows compared exactly: sums {sums}, sums of squares {squares} of {len(distinct[fn])}")
        assert sums == squares == len(distinct[fn]), (sums, squares)
    if cfg == "cfg5" and fn == "enet_conv":
        assert any(" NT 2:" in s for s in notes), "no NT = 2 convolution in cfg5's step"
    if cfg == "cfg5" and fn == "enet_wgrad":         # the initial 1 -> 13 convolution: 512,000 pixels, sps 16 -> 32 under the cap
        assert "enet mwgrad 1 x 1 tiles: pps 512, 1000 slices" in notes, "no weight gradient at the 1,024-slice cap in cfg5's step"
    if cfg == "fp32":
        assert all(s.startswith(("enet conv valu", "enet wgrad valu")) for s in notes), notes
