"""The data-movement kernels of csrc/pointwise.hip at training scale, against float64 references: 2x2 ceil-mode max pooling with and
without routing codes (``K.maxpool_fwd``), un-pooling from x, from codes and with the skip connection's gather (``K.maxpool_bwd``), the
bilinear resize (``K.bilinear_fwd``, ``K.bilinear_fwd_batched``, ``K.bilinear_bwd``: vector, scalar and eight-lane "split" kernels), Philox
dropout (``K.dropout_fwd`` with a host offset and with the device counter, ``K.dropout_apply``, ``K.dropout_maxpool_fwd``), ``K.relu_bwd``,
``K.cast`` and the weight repacks (``K.pack_weight``, ``K.pack_weights_batched`` on 32- and 64-edge tiles).

References (plain, float64; the unmarked tests check them on the CPU):
  * `resize_mats(n_in, n_out)` -> (W, S, delta): the align_corners interpolation matrix W[j, i] = max(0, 1 - |r_j - i|) with
    r_j = j (n_in - 1) / (n_out - 1), its support S widened by delta = 2 U (n_in - 1) + 2 U (U = 2^-24: what an fp32 ``scale * j`` can be off
    by).  Forward y = Wh x Ww^T, backward dx = Wh^T dy Ww, as einsums on NHWC; equal to F.interpolate(float64) and its autograd to 1e-12.
  * `pool_ref` (first maximum in scan order, bit 2 = maximum > 0, code 8 = no maximum) and `unpool_ref`, which scatters by the codes;
    equal to F.max_pool2d(ceil_mode=True) and its gradient on tie-free data.
  * `philox4x32_10` in numpy uint64 from the published round function, held to the Random123 known-answer vectors, and `dropout_keep`,
    the kernel's mapping onto it: key = (seed lo, seed hi), counter = (c lo, c hi, 0, 0) with c = offset + g, g the index of the
    4-channel group in the dense [n][h][w][c / 4] walk; lane i keeps iff (r_i >> 8) 2^-24 >= p in fp32; the value is
    fl32(x fl32(1 / (1 - p))) rounded once to the storage type, else 0.
  * every fp32 product of the reference (a scale, a dropout factor) is the float64 product of the two fp32 numbers rounded once.

Exact cases, bit for bit.  Bilinear sizes with a dyadic (in - 1) / (out - 1) make the scale, every ``scale * j``, every weight and every
weight product exact in fp32; on small-integer data every sum is then exact whatever the FMA contraction, and the kernel must equal the
float64 reference exactly for fp32 and after one round-to-nearest-even for bf16: a lost, duplicated or mis-weighted candidate -- of the
widened range of the gather, of the eight-lane fold on a ragged last block, on either side of the split kernel's 262,144-group threshold
-- fails at any magnitude.  Pooling and un-pooling move values (integers in [0, 3]: most windows hold ties), dropout draws a stream that
the reference reproduces, relu_bwd / cast / repack move or round single values: all bit for bit.  Outputs are pre-filled with NaN, or
with known integers where the kernel accumulates; channel slices sit in wider buffers whose other bytes must keep their bits.

Derived bounds, at the sizes get_arch("unet") issues (Gaussian data).  The kernel's fp32 ``scale * j`` is off by up to delta, so each
weight is off by at most delta on the support S; first order, with 1 % slack:
    forward   |y - ref|  <= dh (Sh |x| Ww^T) + dw (Wh |x| Sw^T) + 8 U (Wh |x| Ww^T)        (+ 2^-8 |ref| for a bf16 store)
    backward  |dx - ref| <= dh (Sh^T |dy| Ww) + dw (Wh^T |dy| Sw) + n U (Wh^T |dy| Ww)     (+ 2^-8 |ref| for a bf16 store)
with n = (largest column sum of Sh) x (largest column sum of Sw) + 4.  The un-pooling with the skip gather carries the backward bound of
its gather + 2 U |dy + gather| for the fp32 sum and the scale, routed like the values.  `test_bound_holds_for_torch_fp32` keeps the
bound honest on the CPU with torch's fp32 resize in the kernel's place (err / bound 0.01 ... 0.59 over the sizes).  The hip_ops fall-back
of the skip gather for views off the vector width (the accumulating scalar bilinear backward onto a copy of dy, then the one-element-per-
thread un-pooling) forms dy + gather in memory, in the storage type: one more bf16 half-ulp on the sum there.

Largest err / bound per family, as printed on an MI355X (the bf16 figures are the store's half ulp, which reaches 2^-8 |ref| just above a
power of two):

    family               bf16 store   fp32     worst fp32 case
    bilinear forward     0.995        0.331    98 -> 24, C = 64
    bilinear backward    0.994        0.589    24 -> 98, C = 64
    skip gather          0.996        0.588    x 196 <- skip 24, C = 64
    (fall-back, sum formed in memory: 0.496 bf16, 0.186 fp32; logits 84 -> 256, C = 4: forward 0.253, split backward 0.221)

`test_model_geometry_is_covered` runs one eager training forward + backward of get_arch("unet") at B = 1 (256^2 bf16, 200^2 bf16 with
d/dx, 256^2 fp32) with the pointwise functions of hip_ops wrapped: every recorded (function, dtype, C, spatial sizes, flags) must be one
that the tables below replay (`COVERED`); a recording that differs fails.

Not here: the 64-bit branch of `decode` (more than 2^31 vector groups: tens of GB), and the stem, head and bias-gradient kernels
(test_conv_kernels_scale_gpu.py has them)."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_kernels_scale_gpu import Buf, Stats, cdiv, compare, desc_of, gen, ints, nan_fill, pool_ref, same_bits

gpu = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
UB = 2.0 ** -8
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [BF16, F32]
S07 = float(np.float32(1.0) / np.float32(0.7))          # fl32(1 / 0.7): the un-dropout scale of p = 0.3
FLAGS = [(False, 1.0), (True, 2.0), (True, S07)]         # (relu_mask, scale)


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).replace("torch.", "")
    if isinstance(v, (tuple, list)):
        return "x".join(_id(e) for e in v)
    return str(v)


# ================================================================================================ references (float64, any device)
def resize_mats(n_in, n_out, device="cpu"):
    """-> (W, S, delta) of one axis of an align_corners resize n_in -> n_out (module docstring)."""
    j = torch.arange(n_out, dtype=torch.float64, device=device)
    i = torch.arange(n_in, dtype=torch.float64, device=device)
    r = j * (n_in - 1) / (n_out - 1) if n_out > 1 else torch.zeros_like(j)
    d = (r[:, None] - i[None, :]).abs()
    delta = 2 * U * (n_in - 1) + 2 * U
    return (1 - d).clamp_min(0), (d < 1 + delta).to(torch.float64), delta


def resize_fwd(x, A, B):
    """y[n, j, k, c] = sum A[j, h] x[n, h, w, c] B[k, w]."""
    return torch.einsum("njwc,kw->njkc", torch.einsum("jh,nhwc->njwc", A, x), B)


def resize_bwd(dy, A, B):
    """dx[n, h, w, c] = sum A[j, h] dy[n, j, k, c] B[k, w]."""
    return torch.einsum("nhkc,kw->nhwc", torch.einsum("jh,njkc->nhkc", A, dy), B)


def resize_bound(a, mh, mw, n_u, apply):
    """The first-order bound of the module docstring on |a| = |x| (apply = resize_fwd) or |dy| (apply = resize_bwd), 1 % slack."""
    (Wh, Sh, dh), (Ww, Sw, dw) = mh, mw
    return 1.01 * (dh * apply(a, Sh, Ww) + dw * apply(a, Wh, Sw) + n_u * U * apply(a, Wh, Ww))


def bwd_chain(mh, mw):
    return int(mh[1].sum(0).max() * mw[1].sum(0).max()) + 4


def unpool_ref(codes, g, shape, relu_mask=False, scale=1.0):
    """The un-pooling of g [n, Hp, Wp, C] to ``shape`` = [n, H, W, C] by the codes of `pool_ref`: g goes to window position code & 3,
    nowhere with code 8; with relu_mask it is first multiplied by scale where bit 2 is set and dropped elsewhere.  The product is the
    float64 one, rounded once when g is fp32.  In g's dtype."""
    n, H, W, C = shape
    Hp, Wp = cdiv(H, 2), cdiv(W, 2)
    if relu_mask:
        prod = (g.double() * float(scale)).to(g.dtype)
        g = torch.where((codes & 4) != 0, prod, torch.zeros_like(g))
    out = torch.zeros(n, 2 * Hp, 2 * Wp, C, dtype=g.dtype, device=g.device)
    for k in range(4):
        out[:, k >> 1::2, k & 1::2, :] = torch.where((codes & 11) == k, g, torch.zeros_like(g))
    return out[:, :H, :W, :]


_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(key, ctr):
    """Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): key (k0, k1) and
    counter (c0, c1, c2, c3) as uint64 arrays holding 32-bit words -> four arrays of 32-bit words."""
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _M32 for k in key)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in ctr)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def dropout_keep(shape, p, seed, offset):
    """The keep mask (bool numpy [n, h, w, c]) of the dropout kernels for a view of ``shape`` (module docstring)."""
    n, h, w, c = shape
    assert c % 4 == 0
    G = n * h * w * (c // 4)
    with np.errstate(over="ignore"):
        ctr = np.uint64(offset & (2 ** 64 - 1)) + np.arange(G, dtype=np.uint64)         # wraps modulo 2^64, as the kernel's sum
    zero = np.zeros(G, dtype=np.uint64)
    r = philox4x32_10((np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)), (ctr & _M32, ctr >> _S32, zero, zero))
    u = (np.stack(r, axis=-1) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).reshape(n, h, w, c)


def dropout_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_ref(x, p, seed, offset):
    """-> (mask uint8, dropped values in x's dtype), on x's device."""
    keep = torch.from_numpy(dropout_keep(tuple(x.shape), p, seed, offset)).to(x.device)
    val = (x.double() * dropout_scale(p)).float()
    return keep.to(torch.uint8), torch.where(keep, val, torch.zeros_like(val)).to(x.dtype)


# ------------------------------------------------------------------------------------------------ the references on the CPU
MODEL_RESIZES = [(126, 88, 64), (61, 48, 128), (29, 28, 256), (13, 18, 512),        # 256^2: pooled size -> concatenation size, channels
                 (98, 24, 64), (47, 16, 128), (22, 12, 256), (9, 10, 512)]          # 200^2
MODEL_LOGITS = [(84, 256, 4), (84, 256, 2), (20, 200, 2)]                           # fp32


def test_resize_reference_matches_interpolate():
    g = torch.Generator().manual_seed(0)
    for (hi, wi, ho, wo) in [(13, 18, 18, 13), (7, 5, 1, 9), (1, 5, 7, 9), (29, 29, 28, 28), (20, 17, 61, 40), (33, 9, 9, 33), (6, 6, 6, 6)]:
        x = torch.randn(2, 3, hi, wi, generator=g, dtype=torch.float64, requires_grad=True)
        y = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
        (Wh, _, _), (Ww, _, _) = resize_mats(hi, ho), resize_mats(wi, wo)
        got = resize_fwd(x.detach().permute(0, 2, 3, 1), Wh, Ww)
        assert torch.allclose(got.permute(0, 3, 1, 2), y, rtol=0, atol=1e-12)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        (dx,) = torch.autograd.grad(y, x, dy)
        got = resize_bwd(dy.permute(0, 2, 3, 1), Wh, Ww)
        assert torch.allclose(got.permute(0, 3, 1, 2), dx, rtol=0, atol=1e-12)


def test_resize_support_holds_the_weights():
    """S covers W's support, and at most one more candidate on each side of it."""
    for n_in, n_out in [(126, 88), (84, 256), (13, 18), (9, 10), (20, 200), (257, 1025), (97, 1), (1, 7), (5, 9)]:
        W, S, delta = resize_mats(n_in, n_out)
        assert bool((S[W > 0] == 1).all()) and delta == 2 * U * n_in
        assert float((S - (W > 0).double()).sum(1).max()) <= 2
        assert torch.allclose(W.sum(1), torch.ones(n_out, dtype=torch.float64), rtol=0, atol=1e-12)


def test_pool_reference_matches_max_pool2d():
    """pool_ref / unpool_ref against F.max_pool2d(ceil_mode=True) and its gradient on tie-free data (a permutation), odd extents."""
    g = torch.Generator().manual_seed(1)
    for (n, H, W, C) in [(2, 7, 9, 3), (1, 8, 6, 4), (1, 1, 7, 2), (2, 5, 1, 2)]:
        x = (torch.randperm(n * H * W * C, generator=g).double() - 100.0).reshape(n, C, H, W).requires_grad_(True)
        y = F.max_pool2d(x, 2, stride=2, ceil_mode=True)
        m, codes = pool_ref(x.detach().permute(0, 2, 3, 1))
        assert torch.equal(m.permute(0, 3, 1, 2), y.detach())
        assert torch.equal((codes & 4) != 0, m > 0) and int((codes & 8).sum()) == 0
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        (dx,) = torch.autograd.grad(y, x, dy)
        got = unpool_ref(codes, dy.permute(0, 2, 3, 1), (n, H, W, C))
        assert torch.equal(got.permute(0, 3, 1, 2), dx)
        got = unpool_ref(codes, dy.permute(0, 2, 3, 1), (n, H, W, C), relu_mask=True, scale=2.0)
        assert torch.equal(got.permute(0, 3, 1, 2), dx * 2.0 * (x.detach() > 0))


def test_pool_reference_takes_the_first_maximum():
    x = torch.tensor([[3.0, 3.0, 1.0, 2.0], [3.0, 0.0, 2.0, 2.0]], dtype=torch.float64).reshape(1, 2, 4, 1)
    m, codes = pool_ref(x)
    assert m.flatten().tolist() == [3.0, 2.0] and codes.flatten().tolist() == [0 | 4, 1 | 4]
    got = unpool_ref(codes, torch.tensor([5.0, 7.0], dtype=torch.float64).reshape(1, 1, 2, 1), (1, 2, 4, 1))
    assert got.flatten().tolist() == [5.0, 0.0, 0.0, 7.0, 0.0, 0.0, 0.0, 0.0]


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32_10, one at a time and as one array call."""
    for ctr, key, want in KAT:
        got = philox4x32_10([np.array([k]) for k in key], [np.array([c]) for c in ctr])
        assert tuple(int(v[0]) for v in got) == want, [hex(int(v[0])) for v in got]
    got = philox4x32_10([np.array([k[1][i] for k in KAT]) for i in range(2)], [np.array([k[0][i] for k in KAT]) for i in range(4)])
    assert [tuple(int(v[j]) for v in got) for j in range(3)] == [k[2] for k in KAT]


def test_dropout_reference_keep_rate():
    """A condition on the reference alone: over 640,000 elements the keep rate lies within 5 standard deviations of 1 - p."""
    shape = (2, 25, 25, 512)
    N = 2 * 25 * 25 * 512
    for p, seed, offset in [(0.5, 1234, 0), (0.3, 0x9E3779B97F4A7C15, 7 << 40), (0.5, 99, 2 ** 32 - 37), (0.3, 7, 0)]:
        rate = float(dropout_keep(shape, p, seed, offset).mean())
        assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / N) ** 0.5, (p, seed, offset, rate)
    assert dropout_keep((1, 3, 5, 8), 0.0, 5, 0).all()


def test_dropout_reference_counter_carries():
    """offset + g carries into the counter's high word, and the mask of a view depends on offset + g alone."""
    a = dropout_keep((1, 1, 64, 4), 0.5, 77, 2 ** 32 - 37)
    b = dropout_keep((1, 1, 27, 4), 0.5, 77, 2 ** 32)
    assert np.array_equal(a[:, :, 37:], b) and not np.array_equal(a[:, :, :27], b)


def test_bound_holds_for_torch_fp32():
    """torch's fp32 resize (the same fp32 coordinate arithmetic as the kernel's) against the float64 reference: err / bound <= 1 on every
    size the model issues, forward and backward."""
    g = torch.Generator().manual_seed(2)
    worst = {"fwd": 0.0, "bwd": 0.0}
    for n_in, n_out, _ in MODEL_RESIZES + MODEL_LOGITS:
        x = torch.randn(2, 4, n_in, n_in, generator=g).requires_grad_(True)
        y = F.interpolate(x, size=(n_out, n_out), mode="bilinear", align_corners=True)
        m = resize_mats(n_in, n_out)
        xd = x.detach().permute(0, 2, 3, 1).double()
        ref = resize_fwd(xd, m[0], m[0])
        bound = resize_bound(xd.abs(), m, m, 8, resize_fwd) + 2.0 ** -126
        r = float(((y.detach().permute(0, 2, 3, 1).double() - ref).abs() / bound).max())
        dy = torch.randn(y.shape, generator=g)
        (dx,) = torch.autograd.grad(y, x, dy)
        dyd = dy.permute(0, 2, 3, 1).double()
        ref = resize_bwd(dyd, m[0], m[0])
        bound = resize_bound(dyd.abs(), m, m, bwd_chain(m, m), resize_bwd) + 2.0 ** -126
        rb = float(((dx.permute(0, 2, 3, 1).double() - ref).abs() / bound).max())
        print(f"{n_in} -> {n_out}: torch fp32 err / bound forward {r:.3g}, backward {rb:.3g}")
        assert r <= 1.0 and rb <= 1.0, (n_in, n_out, r, rb)
        worst["fwd"], worst["bwd"] = max(worst["fwd"], r), max(worst["bwd"], rb)
    assert min(worst.values()) > 0.05, worst         # (the bound is not vacuous either)


# ================================================================================================ data, views, checks
def wide_desc(shape, dtype, wide=None, lo=None):
    """The channel slice [lo, lo + c) of a buffer ``wide`` channels wide (default: the second half of a 2c-wide one)."""
    n, h, w, c = shape
    wide = 2 * c if wide is None else wide
    lo = c if lo is None else lo
    return ((n, h, w, c), (h * w * wide, w * wide, wide, 1), lo, dtype)


def dense_desc(shape, dtype):
    return wide_desc(shape, dtype, shape[3], 0)


def int_fill(g, lo, hi):
    return lambda span, dtype: ints(g, (span,), lo, hi, dtype)


def gauss_fill(g):
    return lambda span, dtype: torch.randn(span, generator=g, device=DEV).to(dtype)


def out_buf(desc):
    return Buf(desc, nan_fill)


def bounded(buf, ref, bound, what, family):
    """|view - ref| <= bound (+ 2^-8 |ref| for a bf16 store); the rest of the buffer keeps its bits.  -> err / bound."""
    dtype = buf.desc[3]
    b = bound + (UB * ref.abs() if dtype == BF16 else 0) + 2.0 ** -126
    err = (buf.t.double() - ref).abs()
    ratio = float((err / b).max())
    print(f"{what}: err / bound {ratio:.3g} (max err {float(err.max()):.3g})")
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3g} (max err {float(err.max()):.3g})"
    Stats.note(family, ratio)
    print(f"largest err / bound so far, {family}: {Stats.worst[family]:.3g}")
    exp = buf.before.clone()
    exp.as_strided(*buf.desc[:3]).copy_(buf.t)
    same_bits(buf.base, exp, f"{what}: bytes outside the view")
    return ratio


def exact(buf, ref, what):
    compare(buf, ref, None, 0, what, "exact", True)


def dyadic(ref, what):
    """The premise of the exact cases: every reference value is a multiple of 2^-8 below 2^16 (24 bits hold it and every partial sum)."""
    s = ref * 256.0
    assert bool((s == s.round()).all()) and float(ref.abs().max()) < 2.0 ** 16, f"{what}: the exact-data premise does not hold"


COVERED = set()


def covers(*key):
    COVERED.add(key)


def fl32(v):
    return float(np.float32(v))


# ================================================================================================ 2. bilinear: exact cases
EXACT_ROWS = [   # (h_in, w_in, h_out, w_out, B, C)
    (65, 33, 129, 129, 2, 64),        # scales 0.5, 0.25: the gather kernel (sh is not < 0.5)
    (33, 33, 129, 129, 3, 8),         # 0.25, 0.25: the split kernel, ragged last block
    (129, 97, 65, 129, 2, 64),        # 2, 0.75: down-sampling
    (97, 65, 65, 65, 2, 128),         # 1.5, 1: an identity axis
    (97, 65, 1, 129, 2, 8),           # 0, 0.5: the scale <= 0 branch of `range`
    (1, 5, 7, 9, 2, 8),               # 0, 0.5: a single input row
]
SCALAR_FORMS = [(F32, 2, 4, 2), (BF16, 4, 8, 4), (BF16, 8, 16, 2)]      # (dtype, C, buffer width, first channel): off the 16-byte width
THRESHOLD_C = {F32: 4, BF16: 8}          # 257^2 <-> 1025^2 with one vector group per pixel (the split kernel's threshold, below)


def bil_views(row, dtype, C=None, wide=None, lo=None):
    hi, wi, ho, wo, B, c = row
    c = C or c
    return wide_desc((B, hi, wi, c), dtype, wide, lo), wide_desc((B, ho, wo, c), dtype, wide, lo)


def bil_mats(small, big):
    return resize_mats(small[0][1], big[0][1], DEV), resize_mats(small[0][2], big[0][2], DEV)


def bil_exact_case(K, g, small, big, what):
    """Forward small -> big, backward big -> small and the accumulating backward on an integer pre-fill, bit for bit."""
    mh, mw = bil_mats(small, big)
    x = Buf(small, int_fill(g, -60, 100))
    y = out_buf(big)
    K.bilinear_fwd(x.t, y.t)
    ref = resize_fwd(x.t.double(), mh[0], mw[0])
    dyadic(ref, what)
    exact(y, ref, f"{what} forward")
    x.check_untouched(f"{what} forward input")
    dy = Buf(big, int_fill(g, -100, 60))
    ref = resize_bwd(dy.t.double(), mh[0], mw[0])
    dyadic(ref, what)
    dx = out_buf(small)
    K.bilinear_bwd(dy.t, dx.t)
    exact(dx, ref, f"{what} backward")
    acc = Buf(small, int_fill(g, -100, 100))
    K.bilinear_bwd(dy.t, acc.t, accumulate=True)
    exact(acc, ref + acc.before.as_strided(*acc.desc[:3]).double(), f"{what} backward, accumulating")
    dy.check_untouched(f"{what} backward input")


for _dt in DTYPES:
    for _r in EXACT_ROWS:
        covers("bilinear_fwd", _dt, _r[5], _r[0:2], _r[2:4])
        covers("bilinear_fwd_batched", _dt, _r[5], _r[0:2], _r[2:4])
        for _a in (False, True):
            covers("bilinear_bwd", _dt, _r[5], _r[0:2], _r[2:4], _a)
for _dt, _c, _, _ in SCALAR_FORMS:
    for _r in EXACT_ROWS[:2]:
        covers("bilinear_fwd", _dt, _c, _r[0:2], _r[2:4])
        covers("bilinear_fwd_batched", _dt, _c, _r[0:2], _r[2:4])
        for _a in (False, True):
            covers("bilinear_bwd", _dt, _c, _r[0:2], _r[2:4], _a)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("row", EXACT_ROWS, ids=_id)
def test_bilinear_exact(K, dtype, row):
    small, big = bil_views(row, dtype)
    bil_exact_case(K, gen(100 + EXACT_ROWS.index(row)), small, big, f"bilinear {_id(row)} {_id(dtype)}")


@gpu
@pytest.mark.parametrize("form", SCALAR_FORMS, ids=_id)
@pytest.mark.parametrize("row", EXACT_ROWS[:2], ids=_id)
def test_bilinear_exact_scalar_forms(K, form, row):
    """Views off the 16-byte width: the one-element-per-thread forward and gather kernels."""
    dtype, C, wide, lo = form
    small, big = bil_views(row, dtype, C, wide, lo)
    bil_exact_case(K, gen(120 + EXACT_ROWS.index(row)), small, big, f"bilinear scalar form {_id(row)} C {C} {_id(dtype)} [{lo}:{lo + C}] of {wide}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bilinear_exact_batched_forward(K, dtype):
    """All exact cases of one dtype in one dct_bilinear_fwd_batched call, destinations in the second half of 2C-wide buffers."""
    g = gen(140)
    xs, ys, refs = [], [], []
    rows = EXACT_ROWS + [(257, 257, 1025, 1025, 3, THRESHOLD_C[dtype])]
    for row in rows:
        hi, wi, ho, wo, B, C = row
        xs.append(Buf(dense_desc((B, hi, wi, C), dtype), int_fill(g, -60, 100)))
        ys.append(out_buf(wide_desc((B, ho, wo, C), dtype)))
        refs.append(resize_fwd(xs[-1].t.double(), resize_mats(hi, ho, DEV)[0], resize_mats(wi, wo, DEV)[0]))
    K.bilinear_fwd_batched([x.t for x in xs], [y.t for y in ys])
    for row, y, ref in zip(rows, ys, refs):
        dyadic(ref, "batched forward")
        exact(y, ref, f"batched forward {_id(row)} {_id(dtype)}")


@gpu
def test_bilinear_exact_batched_forward_scalar_forms(K):
    """The batched call on views off the vector width (hip_ops falls back to one launch per tensor)."""
    g = gen(141)
    for dtype, C, wide, lo in SCALAR_FORMS:
        xs, ys, refs = [], [], []
        for row in EXACT_ROWS[:2]:
            small, big = bil_views(row, dtype, C, wide, lo)
            xs.append(Buf(small, int_fill(g, -60, 100)))
            ys.append(out_buf(big))
            mh, mw = bil_mats(small, big)
            refs.append(resize_fwd(xs[-1].t.double(), mh[0], mw[0]))
        K.bilinear_fwd_batched([x.t for x in xs], [y.t for y in ys])
        for row, y, ref in zip(EXACT_ROWS, ys, refs):
            exact(y, ref, f"batched forward, scalar form {_id(row)} C {C} {_id(dtype)}")


THRESHOLD = [(F32, 4, 3), (F32, 4, 4), (BF16, 8, 3), (BF16, 8, 4)]       # 257^2 source pixels x B: 198,147 / 264,196 groups around 262,144
for _dt, _c, _ in THRESHOLD:
    covers("bilinear_fwd", _dt, _c, (257, 257), (1025, 1025))
    covers("bilinear_fwd_batched", _dt, _c, (257, 257), (1025, 1025))
    for _a in (False, True):
        covers("bilinear_bwd", _dt, _c, (257, 257), (1025, 1025), _a)


@gpu
@pytest.mark.parametrize("dtype,C,B", THRESHOLD, ids=_id)
def test_bilinear_exact_around_the_split_threshold(K, dtype, C, B):
    """257^2 <- 1025^2 (scales 0.25) with one vector group per pixel: B = 3 runs the eight-lane split kernel, B = 4 the gather kernel
    (and the forward pass at that size beside them)."""
    assert (B * 257 * 257 < 262144) == (B == 3)
    g = gen(150 + B)
    mh = resize_mats(257, 1025, DEV)
    x = ints(g, (B, 257, 257, C), -60, 100, dtype)
    y = out_buf(dense_desc((B, 1025, 1025, C), dtype))
    K.bilinear_fwd(x, y.t)
    ref = resize_fwd(x.double(), mh[0], mh[0])
    dyadic(ref, "threshold")
    exact(y, ref, f"forward 257 -> 1025, B {B}, {_id(dtype)}")
    del y, ref
    dy = ints(g, (B, 1025, 1025, C), -100, 60, dtype)
    ref = resize_bwd(dy.double(), mh[0], mh[0])
    dyadic(ref, "threshold")
    dx = out_buf(dense_desc((B, 257, 257, C), dtype))
    K.bilinear_bwd(dy, dx.t)
    exact(dx, ref, f"backward 1025 -> 257, B {B}, {_id(dtype)}")
    acc = Buf(dense_desc((B, 257, 257, C), dtype), int_fill(g, -100, 100))
    K.bilinear_bwd(dy, acc.t, accumulate=True)
    exact(acc, ref + acc.before.view(B, 257, 257, C).double(), f"accumulating backward 1025 -> 257, B {B}, {_id(dtype)}")


# ================================================================================================ 3. bilinear: the model's geometry
for _i, _o, _c in MODEL_RESIZES:
    for _dt in DTYPES:
        covers("bilinear_fwd", _dt, _c, (_i, _i), (_o, _o))
        covers("bilinear_fwd_batched", _dt, _c, (_i, _i), (_o, _o))
        covers("bilinear_bwd", _dt, _c, (_i, _i), (_o, _o), False)
for _i, _o, _c in MODEL_LOGITS:
    covers("bilinear_fwd", F32, _c, (_i, _i), (_o, _o))
    covers("bilinear_bwd", F32, _c, (_i, _i), (_o, _o), False)


def bil_model_case(K, g, dtype, n_in, n_out, C, sliced, what):
    m = resize_mats(n_in, n_out, DEV)
    x = Buf(dense_desc((2, n_in, n_in, C), dtype), gauss_fill(g))
    y = out_buf(wide_desc((2, n_out, n_out, C), dtype) if sliced else dense_desc((2, n_out, n_out, C), dtype))
    K.bilinear_fwd(x.t, y.t)
    xd = x.t.double()
    bounded(y, resize_fwd(xd, m[0], m[0]), resize_bound(xd.abs(), m, m, 8, resize_fwd), f"{what} forward", "bilinear forward")
    dy = Buf(desc_of(y.t), gauss_fill(g))
    dx = out_buf(x.desc)
    K.bilinear_bwd(dy.t, dx.t)
    dyd = dy.t.double()
    bounded(dx, resize_bwd(dyd, m[0], m[0]), resize_bound(dyd.abs(), m, m, bwd_chain(m, m), resize_bwd), f"{what} backward",
            "bilinear backward")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("n_in,n_out,C", MODEL_RESIZES, ids=_id)
def test_bilinear_model_skips(K, dtype, n_in, n_out, C):
    """A skip connection's resize (into the second half of the concatenation) and its backward on Gaussian data, within the bound."""
    bil_model_case(K, gen(200 + n_in), dtype, n_in, n_out, C, True, f"skip {n_in} -> {n_out} C {C} {_id(dtype)}")


@gpu
@pytest.mark.parametrize("n_in,n_out,C", MODEL_LOGITS, ids=_id)
def test_bilinear_model_logits(K, n_in, n_out, C):
    """The classifier's logits (fp32, dense): C = 4 takes the vector forward and the split backward, C = 2 the scalar forms."""
    bil_model_case(K, gen(220 + n_in + C), F32, n_in, n_out, C, False, f"logits {n_in} -> {n_out} C {C}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("rows", [MODEL_RESIZES[:4], MODEL_RESIZES[4:]], ids=["256", "200"])
def test_bilinear_model_batched_forward(K, dtype, rows):
    """The four skip resizes of one forward pass in one launch, deepest level first as the model issues them."""
    g = gen(240)
    xs, ys = [], []
    for n_in, n_out, C in reversed(rows):
        xs.append(Buf(dense_desc((2, n_in, n_in, C), dtype), gauss_fill(g)))
        ys.append(out_buf(wide_desc((2, n_out, n_out, C), dtype)))
    K.bilinear_fwd_batched([x.t for x in xs], [y.t for y in ys])
    for (n_in, n_out, C), x, y in zip(reversed(rows), xs, ys):
        m = resize_mats(n_in, n_out, DEV)
        xd = x.t.double()
        bounded(y, resize_fwd(xd, m[0], m[0]), resize_bound(xd.abs(), m, m, 8, resize_fwd),
                f"batched skip {n_in} -> {n_out} C {C} {_id(dtype)}", "bilinear forward")


# ================================================================================================ 4. pooling and un-pooling
POOL_SIZES = [(2, 252, 252, 64), (2, 122, 122, 128), (2, 57, 57, 256), (2, 25, 25, 512), (2, 23, 25, 8), (2, 1, 7, 8)]
for _s in POOL_SIZES:
    for _dt in DTYPES:
        for _codes in (False, True):
            covers("maxpool_fwd", _dt, _s[3], _s[1:3], _codes)
        for _m, _sc in FLAGS:
            for _via in ("x", "codes"):
                covers("maxpool_bwd", _dt, _s[3], _s[1:3], None, _m, fl32(_sc), _via)


def pooled_shape(shape):
    return (shape[0], cdiv(shape[1], 2), cdiv(shape[2], 2), shape[3])


def pool_descs(shape, dtype):
    """Dense at the model's sizes; the small shapes sit in the second half of a 16-wide buffer."""
    mk = wide_desc if shape[3] == 8 else dense_desc
    return mk(shape, dtype), mk(pooled_shape(shape), dtype)


def pool_case(K, g, x, what):
    """Forward with and without codes, backward from x and from the codes under every flag, against pool_ref / unpool_ref: every bit."""
    dtype, shape = x.desc[3], x.desc[0]
    _, pd = pool_descs(shape, dtype)
    m, codes = pool_ref(x.t.double())
    y = out_buf(pd)
    K.maxpool_fwd(x.t, y.t)
    y.check_out(m.to(dtype), f"{what}: pooled values")
    y = out_buf(pd)
    got = torch.full(pd[0], 0xA5, dtype=torch.uint8, device=DEV)
    K.maxpool_fwd(x.t, y.t, codes=got)
    y.check_out(m.to(dtype), f"{what}: pooled values beside the codes")
    same_bits(got, codes, f"{what}: codes")
    dy = Buf(pd, gauss_fill(g))
    for mask, scale in FLAGS:
        want = unpool_ref(codes, dy.t.float(), shape, mask, scale).to(dtype)
        dx = out_buf(x.desc)
        K.maxpool_bwd(x.t, dy.t, dx.t, relu_mask=mask, scale=scale)
        dx.check_out(want, f"{what}: un-pooling from x, mask {mask} scale {scale}")
        dx = out_buf(x.desc)
        K.maxpool_bwd(None, dy.t, dx.t, relu_mask=mask, scale=scale, codes=codes)
        dx.check_out(want, f"{what}: un-pooling from codes, mask {mask} scale {scale}")
    x.check_untouched(f"{what}: input")
    return m, codes


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("zeros", [False, True], ids=["ties", "ties+zeros"])
@pytest.mark.parametrize("shape", POOL_SIZES, ids=_id)
def test_pool_and_unpool_on_ties(K, dtype, zeros, shape):
    """Integers in [0, 3] (most windows hold ties), without and with a ReLU-like half of zeros: the first maximum in scan order wins."""
    g = gen(300 + shape[1])
    x = Buf(pool_descs(shape, dtype)[0], int_fill(g, 0, 3))
    if zeros:
        x.base.mul_((torch.rand(x.base.shape, generator=g, device=DEV) < 0.5).to(dtype))
        x.before = x.base.clone()
    m, codes = pool_case(K, g, x, f"pool {_id(shape)} {_id(dtype)} zeros {zeros}")
    if shape[1] > 1:
        assert float(((codes & 3) != 0).double().mean()) > 0.2 and int((codes & 8).sum()) == 0


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_pool_special_windows(K, dtype):
    """Windows of all NaN, all -inf, one NaN among numbers, -0.0 against +0.0 (both orders) and negative numbers: the documented semantics."""
    nan, inf = float("nan"), float("inf")
    wins = [[nan, nan, nan, nan], [-inf, -inf, -inf, -inf], [1.0, nan, 3.0, 2.0], [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0],
            [-3.0, -1.0, -1.0, -2.0]]
    x = torch.empty(1, 4, 6, 8, dtype=torch.float64)
    for i, wv in enumerate(wins):
        for c in range(8):
            rot = wv[c % 4:] + wv[:c % 4]                                 # the window's contents move round with the channel
            x[0, 2 * (i // 3):2 * (i // 3) + 2, 2 * (i % 3):2 * (i % 3) + 2, c] = torch.tensor(rot, dtype=torch.float64).reshape(2, 2)
    xb = Buf(pool_descs((1, 4, 6, 8), dtype)[0], nan_fill)
    xb.t.copy_(x.to(dtype))
    xb.before = xb.base.clone()
    m, codes = pool_case(K, gen(350), xb, f"special windows {_id(dtype)}")
    m, codes = m.cpu(), codes.cpu()
    assert bool((codes[0, 0, 0] == 8).all()) and bool((codes[0, 0, 1] == 8).all())          # nothing routed: un-pooling checked in pool_case
    assert bool((m[0, 0, 0] == -inf).all()) and bool((m[0, 0, 1] == -inf).all())
    assert bool(((codes[0, 1, 0] & 12) == 0).all()) and bool(((codes[0, 1, 1] & 12) == 0).all())      # zeros of either sign: bit 2 clear
    assert bool((m[0, 1, 0] == 0).all()) and bool(((codes[0, 1, 0] & 3) == 0).all())                    # ... and the first one wins
    assert codes[0, 0, 2].tolist() == [4 | 2, 4 | 1, 4 | 0, 4 | 3, 4 | 2, 4 | 1, 4 | 0, 4 | 3] and bool((m[0, 0, 2] == 3.0).all())
    assert bool((m[0, 1, 2] == -1.0).all()) and bool(((codes[0, 1, 2] & 12) == 0).all())
    got = torch.full((1, 4, 6, 8), float("nan"), dtype=dtype, device=DEV)
    dy = torch.ones(1, 2, 3, 8, dtype=dtype, device=DEV)
    K.maxpool_bwd(xb.t, dy, got, relu_mask=False)
    assert float(got[0, 0:2, 0:4].float().abs().sum()) == 0.0                                           # nothing routed from x either


# ---- un-pooling with the skip connection's gather
SKIP_EXACT = [((129, 65), (129, 129)), ((130, 66), (129, 129)), ((129, 65), (33, 17)), ((130, 66), (33, 17))]      # x (pooled 65 x 33), skip; C = 64
SKIP_MODEL = [(252, 88, 64), (122, 48, 128), (57, 28, 256), (25, 18, 512), (196, 24, 64), (94, 16, 128), (43, 12, 256), (18, 10, 512)]
SKIP_MODEL_FLAGS = [(True, 1.0), (True, 2.0)]            # what the model passes: the un-dropout scale at level 4, 1 elsewhere
for _dt in DTYPES:
    for _x, _s in SKIP_EXACT:
        for _m, _sc in FLAGS:
            covers("maxpool_bwd", _dt, 64, _x, _s, _m, fl32(_sc), "codes")
    for _x, _s, _c in SKIP_MODEL:
        for _m, _sc in SKIP_MODEL_FLAGS:
            covers("maxpool_bwd", _dt, _c, (_x, _x), (_s, _s), _m, fl32(_sc), "codes")


def tie_codes(g, shape):
    """Routing codes of tie-rich data with a ReLU-like share of zeros, from the reference."""
    x = ints(g, shape, 0, 3, F32) * (torch.rand(shape, generator=g, device=DEV) < 0.6)
    return pool_ref(x.double())[1].contiguous()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("xs,ss", SKIP_EXACT, ids=_id)
def test_unpool_with_skip_gather_exact(K, dtype, xs, ss):
    """dx = unpool(dy + Wh^T skip Ww) at dyadic scales (0.5 / 0.25 up, 2 / 2 down) on integers far above 2^8 -- dy multiples of 8 up to
    800, skip up to 100 x 8 per weight unit, so the gather and the sum need more than bf16's eight bits: an extra bf16 rounding of either
    addend shows.  Every bit, under every flag."""
    g = gen(400 + xs[0] + ss[0])
    B, C = 2, 64
    shape = (B, xs[0], xs[1], C)
    ps = pooled_shape(shape)
    assert ps[1:3] == (65, 33)
    codes = tie_codes(g, shape)
    dy = Buf(dense_desc(ps, dtype), int_fill(g, -60, 100))
    dy.base.mul_(8)
    dy.before = dy.base.clone()
    skip = Buf(wide_desc((B, ss[0], ss[1], C), dtype), int_fill(g, -60, 100))
    skip.base.mul_(8)
    skip.before = skip.base.clone()
    mh, mw = resize_mats(65, ss[0], DEV), resize_mats(33, ss[1], DEV)
    gather = resize_bwd(skip.t.double(), mh[0], mw[0])
    dyadic(gather / 64.0, "skip gather")
    assert float(gather.abs().max()) > 3 * 2.0 ** 8 and float(dy.t.double().abs().max()) > 3 * 2.0 ** 8
    total = (dy.t.double() + gather).float()
    assert bool((total.double() == dy.t.double() + gather).all())
    for mask, scale in FLAGS:
        dx = out_buf(dense_desc(shape, dtype))
        K.maxpool_bwd(None, dy.t, dx.t, relu_mask=mask, scale=scale, codes=codes, skip=skip.t)
        dx.check_out(unpool_ref(codes, total, shape, mask, scale).to(dtype), f"skip gather {xs} <- {ss} {_id(dtype)} mask {mask} scale {scale}")
    dy.check_untouched("dy")
    skip.check_untouched("skip")


def skip_bounded_case(K, g, dtype, shape, s, flags, what, skip_desc=None, dy_desc=None, dx_desc=None, in_memory=False):
    """Gaussian dy and skip: dx against unpool_ref(codes, dy + Wh^T skip Ww) within the backward bound of the gather + 2 U |sum|
    (+ one bf16 half-ulp of the sum where it is formed in memory), routed as the values are."""
    ps = pooled_shape(shape)
    C = shape[3]
    codes = tie_codes(g, shape)
    dy = Buf(dy_desc or dense_desc(ps, dtype), gauss_fill(g))
    skip = Buf(skip_desc or wide_desc((shape[0], s, s, C), dtype), gauss_fill(g))
    mh, mw = resize_mats(ps[1], s, DEV), resize_mats(ps[2], s, DEV)
    sd = skip.t.double()
    total = dy.t.double() + resize_bwd(sd, mh[0], mw[0])
    tb = resize_bound(sd.abs(), mh, mw, bwd_chain(mh, mw), resize_bwd) + 2 * U * total.abs()
    if in_memory and dtype == BF16:
        tb = tb + UB * total.abs()
    for mask, scale in flags:
        dx = out_buf(dx_desc or dense_desc(shape, dtype))
        K.maxpool_bwd(None, dy.t, dx.t, relu_mask=mask, scale=scale, codes=codes, skip=skip.t)
        bounded(dx, unpool_ref(codes, total, shape, mask, scale), unpool_ref(codes, tb, shape, mask, scale),
                f"{what} mask {mask} scale {scale}", "skip gather")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("x,s,C", SKIP_MODEL, ids=_id)
def test_unpool_with_skip_gather_model_sizes(K, dtype, x, s, C):
    skip_bounded_case(K, gen(450 + x), dtype, (2, x, x, C), s, SKIP_MODEL_FLAGS, f"skip gather {x} <- {s} C {C} {_id(dtype)}")


SKIP_FALLBACK = [(BF16, 4, 8, 4), (BF16, 8, 16, 2), (F32, 2, 4, 2)]        # (dtype, C, buffer width, first channel): off the vector width
for _dt, _c, _, _ in SKIP_FALLBACK:
    covers("maxpool_bwd", _dt, _c, (25, 23), (18, 18), True, 2.0, "codes")


@gpu
@pytest.mark.parametrize("dtype,C,wide,lo", SKIP_FALLBACK, ids=_id)
def test_unpool_with_skip_gather_off_the_vector_width(K, dtype, C, wide, lo):
    """Views the 16-byte kernel cannot take: hip_ops runs the scalar bilinear backward into a buffer, adds dy there and un-pools with the
    one-element-per-thread form.  The same reference; the sum is rounded to the storage type in memory (bf16: one more half-ulp)."""
    shape = (2, 25, 23, C)
    ps = pooled_shape(shape)
    skip_bounded_case(K, gen(470 + C), dtype, shape, 18, [(True, 2.0)], f"skip gather fall-back C {C} {_id(dtype)} [{lo}:{lo + C}] of {wide}",
                      skip_desc=wide_desc((2, 18, 18, C), dtype, wide, lo), dy_desc=wide_desc(ps, dtype, wide, lo),
                      dx_desc=wide_desc(shape, dtype, wide, lo), in_memory=True)


# ================================================================================================ 5. dropout
SEED = 0x9E3779B97F4A7C15
DROP_SITES = [((2, 25, 25, 512), None), ((2, 9, 9, 1024), None), ((1, 5, 5, 1024), None), ((1, 3, 5, 8), 16)]      # (shape, buffer width or dense)
DROP_P = [0.5, 0.3, 0.0]
DROP_OFFSETS = [0, 2 ** 32 - 37, 7 << 40]
DROP_POOL_SITES = [(2, 25, 23, 512), (1, 25, 25, 512), (1, 18, 18, 512)]
for _dt in DTYPES:
    for _s, _ in DROP_SITES:
        for _p in DROP_P:
            for _form in ("host", "dev"):
                for _mask in (False, True):
                    covers("dropout_fwd", _dt, _s[3], _s[1:3], fl32(_p), _form, _mask)
            covers("dropout_apply", _dt, _s[3], _s[1:3], fl32(_p))
    for _s in DROP_POOL_SITES:
        for _p in (0.5, 0.3):
            covers("dropout_maxpool_fwd", _dt, _s[3], _s[1:3], fl32(_p))


def drop_descs(shape, wide, dtype):
    return wide_desc(shape, dtype, wide, wide - shape[3]) if wide else dense_desc(shape, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape,wide", DROP_SITES, ids=_id)
def test_dropout_stream_host_offset(K, dtype, shape, wide):
    """Mask and values of dct_dropout_fwd against the numpy Philox reference for offsets 0, 2^32 - 37 (offset + g carries into the counter's
    high word) and 7 << 40, p = 0.5 / 0.3 / 0; dct_dropout_apply with that mask gives the same bits."""
    g = gen(500 + shape[1])
    x = Buf(drop_descs(shape, wide, dtype), gauss_fill(g))
    for p in DROP_P:
        for offset in DROP_OFFSETS:
            mref, yref = dropout_ref(x.t, p, SEED, offset)
            y = out_buf(x.desc)
            mask = torch.full(shape, 0xA5, dtype=torch.uint8, device=DEV)
            K.dropout_fwd(x.t, y.t, p, SEED, offset, mask_out=mask)
            same_bits(mask, mref, f"dropout mask {_id(shape)} p {p} offset {offset}")
            y.check_out(yref, f"dropout values {_id(shape)} {_id(dtype)} p {p} offset {offset}")
            y = out_buf(x.desc)
            K.dropout_fwd(x.t, y.t, p, SEED, offset)
            y.check_out(yref, f"dropout values without mask_out {_id(shape)} {_id(dtype)} p {p} offset {offset}")
        y = out_buf(x.desc)
        K.dropout_apply(x.t, y.t, mref, p)
        y.check_out(yref, f"dropout_apply {_id(shape)} {_id(dtype)} p {p}")
        if p > 0:
            assert 0 < int(mref.sum()) < mref.numel()
    x.check_untouched("dropout input")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape,wide", DROP_SITES, ids=_id)
def test_dropout_stream_device_counter(K, dtype, shape, wide):
    """The device-counter form from counters 0 and 41: the launch that reads word ``parity`` = n draws offset (n + 1) << 40 and leaves n + 1
    in the other word -- both parities in turn, with and without mask_out."""
    g = gen(520 + shape[1])
    x = Buf(drop_descs(shape, wide, dtype), gauss_fill(g))
    for p in DROP_P:
        for start in (0, 41):
            for first in (0, 1):
                state = torch.tensor([start, start], dtype=torch.int64, device=DEV)
                n = start
                for k, parity in enumerate((first, first ^ 1)):
                    mref, yref = dropout_ref(x.t, p, SEED, (n + 1) << 40)
                    y = out_buf(x.desc)
                    mask = torch.full(shape, 0xA5, dtype=torch.uint8, device=DEV) if k == 0 else None
                    K.dropout_fwd(x.t, y.t, p, SEED, 12345, mask_out=mask, calls_dev=state, parity=parity)
                    what = f"device-counter dropout {_id(shape)} {_id(dtype)} p {p} from {start}, launch {k}, parity {parity}"
                    y.check_out(yref, what)
                    if mask is not None:
                        same_bits(mask, mref, what + ": mask")
                    n += 1
                    want = [start, start]
                    want[parity ^ 1] = n
                    if k == 1:
                        want[parity] = n - 1
                    assert state.tolist() == want, (what, state.tolist(), want)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", DROP_POOL_SITES, ids=_id)
def test_dropout_and_pool_against_the_reference(K, dtype, shape):
    """dct_dropout_maxpool2x2_fwd_codes: pooled values and codes equal pool_ref(dropout_ref(x)) -- the reference, not the two launches --
    on ReLU'd Gaussian data (dropped and clamped zeros tie), from counters 0 and 41, both parities; the counter words afterwards."""
    g = gen(540 + shape[2])
    x = torch.randn(shape, generator=g, device=DEV).clamp_min(0).to(dtype)
    ps = pooled_shape(shape)
    for p in (0.5, 0.3):
        for start, parity in ((0, 0), (41, 1)):
            state = torch.tensor([start, start], dtype=torch.int64, device=DEV)
            _, dropped = dropout_ref(x, p, SEED, (start + 1) << 40)
            m, cref = pool_ref(dropped.double())
            y = out_buf(dense_desc(ps, dtype))
            codes = torch.full(ps, 0xA5, dtype=torch.uint8, device=DEV)
            K.dropout_maxpool_fwd(x, y.t, codes, p, SEED, state, parity)
            what = f"dropout + pool {_id(shape)} {_id(dtype)} p {p} from {start}"
            y.check_out(m.to(dtype), what + ": pooled values")
            same_bits(codes, cref, what + ": codes")
            want = [start, start]
            want[parity ^ 1] = start + 1
            assert state.tolist() == want
            assert float(m.max()) > 0 and bool(((cref & 4) == 0).any())


# ================================================================================================ 6. relu_bwd, cast, repack
RELU_SITES = [((2, 57, 57, 256), None), ((1, 3, 5, 8), 16)]
RELU_SCALES = [1.0, 2.0, S07]
for _dt in DTYPES:
    for _s, _ in RELU_SITES:
        for _sc in RELU_SCALES:
            covers("relu_bwd", _dt, _s[3], _s[1:3], fl32(_sc))


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape,wide", RELU_SITES, ids=_id)
def test_relu_bwd_gates_and_rounds_once(K, dtype, shape, wide):
    """y = a > 0 ? fl32(g scale) : 0, rounded once: the gate on +-0, the smallest normal, a negative tiny value, NaN and +-inf mixed into
    Gaussian data; scales 1, 2 and fl32(1 / 0.7)."""
    gg = gen(600 + shape[1])
    desc = drop_descs(shape, wide, dtype)
    a = Buf(desc, gauss_fill(gg))
    tiny = float(torch.finfo(dtype).tiny)
    special = torch.tensor([0.0, -0.0, tiny, -tiny, float("nan"), float("inf"), -float("inf")], dtype=dtype, device=DEV)
    pick = torch.randint(0, 3 * len(special), a.base.shape, generator=gg, device=DEV)
    a.base.copy_(torch.where(pick < len(special), special[pick.clamp_max(len(special) - 1)], a.base))
    a.before = a.base.clone()
    gr = Buf(desc, gauss_fill(gg))
    gate = a.t.float() > 0
    for v, want in zip(special.tolist(), [False, False, True, False, False, True, False]):
        af = a.t.float()
        sel = torch.isnan(af) if v != v else (af == v) & (torch.signbit(af) == (str(v)[0] == "-"))
        assert bool(sel.any()) or shape[1] < 8, v            # (the large site holds every special value)
        assert bool((gate[sel] == want).all()), v
    for scale in RELU_SCALES:
        y = out_buf(desc)
        K.relu_bwd(gr.t, a.t, y.t, scale=scale)
        prod = (gr.t.double() * float(scale)).float()
        y.check_out(torch.where(gate, prod, torch.zeros_like(prod)).to(dtype), f"relu_bwd {_id(shape)} {_id(dtype)} scale {scale}")
    a.check_untouched("a")
    gr.check_untouched("g")


CAST_PAIRS = [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16), (F32, F16), (F16, F32), (F16, F16)]
CAST_SHAPE = (2, 31, 33, 5)
for _a, _b in CAST_PAIRS:
    covers("cast", _a, _b, CAST_SHAPE[3], CAST_SHAPE[1:3])


def cast_specials(src):
    """fp32 values whose rounding to bf16 / f16 is decided by a tie, by the largest finite value or by the subnormal range; rounded to
    ``src`` first where that is narrower (they stay interesting: infinities, zeros, subnormals, the largest finite value)."""
    v = []
    for k in (8, 11):                        # ties of an 8-bit (bf16) and an 11-bit (f16) significand: to even, both ways, and just off the tie
        h = 2.0 ** -k
        v += [1 + h, 1 + 3 * h, 1 + h + 2.0 ** -23, 1 + h - 2.0 ** -23, 1 + 3 * h - 2.0 ** -23, -(1 + h), -(1 + 3 * h), 1 + 5 * h, 2 - h]
    bmax, hmax = 3.3895313892515355e38, 65504.0
    v += [bmax, bmax * (1 + 2.0 ** -9), bmax * (1 + 2.0 ** -10), 3.4028234663852886e38, -bmax * (1 + 2.0 ** -9), -3.4028234663852886e38]
    v += [hmax, 65519.996, 65520.0, 65536.0, -65520.0, 1e5, -1e5]
    v += [float("inf"), -float("inf"), 0.0, -0.0, float("nan")]
    v += [2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -149, -2.0 ** -140, 1e-40]                   # fp32 / bf16 subnormals
    v += [2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), -2.0 ** -24, 6e-8, 3e-6]   # f16 subnormals
    return torch.tensor(v, dtype=torch.float32).to(src)


@gpu
@pytest.mark.parametrize("src,dst", CAST_PAIRS, ids=_id)
def test_cast_rounds_as_torch(K, src, dst):
    """All seven dtype pairs on strided views: bit-equal to torch's CPU conversion on Gaussian data, rounding ties, values just above the
    largest finite bf16 / f16, +-inf, +-0 and subnormals; a NaN gives a NaN (any payload)."""
    g = gen(650)
    sd = wide_desc(CAST_SHAPE, src, 8, 1)
    x = Buf(sd, lambda span, dt: (torch.randn(span, generator=g, device=DEV) * 3).to(dt))
    sp = cast_specials(src).to(DEV)
    pick = torch.randint(0, 4 * len(sp), x.base.shape, generator=g, device=DEV)
    x.base.copy_(torch.where(pick < len(sp), sp[pick.clamp_max(len(sp) - 1)], x.base))
    x.before = x.base.clone()
    y = out_buf(wide_desc(CAST_SHAPE, dst, 8, 2))
    K.cast(x.t, y.t)
    want = x.t.cpu().to(dst).to(DEV)
    nans = torch.isnan(x.t)
    assert bool(nans.any()) and bool(torch.isnan(y.t[nans]).all()), "a NaN must stay a NaN"
    y.t[nans] = want[nans]
    y.check_out(want, f"cast {_id(src)} -> {_id(dst)}")
    x.check_untouched("cast input")
    if src == F32 and dst != F32:
        assert bool(torch.isinf(want[~torch.isinf(x.t)]).any()), "the overflow cases are in the data"


# the UNet's transposed packs: every 3x3 convolution but the stem as [Cout, 9, Cin] -> data-gradient layout (mode 1, taps flipped), the four
# up-convolutions as [Cin, 4, Cout] -> forward layout (mode 2)
UNET_CONVS = [(64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (512, 256), (512, 512), (1024, 512), (1024, 1024), (512, 1024), (512, 512),
              (256, 512), (256, 256), (128, 256), (128, 128), (64, 128), (64, 64)]
UNET_UPCONVS = [(1024, 512), (512, 256), (256, 128), (128, 64)]
UNET_PACKS = [(co, 9, ci, 1, True) for co, ci in UNET_CONVS] + [(ci, 4, co, 2, False) for ci, co in UNET_UPCONVS]
PACK_TABLES = [("bf16 -> bf16, 64-edge", BF16, BF16, UNET_PACKS, 64), ("fp32 -> fp32, 32-edge", F32, F32, UNET_PACKS, 32),
               ("fp32 and bf16 -> bf16, 32-edge", None, BF16, UNET_PACKS[:6] + [(96, 9, 64, 1, True), (64, 4, 32, 2, False)] + UNET_PACKS[17:], 32)]
for _, _s, _d, _jobs, _edge in PACK_TABLES:
    covers("pack_weights_batched", _d, _edge)
    for _i, _j in enumerate(_jobs):
        covers("pack_jobs_table", _s or (F32 if _i % 2 else BF16), _d, *_j, _edge)
PACK_SINGLE = [(128, 9, 64), (64, 9, 128), (256, 4, 128), (1024, 9, 1024), (1024, 4, 512), (96, 9, 40), (1, 1, 1000003)]
for _d in DTYPES:
    covers("pack_weight", _d, 0, False)
    for _p, _t, _q in PACK_SINGLE:
        for _tr in (1, 2):
            for _f in (False, True):
                covers("pack_weight", _d, _tr, _f, _p, _t, _q)


def pack_want(src, mode, flip):
    t = src.flip(1) if flip else src
    return (t.permute(2, 1, 0) if mode == 1 else t.permute(1, 2, 0)).contiguous().flatten()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("P,T,Q", PACK_SINGLE, ids=_id)
def test_pack_weight(K, dtype, P, T, Q):
    """dct_pack_weight: the plain conversion (transpose 0) and both transposed layouts, with and without the tap flip, on integer data in
    [-128, 127]: a torch permute, bit for bit; P, Q multiples of 32 take the tiled kernel, the others the element-wise one."""
    g = gen(700 + P)
    src = ints(g, (P, T, Q), -128, 127, F32)
    n = P * T * Q
    for transpose in (0, 1, 2):
        for flip in ((False,) if transpose == 0 else (False, True)):
            dst = out_buf(((n,), (1,), 8, dtype))
            K.pack_weight(src, dst.t, P, T, Q, transpose=transpose, flip_taps=flip)
            want = src.flatten() if transpose == 0 else pack_want(src, transpose, flip)
            dst.check_out(want.to(dtype), f"pack_weight {P} x {T} x {Q} transpose {transpose} flip {flip} {_id(dtype)}")


@gpu
@pytest.mark.parametrize("name,sdt,ddt,jobs,edge", PACK_TABLES, ids=[t[0].replace(" ", "") for t in PACK_TABLES])
def test_pack_weights_batched(K, name, sdt, ddt, jobs, edge):
    """Every transposed pack of a UNet in ONE table and launch: destinations lie 64 elements apart in one pre-filled buffer, which must
    equal the torch permutes with the gaps untouched."""
    g = gen(720)
    GAP = 64
    total = sum(P * T * Q + GAP for P, T, Q, _, _ in jobs) + GAP
    dst = torch.full((total,), -7.0, dtype=ddt, device=DEV)
    want = dst.clone()
    table, off = [], GAP
    for i, (P, T, Q, mode, flip) in enumerate(jobs):
        src = ints(g, (P, T, Q), -128, 127, sdt or (F32 if i % 2 else BF16))
        n = P * T * Q
        table.append((src, dst[off:off + n], P, T, Q, mode, flip))
        want[off:off + n] = pack_want(src, mode, flip).to(ddt)
        off += n + GAP
    tab, njobs, tiles, got_edge = K.pack_jobs_table(table, torch.device(DEV))
    assert got_edge == edge and njobs == len(jobs)
    K.pack_weights_batched(tab, njobs, tiles, ddt, got_edge)
    torch.cuda.synchronize()
    same_bits(dst, want, f"batched packs, {name}")


# ================================================================================================ 7. the model issues nothing else
REC_FNS = ("maxpool_fwd", "maxpool_bwd", "bilinear_fwd", "bilinear_fwd_batched", "bilinear_bwd", "dropout_fwd", "dropout_maxpool_fwd",
           "dropout_apply", "relu_bwd", "cast", "pack_weight", "pack_jobs_table", "pack_weights_batched")
MODEL_CONFIGS = [(256, 4, BF16, False), (200, 2, BF16, True), (256, 4, F32, True)]        # (H, classes, compute dtype, d/dx); B = 1, dropout 0.5


def _hw(t):
    return (int(t.shape[1]), int(t.shape[2]))


def call_keys(name, b, result):
    """The (function, dtype, C, spatial sizes, flags) keys of one recorded call (bound arguments ``b``)."""
    if name == "maxpool_fwd":
        return [(name, b["x"].dtype, b["x"].shape[3], _hw(b["x"]), b["codes"] is not None)]
    if name == "maxpool_bwd":
        return [(name, b["dy"].dtype, b["dy"].shape[3], _hw(b["dx"]), None if b["skip"] is None else _hw(b["skip"]), bool(b["relu_mask"]),
                 fl32(b["scale"]), "x" if b["codes"] is None else "codes")]
    if name == "bilinear_fwd":
        return [(name, b["x"].dtype, b["x"].shape[3], _hw(b["x"]), _hw(b["y"]))]
    if name == "bilinear_fwd_batched":
        return [(name, x.dtype, x.shape[3], _hw(x), _hw(y)) for x, y in zip(b["xs"], b["ys"])]
    if name == "bilinear_bwd":
        return [(name, b["dy"].dtype, b["dy"].shape[3], _hw(b["dx"]), _hw(b["dy"]), bool(b["accumulate"]))]
    if name == "dropout_fwd":
        return [(name, b["x"].dtype, b["x"].shape[3], _hw(b["x"]), fl32(b["p"]), "host" if b["calls_dev"] is None else "dev", b["mask_out"] is not None)]
    if name in ("dropout_maxpool_fwd", "dropout_apply"):
        return [(name, b["x"].dtype, b["x"].shape[3], _hw(b["x"]), fl32(b["p"]))]
    if name == "relu_bwd":
        return [(name, b["g"].dtype, b["g"].shape[3], _hw(b["g"]), fl32(b["scale"]))]
    if name == "cast":
        return [(name, b["x"].dtype, b["y"].dtype, b["x"].shape[3], _hw(b["x"]))]
    if name == "pack_weight":
        tr = int(b["transpose"])
        return [(name, b["dst"].dtype, tr, bool(b["flip_taps"])) + ((b["P"], b["T"], b["Q"]) if tr else ())]
    if name == "pack_jobs_table":
        return [(name, s.dtype, d.dtype, P, T, Q, mode, bool(flip), result[3]) for s, d, P, T, Q, mode, flip in b["jobs"]]
    assert name == "pack_weights_batched", name
    return [(name, b["dtype"], b["edge"])]


def record_model(K, H, classes, dtype, need_dx):
    from dct_amd.arch import get_arch
    torch.manual_seed(5)
    net = get_arch("unet", {"num_classes": classes, "compute_dtype": dtype, "dropout_p": 0.5}).to(DEV).train()
    keys, depth = [], [0]
    orig = {f: getattr(K, f) for f in REC_FNS}

    def wrap(name):
        sig = inspect.signature(orig[name])

        def fn(*a, **kw):
            top = depth[0] == 0
            depth[0] += 1
            try:
                out = orig[name](*a, **kw)
            finally:
                depth[0] -= 1
            if top:
                b = sig.bind(*a, **kw)
                b.apply_defaults()
                keys.extend(call_keys(name, b.arguments, out))
            return out
        return fn
    for f in REC_FNS:
        setattr(K, f, wrap(f))
    try:
        x = torch.rand(1, 1, H, H, generator=gen(1), device=DEV).requires_grad_(need_dx)
        out = net(x)
        out.backward(torch.randn(out.shape, generator=gen(2), device=DEV))
    finally:
        for f in REC_FNS:
            setattr(K, f, orig[f])
    torch.cuda.synchronize()
    return keys


@gpu
def test_model_geometry_is_covered(K):
    """One eager training forward + backward of get_arch("unet") per configuration with the pointwise functions of hip_ops wrapped: every
    recorded (function, dtype, C, spatial sizes, flags) is one that the tests above replay."""
    for H, classes, dtype, need_dx in MODEL_CONFIGS:
        keys = record_model(K, H, classes, dtype, need_dx)
        names = sorted({k[0] for k in keys})
        print(f"{H}^2 {_id(dtype)}: {len(keys)} recorded pointwise calls / jobs of {names}")
        missing = sorted({k for k in keys if k not in COVERED}, key=repr)
        assert not missing, f"{H}^2 {_id(dtype)}: the model issues what no table above covers: {missing}"
        for must in ("bilinear_fwd", "bilinear_bwd", "maxpool_bwd", "dropout_fwd", "pack_jobs_table"):
            assert must in names, (must, names)
