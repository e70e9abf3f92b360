"""The UNet convolution kernels at training scale, against float64 references: the implicit-GEMM convolutions of csrc/igemm.hip
(``K.conv2d``: per-tap igemm / igemm2 with split-K, shared-halo igemm3m, packed-rows igemm3p with channel-slice splits, their fused
epilogues), the weight gradients of csrc/wgrad.hip (``K.conv2d_wgrad``: wgrad, wgrad2, wgrad3 and their pixel chunks) and the small
UNet-only kernels (``K.conv_cin1_fwd/dgrad/wgrad``, ``K.head_fwd/head_bwd``, ``K.bias_grad``, ``K.bias_grad_batched``).

References are computed in float64 on the device, as one shifted-view GEMM per filter tap on NHWC tensors (`conv_ref`, `wgrad_ref`;
`test_reference_helpers_match_conv2d` checks them against F.conv2d on the CPU).

Exact-integer data (the main tool).  Activations, gradients and weights are small integers, which bf16 and fp32 hold exactly, and the
biases are fp32 integers.  The ranges keep the sum of |terms| of every output below 2^24 (asserted per case by `assert_exact_range`),
so every partial sum -- in any order, split, chunk or fold -- is an integer below 2^24 and fp32 accumulation is exact.  The data have
non-zero means, so the partial sums of a K-step chain, a split-K slab or a pixel chunk are mostly far above 2^11: a slab or accumulator
that is rounded to bf16 / fp16 anywhere changes them.  The kernel then equals the float64 reference BIT FOR BIT -- exactly for fp32
outputs, after one round-to-nearest-even for bf16 outputs -- and a lost, duplicated or misplaced pixel, tap, channel slice, split or
chunk fails at any scale.  Places where production rounds an intermediate to bf16 on purpose, and the reference rounds it the same way:
  * the fused stem weight gradient (``stem=``) reads the masked data gradient of its 64 -> 64 convolution after the bf16 rounding;
  * max-pooling with codes (``pool_out`` / ``pool_codes``) pools the bf16-rounded convolution output.
Outputs are pre-filled with NaN, or with known integers where the kernel accumulates; the bytes of a view's buffer outside the view
must stay as they were.

Gaussian data, as in training (`test_gaussian_recorded`).  With U = 2^-24 and |x| (*) |w| the float64 reference on absolute values,
an output of a chain of n fp32 additions is off by at most  n U (|x| (*) |w|)  (first order; the MFMA's internal sums are counted as
one addition per product).  n is what the PLANNED kernel runs: the products of one split (conv: K / splits) or of one pixel chunk
(weight gradient: pixels per chunk x 1 product each), plus the fold over the splits or chunks (+ 2 for the bias and the accumulate
adds).  A bf16 store adds half a bf16 ulp, at most 2^-8 |ref|.  The largest measured err / bound is printed per family.

Every conv-family call of one eager forward and backward of get_arch("unet") is recorded (views, strides and keyword flags) for
cfg2 (256^2, C = 4, B = 8, bf16, dropout 0.5), cfg4u (200^2, C = 2, B = 8, bf16, with d/dx) and the fp32 parity mode (256^2, B = 2,
with d/dx), and replayed on fresh data of the same geometry (`test_recorded_call`).  Planner edges beyond the model's shapes
(`test_*_plan_edges`) assert through dct_debug_last_plan that the intended kernel and split / chunk count ran; the Python mirrors of
the planners (`igemm_plan`, `packed_plan`, `wgrad_plan`) predict them.  The 32-bit addressing guards (`test_*_guard`: lean x_bytes, igemm3m's x32 and
y16, wgrad's fits32 / M and wgrad3's row offset) run one case just below and one just above a guard with data only in the first and
last image (or row band)."""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
UB = 2.0 ** -8
EXACT = 2.0 ** 24

# dct_tune_set knobs (include/dct.h) and their shipped values
IGEMM_SPLIT, WGRAD_CHUNKS, IGEMM_HALO, WGRAD_ROWS, IGEMM_PACKED = 1, 3, 7, 8, 10
WGRAD_TARGET, WGRAD3_TARGET, IGEMM_XCD, LEAN = 14, 15, 39, 38
DEFAULTS = {IGEMM_SPLIT: -1, WGRAD_CHUNKS: -1, IGEMM_HALO: 1, WGRAD_ROWS: 1, IGEMM_PACKED: 1, WGRAD_TARGET: 256, WGRAD3_TARGET: 768,
            IGEMM_XCD: 1, LEAN: 31}


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


def plan_note():
    from dct_amd import _lib
    f = _lib.load().dct_debug_last_plan
    f.restype = ctypes.c_char_p
    return f().decode()


# ================================================================================================ references (float64, any device)
def conv_ref(x, w, R, S, stride=1, dil=1, pad_h=0, pad_w=0, Ho=None, Wo=None):
    """x [n, H, W, Cin], w [N, R, S, Cin] -> [n, Ho, Wo, N] = sum over taps of x[shifted] @ w[:, r, s].T, in x's dtype."""
    n, H, W, _ = x.shape
    if Ho is None:
        Ho = (H + 2 * pad_h - dil * (R - 1) - 1) // stride + 1
        Wo = (W + 2 * pad_w - dil * (S - 1) - 1) // stride + 1
    xp = F.pad(x, (0, 0, pad_w, pad_w, pad_h, pad_h))
    out = torch.zeros(n, Ho, Wo, w.shape[0], dtype=x.dtype, device=x.device)
    for r in range(R):
        for s in range(S):
            v = xp[:, r * dil: r * dil + (Ho - 1) * stride + 1: stride, s * dil: s * dil + (Wo - 1) * stride + 1: stride, :]
            out += v @ w[:, r, s, :].T
    return out


def wgrad_ref(p, q, R, S, stride=1, dil=1, pad_h=0, pad_w=0):
    """dw[pc, r, s, qc] = sum over pixels m of p[m, pc] q[m shifted by the tap, qc] (p = dy at the output, q = x at the input)."""
    n, Ho, Wo, Cp = p.shape
    qp = F.pad(q, (0, 0, pad_w, pad_w, pad_h, pad_h))
    pf = p.reshape(-1, Cp)
    dw = torch.empty(Cp, R, S, q.shape[3], dtype=p.dtype, device=p.device)
    for r in range(R):
        for s in range(S):
            v = qp[:, r * dil: r * dil + (Ho - 1) * stride + 1: stride, s * dil: s * dil + (Wo - 1) * stride + 1: stride, :]
            dw[:, r, s, :] = pf.T @ v.reshape(-1, q.shape[3])
    return dw


def test_reference_helpers_match_conv2d():
    """The tap-GEMM references against F.conv2d (and its weight gradient by autograd) in float64 on the CPU: padding, stride,
    dilation, non-square filters."""
    g = torch.Generator().manual_seed(0)
    for (n, H, W, Ci, Co, R, S, st, dil, ph, pw) in [(2, 9, 11, 5, 7, 3, 3, 1, 1, 0, 0), (1, 10, 8, 3, 4, 3, 3, 1, 1, 2, 2),
                                                     (2, 12, 10, 4, 6, 2, 2, 2, 1, 0, 0), (1, 13, 13, 3, 2, 3, 3, 1, 2, 2, 1),
                                                     (1, 7, 9, 2, 3, 1, 1, 1, 1, 0, 0), (2, 11, 9, 3, 5, 3, 2, 2, 1, 1, 0)]:
        x = torch.randn(n, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, R, S, generator=g, dtype=torch.float64)
        y = F.conv2d(x, w, stride=st, dilation=dil, padding=(ph, pw))
        got = conv_ref(x.detach().permute(0, 2, 3, 1), w.permute(0, 2, 3, 1), R, S, st, dil, ph, pw)
        assert torch.allclose(got.permute(0, 3, 1, 2), y, rtol=1e-12, atol=1e-12)
        dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        wr = w.clone().requires_grad_(True)
        F.conv2d(x.detach(), wr, stride=st, dilation=dil, padding=(ph, pw)).backward(dy)
        dw = wgrad_ref(dy.permute(0, 2, 3, 1), x.detach().permute(0, 2, 3, 1), R, S, st, dil, ph, pw)
        assert torch.allclose(dw.permute(0, 3, 1, 2), wr.grad, rtol=1e-12, atol=1e-12)


# ================================================================================================ planner mirrors (csrc/igemm.hip, wgrad.hip)
def cdiv(a, b):
    return -(-a // b)


def igemm_plan(dtype, Cin, N, M, R, S, split=-1):
    """make_plan -> (v2, bm, bn, tiles, splits, kiters_per_split)."""
    v2 = dtype == torch.bfloat16 and Cin % 64 == 0
    if v2:
        bk, (bn, bm) = 64, ((128, 128) if N % 128 == 0 else (64, 256))
    else:
        bk, bn, bm = (32 if dtype == torch.bfloat16 else 16), (128 if N % 128 == 0 else 64), 128
    kiters = R * S * Cin // bk
    tiles = cdiv(M, bm) * (N // bn)
    splits = 1
    if v2:
        if tiles < 96 and kiters >= 4:
            splits = min((450 + tiles // 2) // tiles, 8)
            while splits > 1 and kiters // splits < 4:
                splits -= 1
    elif tiles < 384:
        splits = min(cdiv(768, tiles), 16)
        while splits > 1 and kiters // splits < 4:
            splits -= 1
    if split >= 1:
        splits = split
    splits = min(splits, kiters)
    kps = cdiv(kiters, splits)
    return v2, bm, bn, tiles, cdiv(kiters, kps), kps


def packed_plan(n, Ho, Wo, Cin, N):
    """make_plan_p (3x3 stride-1 bf16 with the packed kernel on) -> (PR, tiles_per_img, splits, cps) or None."""
    if Cin % 64 or N % 128 or Wo > 126:
        return None
    PR = min(128 // Wo, 192 // (Wo + 2) - 2, Ho)
    if PR < 1:
        return None
    tiles = cdiv(Ho, PR)
    if Ho * Wo / (tiles * 128.0) < 0.5:
        return None
    nch = Cin // 64
    blocks0 = n * tiles * (N // 128)
    splits = 1
    if blocks0 < 160:
        splits = min((160 + 48 + blocks0 - 1) // blocks0, nch)
        while splits > 1 and nch // splits < 4:
            splits -= 1
    if nch // splits < 4 or blocks0 * splits < 160:
        return None
    cps = cdiv(nch, splits)
    return PR, tiles, cdiv(nch, cps), cps


def wgrad_plan(dtype, p_shape, q_shape, R, S, stride=1, dil=1, pad=0, chunks_knob=-1, rows=1, target=256, target3=768, lean=31):
    """make_wplan for dense p / q -> dict(kind, chunks, ppc | spc, nseg, pitch)."""
    n, Hp, Wp, Cp = p_shape
    _, Hq, Wq, Cq = q_shape
    M = n * Hp * Wp
    fits32 = n * Hp * Wp * Cp < 2 ** 30 and n * Hq * Wq * Cq < 2 ** 30
    v2 = dtype == torch.bfloat16 and M < 2 ** 24 and fits32
    bkp = 64 if v2 else (32 if dtype == torch.bfloat16 else 16)
    bp, bq = (128 if Cp % 128 == 0 else 64), (128 if Cq % 128 == 0 else 64)
    tiles = (Cp // bp) * (Cq // bq) * R * S
    if v2:
        chunks = min((target + tiles // 2) // tiles, 64, cdiv(M, 4 * bkp))
    else:
        chunks = min(cdiv(1536, tiles), cdiv(M, 8 * bkp))
    per_chunk = Cp * Cq * R * S * 4
    while chunks > 1 and chunks * per_chunk > (192 << 20):
        chunks -= 1
    if chunks_knob >= 1:
        chunks = chunks_knob
    chunks = max(chunks, 1)
    ppc = cdiv(cdiv(M, chunks), bkp) * bkp
    out = dict(kind="wgrad2" if v2 else "wgrad", chunks=cdiv(M, ppc), ppc=ppc, tiles=tiles)
    if v2 and rows and R == 3 and S == 3 and stride == 1 and dil == 1:
        skips = (lean & 17) == 17 and pad == 0
        if Wp > 64:
            segs, pitch, nr = cdiv(Wp, 64), 0, 1
            units = Hp * segs
            tail = Wp - 64 * (segs - 1)
            fill = Wp / (16.0 * (4 * (segs - 1) + cdiv(tail, 16))) if skips else Wp / (segs * 64.0)
        else:
            segs, pitch = 1, Wp + 2
            nr = max(66 // pitch, 1)
            steps = cdiv(Hp, nr)
            fill = Hp * Wp / (steps * 64.0)
            units = steps
        if fill >= 0.70 and Hp * Wp * Cp < 2 ** 29 and Hq * Wq * Cq < 2 ** 29:
            nseg = n * units
            tiles3 = (Cp // 64) * (Cq // 64) * 3
            ch = min((target3 // 2 + tiles3 // 2) // tiles3, 256, nseg // 8)
            while ch > 1 and ch * per_chunk > (192 << 20):
                ch -= 1
            if chunks_knob >= 1:
                ch = chunks_knob
            ch = max(ch, 1)
            spc = cdiv(nseg, ch)
            out = dict(kind="wgrad3", chunks=cdiv(nseg, spc), spc=spc, nseg=nseg, pitch=pitch, segs=segs, tiles=tiles3)
    out["direct"] = out["kind"] != "wgrad" and out["chunks"] == 1
    return out


def wgrid(chunks, tiles):
    return (cdiv(chunks, 8) * 8 if chunks >= 8 else chunks) * tiles


# ================================================================================================ data and checks
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def ints(g, shape, lo, hi, dtype):
    """Integers uniform in [lo, hi], exact in ``dtype``."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g, device=DEV, dtype=torch.int32).to(dtype)


def bits_of(t):
    """ReLU-gate bits of a dense NHWC tensor as the kernels lay them out: byte (pixel, c // 8), bit c % 8."""
    pos = (t > 0).to(torch.int32)
    n, h, w, c = pos.shape
    return (pos.view(n, h, w, c // 8, 8) << torch.arange(8, device=pos.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


def pool_ref(y):
    """2x2 ceil-mode max pooling of y [n, H, W, C] with the codes of csrc/pointwise.hip maxpool_fwd_codes_kernel: the window position
    (scan order 0..3) of the FIRST maximum (strictly greater replaces), bit 2 set when the maximum is > 0."""
    n, H, W, C = y.shape
    Hp, Wp = cdiv(H, 2), cdiv(W, 2)
    yp = F.pad(y, (0, 0, 0, 2 * Wp - W, 0, 2 * Hp - H), value=float("-inf"))
    m = torch.full((n, Hp, Wp, C), float("-inf"), dtype=y.dtype, device=y.device)
    arg = torch.full((n, Hp, Wp, C), 8, dtype=torch.uint8, device=y.device)
    for k in range(4):
        v = yp[:, k >> 1::2, k & 1::2, :]
        gt = v > m
        m = torch.where(gt, v, m)
        arg = torch.where(gt, torch.full_like(arg, k), arg)
    return m, arg | ((m > 0).to(torch.uint8) << 2)


def same_bits(got, want, what):
    """Bitwise equality (NaN patterns included) of two tensors of one dtype."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    iv = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    a, b = got.contiguous().view(iv), want.contiguous().view(iv)
    bad = a != b
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} differ; first at {idx}: got {got.reshape(-1)[i].item()!r} "
                             f"want {want.reshape(-1)[i].item()!r}")


def assert_exact_range(abs_ref, what):
    m = float(abs_ref.max()) if abs_ref.numel() else 0.0
    assert m < EXACT, f"{what}: sum |terms| reaches {m:.3g}: the exact-integer premise does not hold"


class Buf(object):
    """A tensor view with the recorded shape / strides on a fresh buffer of its own (the view's offset kept modulo 64 elements, so
    its alignment is the recorded one); the bytes of the buffer outside the view are checked unchanged by `check_out`."""

    def __init__(self, desc, fill):
        shape, stride, off, dtype = desc
        off %= 64
        span = off + 1 + sum((a - 1) * b for a, b in zip(shape, stride)) if all(shape) else off
        self.base = fill(span, dtype)
        self.t = self.base.as_strided(shape, stride, off)
        self.before = self.base.clone()
        self.desc = (shape, stride, off, dtype)

    def check_out(self, want, what):
        """The view equals ``want`` bit for bit and the rest of the buffer is as it was."""
        shape, stride, off, dtype = self.desc
        exp = self.before.clone()
        exp.as_strided(shape, stride, off).copy_(want)
        same_bits(self.base, exp, what)

    def check_untouched(self, what):
        same_bits(self.base, self.before, what)


def nan_fill(span, dtype):
    if dtype in (torch.float32, torch.bfloat16, torch.float64):
        return torch.full((span,), float("nan"), dtype=dtype, device=DEV)
    return torch.full((span,), 0xA5, dtype=dtype, device=DEV)


def desc_of(t):
    return (tuple(t.shape), tuple(t.stride()), t.storage_offset(), t.dtype)


# ================================================================================================ recording the model's calls
CONV_FNS = ("conv2d", "conv2d_wgrad", "bias_grad", "bias_grad_batched", "conv_cin1_fwd", "conv_cin1_dgrad", "conv_cin1_wgrad",
            "head_fwd", "head_bwd")
CONFIGS = {   # name -> (H, C, B, dtype, dropout, need_dx)
    "cfg2": (256, 4, 8, torch.bfloat16, 0.5, False),
    "cfg4u": (200, 2, 8, torch.bfloat16, 0.5, True),
    "fp32": (256, 4, 2, torch.float32, 0.5, True),
}
# calls per configuration: forward 1 stem + 21 conv2d + 1 head; backward 1 head + 21 weight gradients + 21 data gradients (the stem's
# weight gradient rides in the last one where it can: cfg2) + the four up-convolutions' bias gradients in one batched call; fp32 takes
# the bias gradients of the 17 3x3 convolutions as calls of their own; with d/dx the stem's weight and data gradients are calls too
COUNTS = {"cfg2": 67, "cfg4u": 69, "fp32": 86}


def _desc(v):
    if isinstance(v, torch.Tensor):
        return ("T", desc_of(v))
    if isinstance(v, (list, tuple)):
        return type(v)(_desc(e) for e in v)
    return v


_RECORDED = {}


def recorded(K, cfg):
    """The conv-family calls of one eager training forward + backward of get_arch("unet") for ``cfg``: (fn, args, kwargs) with every
    tensor replaced by ("T", (shape, stride, offset, dtype))."""
    if cfg in _RECORDED:
        return _RECORDED[cfg]
    from dct_amd.arch import get_arch
    H, C, B, dt, p, need_dx = CONFIGS[cfg]
    torch.manual_seed(5)
    net = get_arch("unet", {"num_classes": C, "compute_dtype": dt, "dropout_p": p}).to(DEV).train()
    calls, depth = [], [0]
    orig = {f: getattr(K, f) for f in CONV_FNS}

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
    for f in CONV_FNS:
        setattr(K, f, wrap(f))
    try:
        x = torch.rand(B, 1, H, H, generator=gen(1), device=DEV).requires_grad_(need_dx)
        out = net(x)
        out.backward(torch.randn(out.shape, generator=gen(2), device=DEV))
    finally:
        for f in CONV_FNS:
            setattr(K, f, orig[f])
    torch.cuda.synchronize()
    del net
    _RECORDED[cfg] = calls
    return calls


# ================================================================================================ replay of one call
class Data(object):
    """Value ranges of one replay: exact integers (mode "int") or Gaussian (mode "gauss")."""

    def __init__(self, mode, seed):
        self.mode, self.g = mode, gen(seed)

    def act(self, shape, dtype):          # activations: non-negative integers (mean 1.5) / |N(0, 1)|
        if self.mode == "int":
            return ints(self.g, shape, 0, 3, dtype)
        return torch.randn(tuple(shape), generator=self.g, device=DEV).abs().to(dtype)

    def grad(self, shape, dtype):         # gradients and weights: integers in [-1, 2] (mean 0.5) / N(0, 1)
        if self.mode == "int":
            return ints(self.g, shape, -1, 2, dtype)
        return torch.randn(tuple(shape), generator=self.g, device=DEV).to(dtype)

    def sparse(self, shape, dtype, p):    # integers in {-1, 0, 1}, non-zero with probability p
        v = ints(self.g, shape, -1, 1, dtype)
        keep = torch.rand(tuple(shape), generator=self.g, device=DEV) < p
        return torch.where(keep, v, torch.zeros_like(v))


def stem_patches(shape):
    """[n, H, W, 1] indicator of 6 x 6 pixel patches on a 32-pixel grid (every third cell) and of the bottom-right 6 x 6 corner: the
    dense data inside give data gradients of several hundred (beyond bf16's exact integers, so its rounding shows) and stem partials
    far above 2^11, while the sums over all pixels stay below 2^24."""
    n, H, W, _ = shape
    i = torch.arange(H, device=DEV).view(H, 1)
    j = torch.arange(W, device=DEV).view(1, W)
    m = ((i % 32 < 6) & (j % 32 < 6) & ((i // 32 + j // 32) % 3 == 0)) | ((i >= H - 6) & (j >= W - 6))
    return m.view(1, H, W, 1).expand(n, H, W, 1)


def filled(fn):
    """fill(span, dtype) for Buf from a value generator fn(shape, dtype)."""
    return lambda span, dtype: fn((span,), dtype)


class Stats(object):
    worst = {}

    @classmethod
    def note(cls, family, ratio):
        cls.worst[family] = max(cls.worst.get(family, 0.0), ratio)


def compare(buf, ref, absref, n_chain, what, family, exact):
    """Exact: the view equals ref rounded once to its dtype.  Gaussian: |got - ref| <= n U absref (+ half a bf16 ulp)."""
    dtype = buf.desc[3]
    if exact:
        buf.check_out(ref.to(torch.float32).to(dtype), what)
        return
    got = buf.t.double()
    bound = n_chain * U * absref + 2 * U * ref.abs() + (UB * ref.abs() if dtype == torch.bfloat16 else 0) + 2.0 ** -126
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3g} (max err {float(err.max()):.3g})"
    Stats.note(family, ratio)
    exp = buf.before.clone()
    exp.as_strided(*buf.desc[:3]).copy_(buf.t)
    same_bits(buf.base, exp, f"{what}: bytes outside the view")


def replay(K, call, mode, seed, what):
    name, a, kw = call
    fn = globals()["_replay_" + name]
    fn(K, Data(mode, seed), a, dict(kw), what)


def _T(d):
    assert isinstance(d, tuple) and d[0] == "T", d
    return d[1]


def _replay_conv2d(K, D, a, kw, what):
    xd, wd, bd, yd = a
    exact = D.mode == "int"
    stem_call = kw.get("stem") is not None
    dtype = _T(xd)[3]
    n, Hi, Wi, Cin = _T(xd)[0]
    _, Hy, Wy, cout = _T(yd)[0]
    R, S, stride, dil = kw.get("R", 3), kw.get("S", 3), kw.get("stride", 1), kw.get("dil", 1)
    ph, pw = kw.get("pad_h", 0), kw.get("pad_w", 0)
    scatter = kw.get("scatter2x2", False)
    N = 4 * cout if scatter else cout
    Ho, Wo = (Hy // 2, Wy // 2) if scatter else (Hy, Wy)
    if stem_call:      # the stem's gradient sums run over all the output pixels: dense data in patches keep them below 2^24
        x = Buf(_T(xd), filled(D.act))
        x.t.mul_(stem_patches(x.t.shape).to(dtype))
        wb = Buf(_T(wd), filled(D.grad))
    else:
        x = Buf(_T(xd), filled(D.act))
        wb = Buf(_T(wd), filled(D.grad) if exact else filled(lambda s, t: (D.grad(s, torch.float32) / math.sqrt(R * S * Cin)).to(t)))
    assert wb.t.is_contiguous() and wb.t.numel() == N * R * S * Cin, (what, wb.desc)
    w = wb.t.reshape(N, R, S, Cin)
    bias = None
    if bd is not None:
        bias = Buf(_T(bd), filled(lambda s, t: ints(D.g, s, -64, 64, t)) if exact else filled(lambda s, t: torch.randn(s, generator=D.g, device=DEV)))
    acc = kw.get("accumulate", False)
    y = Buf(_T(yd), filled(lambda s, t: ints(D.g, s, -4, 4, t)) if acc else nan_fill)
    mask = mbits = None
    if kw.get("mask") is not None:
        mask = Buf(_T(kw["mask"]), filled(lambda s, t: ints(D.g, s, -1, 2, t)))
        kw["mask"] = mask.t
    if kw.get("mask_bits") is not None:
        mbits = bits_of(mask.t)
        kw["mask_bits"] = mbits
    rbits = None
    if kw.get("relu_bits_out") is not None:
        rbits = Buf(_T(kw["relu_bits_out"]), nan_fill)
        kw["relu_bits_out"] = rbits.t
    pool = codes = None
    if kw.get("pool_out") is not None:
        pool = Buf(_T(kw["pool_out"]), nan_fill)
        kw["pool_out"] = pool.t
        if kw.get("pool_codes") is not None:
            codes = Buf(_T(kw["pool_codes"]), nan_fill)
            kw["pool_codes"] = codes.t
    stem = None
    if stem_call:
        sx_d, sdw_d, sdb_d, sacc = kw["stem"]
        sx = Buf(_T(sx_d), filled(lambda s, t: ints(D.g, s, 0, 1, t)))
        sdw = Buf(_T(sdw_d), filled(lambda s, t: ints(D.g, s, -8, 8, t)) if sacc else nan_fill)
        sdb = Buf(_T(sdb_d), filled(lambda s, t: ints(D.g, s, -8, 8, t)) if sacc else nan_fill)
        stem = (sx, sdw, sdb, sacc)
        kw["stem"] = (sx.t, sdw.t, sdb.t, sacc)
    K.conv2d(x.t, wb.t, bias.t if bias is not None else None, y.t, **kw)
    note = plan_note()
    torch.cuda.synchronize()
    what = f"{what} [{note}]"
    # float64 reference of the whole epilogue
    x64, w64 = x.t.double(), w.double()
    raw = conv_ref(x64, w64, R, S, stride, dil, ph, pw, Ho, Wo)
    absr = conv_ref(x64.abs(), w64.abs(), R, S, stride, dil, ph, pw, Ho, Wo)
    if exact:
        assert_exact_range(absr.max().reshape(1) + (bias.t.abs().max() if bias is not None else 0) + (4 if acc else 0), what)
    if scatter:   # column ab * cout + co of pixel (oy, ox) -> (2 oy + a, 2 ox + b, co)
        raw = raw.view(n, Ho, Wo, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, Hy, Wy, cout)
        absr = absr.view(n, Ho, Wo, 2, 2, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, Hy, Wy, cout)
    v = raw + (bias.t.double() if bias is not None else 0)
    if kw.get("relu"):
        v = v.clamp_min(0)
    if mask is not None:
        mc = kw.get("mask_channels", 0) or cout
        mk = mask.t[..., :mc].double() > 0
        v = v.clone()
        v[..., :mc] = torch.where(mk, v[..., :mc] * kw.get("mask_scale", 1.0), torch.zeros_like(v[..., :mc]))
        absr = absr * max(1.0, kw.get("mask_scale", 1.0))
    if acc:
        v = v + y.before.as_strided(*y.desc[:3]).double()
    if stem is not None:
        sx, sdw, sdb, sacc = stem
        da = v.to(torch.float32).to(dtype).double()          # the masked data gradient, rounded to bf16 as the epilogue rounds it
        xs = sx.t.double().reshape(n, Hy + 2, Wy + 2, 1)
        dw = wgrad_ref(da, xs, 3, 3).reshape(cout, 9)
        db = da.sum((0, 1, 2))
        assert_exact_range(wgrad_ref(da.abs(), xs, 3, 3).reshape(-1) + 8, what + ": stem")
        assert float(da.abs().max()) > 512, f"{what}: the stem's data gradient stays within bf16's exact integers"
        assert not torch.equal(da, v), f"{what}: no bf16 rounding of the stem's data gradient happens"
        assert note.startswith("igemm3m") and "stem weight gradient" in note, note
        if sacc:
            dw = dw + sdw.before.as_strided(*sdw.desc[:3]).double().reshape(cout, 9)
            db = db + sdb.before.as_strided(*sdb.desc[:3]).double()
        sdw.check_out(dw.reshape(sdw.desc[0]).float(), what + ": stem dw")
        sdb.check_out(db.reshape(sdb.desc[0]).float(), what + ": stem db")
        y.check_untouched(what + ": y (not written under stem=)")
        return
    if not exact:
        # the longest fp32 chain of the planned kernel: the products of one split (per-tap or channel-slice split), + the fold
        splits = igemm_plan(dtype, Cin, N, n * Ho * Wo, R, S)[4]
        pp = packed_plan(n, Ho, Wo, Cin, N) if (dtype == torch.bfloat16 and R == S == 3 and stride == dil == 1 and not scatter) else None
        if pp is not None:
            splits = min(splits, pp[2])
        n_chain = R * S * Cin / splits + max(splits, pp[2] if pp else 1) + 2
        compare(y, v, absr, n_chain, what, "conv2d", False)
        return
    yq = v.to(torch.float32).to(dtype)
    if kw.get("pool_only") and "y not stored" in note:
        y.check_untouched(what + ": y (pool_only: not stored)")
    else:
        y.check_out(yq, what + ": y")
    if rbits is not None:
        rbits.check_out(bits_of(yq), what + ": relu bits")
    if pool is not None:
        pm, pc = pool_ref(yq.float())
        pool.check_out(pm.to(dtype), what + ": pooled")
        if codes is not None:
            codes.check_out(pc, what + ": pool codes")


def _replay_conv2d_wgrad(K, D, a, kw, what):
    pd, qd, dwd = a
    exact = D.mode == "int"
    p = Buf(_T(pd), filled(D.grad))
    q = Buf(_T(qd), filled(D.act))
    R, S, stride, dil = kw.get("R", 3), kw.get("S", 3), kw.get("stride", 1), kw.get("dil", 1)
    ph, pw = kw.get("pad_h", 0), kw.get("pad_w", 0)
    acc = kw.get("accumulate", False)
    seedfill = filled(lambda s, t: ints(D.g, s, -64, 64, t)) if acc else nan_fill
    dw = Buf(_T(dwd), seedfill)
    db = None
    if kw.get("db") is not None:
        db = Buf(_T(kw["db"]), seedfill)
        kw["db"] = db.t
    K.conv2d_wgrad(p.t, q.t, dw.t, **kw)
    torch.cuda.synchronize()
    p64, q64 = p.t.double(), q.t.double()
    ref = wgrad_ref(p64, q64, R, S, stride, dil, ph, pw)
    absr = wgrad_ref(p64.abs(), q64.abs(), R, S, stride, dil, ph, pw)
    if exact:
        assert_exact_range(absr + 64, what)
    bref, babs = p64.sum((0, 1, 2)), p64.abs().sum((0, 1, 2))
    if acc:
        ref = ref + dw.before.as_strided(*dw.desc[:3]).double().reshape(ref.shape)
        if db is not None:
            bref = bref + db.before.as_strided(*db.desc[:3]).double()
    pl = wgrad_plan(p.desc[3], p.desc[0], q.desc[0], R, S, stride, dil, ph)
    n_chain = (pl["spc"] * 64 if pl["kind"] == "wgrad3" else pl["ppc"]) + pl["chunks"] + 2
    compare(dw, ref.reshape(dw.desc[0]), absr.reshape(dw.desc[0]), n_chain, what + ": dw", "conv2d_wgrad", exact)
    if db is not None:
        compare(db, bref, babs, n_chain, what + ": db", "conv2d_wgrad", exact)


def _replay_bias_grad(K, D, a, kw, what):
    dyd, dbd = a[:2]
    acc = a[2] if len(a) > 2 else kw.get("accumulate", False)
    dy = Buf(_T(dyd), filled(D.grad))
    db = Buf(_T(dbd), filled(lambda s, t: ints(D.g, s, -64, 64, t)) if acc else nan_fill)
    K.bias_grad(dy.t, db.t, accumulate=acc)
    torch.cuda.synchronize()
    ref = dy.t.double().sum((0, 1, 2)) + (db.before.as_strided(*db.desc[:3]).double() if acc else 0)
    n_px = dy.t.shape[0] * dy.t.shape[1] * dy.t.shape[2]
    compare(db, ref, dy.t.double().abs().sum((0, 1, 2)) + 64, n_px + 2, what, "bias_grad", D.mode == "int")


def _replay_bias_grad_batched(K, D, a, kw, what):
    dyds, dbds = a[:2]
    acc = a[2] if len(a) > 2 else kw.get("accumulate", False)
    dys = [Buf(_T(d), filled(D.grad)) for d in dyds]
    dbs = [Buf(_T(d), filled(lambda s, t: ints(D.g, s, -64, 64, t)) if acc else nan_fill) for d in dbds]
    K.bias_grad_batched([d.t for d in dys], [d.t for d in dbs], accumulate=acc)
    torch.cuda.synchronize()
    for j, (dy, db) in enumerate(zip(dys, dbs)):
        ref = dy.t.double().sum((0, 1, 2)) + (db.before.as_strided(*db.desc[:3]).double() if acc else 0)
        n_px = dy.t.shape[0] * dy.t.shape[1] * dy.t.shape[2]
        compare(db, ref, dy.t.double().abs().sum((0, 1, 2)) + 64, n_px + 2, f"{what}: job {j}", "bias_grad", D.mode == "int")


def _stem_w(D, wd, cout, R, S):
    w = Buf(_T(wd), filled(lambda s, t: ints(D.g, s, -2, 2, t)))
    return w, w.t.reshape(-1)[:cout * R * S].reshape(cout, R, S, 1)


def _replay_conv_cin1_fwd(K, D, a, kw, what):
    xd, wd, bd, yd = a
    x = Buf(_T(xd), filled(lambda s, t: ints(D.g, s, 0, 3, t)))
    _, Hy, Wy, cout = _T(yd)[0]
    R, S = kw.get("R", 3), kw.get("S", 3)
    wb, w = _stem_w(D, wd, cout, R, S)
    bias = Buf(_T(bd), filled(lambda s, t: ints(D.g, s, -8, 8, t)))
    y = Buf(_T(yd), nan_fill)
    rb = None
    if kw.get("relu_bits_out") is not None:
        rb = Buf(_T(kw["relu_bits_out"]), nan_fill)
        kw["relu_bits_out"] = rb.t
    K.conv_cin1_fwd(x.t, wb.t, bias.t, y.t, **kw)
    torch.cuda.synchronize()
    v = conv_ref(x.t.double(), w.double(), R, S, kw.get("stride", 1), kw.get("dil", 1), kw.get("pad_h", 0), kw.get("pad_w", 0), Hy, Wy)
    v = v + bias.t.double()
    if kw.get("relu"):
        v = v.clamp_min(0)
    yq = v.float().to(y.desc[3])
    y.check_out(yq, what + ": y")
    if rb is not None:
        rb.check_out(bits_of(yq), what + ": relu bits")


def _replay_conv_cin1_dgrad(K, D, a, kw, what):
    dyd, wd, dxd = a
    dy = Buf(_T(dyd), filled(D.grad))
    n, Ho, Wo, cout = dy.desc[0]
    assert kw.get("pad_h", 0) == 0 and kw.get("R", 3) == 3
    wb, w = _stem_w(D, wd, cout, 3, 3)
    dx = Buf(_T(dxd), nan_fill)
    K.conv_cin1_dgrad(dy.t, wb.t, dx.t, **kw)
    torch.cuda.synchronize()
    # the transpose of the valid forward convolution: dx[i + r, j + s] += sum_c dy[i, j, c] w[c, r, s]
    ref = torch.zeros(dx.desc[0], dtype=torch.float64, device=DEV)
    w64 = w.double()
    for r in range(3):
        for s in range(3):
            ref[:, r:r + Ho, s:s + Wo, :] += dy.t.double() @ w64[:, r, s, :]
    dx.check_out(ref.float(), what + ": dx")


def _replay_conv_cin1_wgrad(K, D, a, kw, what):
    xd, dyd, dwd, dbd = a
    acc = kw.get("accumulate", False)
    x = Buf(_T(xd), filled(lambda s, t: ints(D.g, s, 0, 3, t)))
    dy = Buf(_T(dyd), filled(D.grad))
    seedfill = filled(lambda s, t: ints(D.g, s, -64, 64, t)) if acc else nan_fill
    dw, db = Buf(_T(dwd), seedfill), Buf(_T(dbd), seedfill)
    K.conv_cin1_wgrad(x.t, dy.t, dw.t, db.t, **kw)
    torch.cuda.synchronize()
    cout = dy.desc[0][3]
    ref = wgrad_ref(dy.t.double(), x.t.double(), 3, 3).reshape(cout, 9)
    assert_exact_range(wgrad_ref(dy.t.double().abs(), x.t.double(), 3, 3).reshape(-1) + 64, what)
    bref = dy.t.double().sum((0, 1, 2))
    if acc:
        ref = ref + dw.before.as_strided(*dw.desc[:3]).double().reshape(cout, 9)
        bref = bref + db.before.as_strided(*db.desc[:3]).double()
    dw.check_out(ref.reshape(dw.desc[0]).float(), what + ": dw")
    db.check_out(bref.reshape(db.desc[0]).float(), what + ": db")


def _replay_head_fwd(K, D, a, kw, what):
    xd, wd, bd, yd = a
    x = Buf(_T(xd), filled(D.act))
    C, Cin = _T(yd)[0][3], x.desc[0][3]
    wb = Buf(_T(wd), filled(D.grad))
    w = wb.t.reshape(-1)[:C * Cin].reshape(C, Cin)
    bias = Buf(_T(bd), filled(lambda s, t: ints(D.g, s, -8, 8, t)))
    y = Buf(_T(yd), nan_fill)
    K.head_fwd(x.t, wb.t, bias.t, y.t)
    torch.cuda.synchronize()
    y.check_out((x.t.double() @ w.double().T + bias.t.double()).float(), what)


def _replay_head_bwd(K, D, a, kw, what):
    xd, dyd, wd, dxd, dwd, dbd = a
    relu_mask, acc = kw.get("relu_mask", True), kw.get("accumulate", False)
    x = Buf(_T(xd), filled(lambda s, t: ints(D.g, s, -1, 3, t)))      # (the ReLU gate x > 0 has both outcomes)
    dy = Buf(_T(dyd), filled(D.grad))
    C, Cin = dy.desc[0][3], x.desc[0][3]
    wb = Buf(_T(wd), filled(D.grad))
    w = wb.t.reshape(-1)[:C * Cin].reshape(C, Cin)
    dx = Buf(_T(dxd), nan_fill)
    seedfill = filled(lambda s, t: ints(D.g, s, -64, 64, t)) if acc else nan_fill
    dw, db = Buf(_T(dwd), seedfill), Buf(_T(dbd), seedfill)
    K.head_bwd(x.t, dy.t, wb.t, dx.t, dw.t, db.t, relu_mask=relu_mask, accumulate=acc)
    torch.cuda.synchronize()
    x64, dy64 = x.t.double(), dy.t.double()
    g = dy64 @ w.double()
    if relu_mask:
        g = torch.where(x64 > 0, g, torch.zeros_like(g))
    dx.check_out(g.float().to(dx.desc[3]), what + ": dx")
    rw = dy64.reshape(-1, C).T @ x64.reshape(-1, Cin)
    assert_exact_range(dy64.abs().reshape(-1, C).T @ x64.abs().reshape(-1, Cin) + 64, what)
    rb = dy64.sum((0, 1, 2))
    if acc:
        rw = rw + dw.before.as_strided(*dw.desc[:3]).double().reshape(C, Cin)
        rb = rb + db.before.as_strided(*db.desc[:3]).double()
    dw.check_out(rw.reshape(dw.desc[0]).float(), what + ": dw")
    db.check_out(rb.reshape(db.desc[0]).float(), what + ": db")


# ================================================================================================ 1. the recorded call set
def _label(call):
    name, a, kw = call
    shapes = "/".join("x".join(map(str, v[1][0])) for v in a if isinstance(v, tuple) and len(v) == 2 and v[0] == "T")
    flags = ",".join(k for k, v in sorted(kw.items()) if v not in (None, False, 0, 1.0) and k not in ("R", "S"))
    return f"{name}({shapes}{';' + flags if flags else ''})"


@gpu
@pytest.mark.parametrize("cfg,idx", [(c, i) for c in CONFIGS for i in range(COUNTS[c])])
def test_recorded_call(K, cfg, idx):
    """Call ``idx`` of the model's recorded conv-family launches, replayed on exact-integer data: bit for bit against float64."""
    calls = recorded(K, cfg)
    assert len(calls) == COUNTS[cfg], (cfg, len(calls), [c[0] for c in calls])
    call = calls[idx]
    replay(K, call, "int", 1000 + idx, f"{cfg}[{idx}] {_label(call)}")


@gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_gaussian_recorded(K, cfg):
    """The recorded conv2d / conv2d_wgrad / bias-gradient calls on Gaussian data, within the error bounds of the module docstring."""
    calls = recorded(K, cfg)
    Stats.worst.clear()
    for idx, call in enumerate(calls):
        if call[0] in ("conv2d", "conv2d_wgrad", "bias_grad", "bias_grad_batched") and call[2].get("stem") is None and \
                not call[2].get("pool_only"):
            replay(K, call, "gauss", 5000 + idx, f"{cfg}[{idx}] gaussian {_label(call)}")
    print(f"{cfg}: largest err / bound per family: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(Stats.worst.items())))
    assert Stats.worst


# ================================================================================================ 2. planner edges
def conv_case(K, B, Cin, H, W, Cout, R=3, S=3, pad=0, stride=1, dtype=torch.bfloat16, seed=0, what=""):
    """One dense conv2d (bias + ReLU) on exact-integer data, checked bit for bit; returns the plan note."""
    D = Data("int", seed)
    x = D.act((B, H, W, Cin), dtype)
    w = D.grad((Cout, R, S, Cin), dtype)
    bias = ints(D.g, (Cout,), -64, 64, torch.float32)
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    y = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=dtype, device=DEV)
    K.conv2d(x, w.reshape(-1), bias, y, R=R, S=S, stride=stride, pad_h=pad, pad_w=pad, relu=True)
    note = plan_note()
    torch.cuda.synchronize()
    ref = (conv_ref(x.double(), w.double(), R, S, stride, 1, pad, pad) + bias.double()).clamp_min(0)
    same_bits(y, ref.float().to(dtype), f"{what} [{note}]")
    return note


def igemm_note(note):
    m = re.match(r"(igemm2?) per-tap (\d+) x (\d+) tile.*: (\d+) tiles x (\d+) splits, (\d+) K-steps each", note)
    assert m, note
    return m.group(1), int(m.group(4)), int(m.group(5)), int(m.group(6))


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout,R,pad,split", [
    (2, 320, 12, 12, 128, 3, 0, -1),      # 2 tiles, 45 K-steps: the planner's 8 splits of 6 (last split 3)
    (2, 320, 12, 12, 128, 3, 0, 2),       # forced 2: 23 + 22
    (2, 320, 12, 12, 128, 3, 0, 4),       # 12 x 3 + 9
    (2, 320, 12, 12, 128, 3, 0, 7),       # 7 x 6 + 3
    (1, 192, 14, 14, 64, 3, 1, 5),        # 64-channel tile (bm 256), 27 K-steps in 5 splits of 6 (last 3), padded
    (1, 64, 97, 130, 128, 3, 0, -1),      # 95 tiles (just under the 96-tile threshold): 9 K-steps -> 2 splits of 5 + 4
    (1, 64, 98, 130, 128, 3, 0, -1),      # 96 tiles: unsplit
    (1, 64, 99, 130, 128, 3, 0, -1),      # 97 tiles: unsplit
    (1, 192, 10, 10, 128, 1, 0, -1),      # 3 K-steps: under the 4-step floor, unsplit
    (1, 448, 10, 10, 128, 1, 0, -1),      # 7 K-steps: one split would keep < 4 -> unsplit
    (1, 512, 10, 10, 128, 1, 0, -1),      # 8 K-steps: 2 splits of 4
    (2, 128, 20, 18, 128, 2, 0, 3),       # 2x2 stride 2 (the up-convolutions' data-gradient form), forced 3 splits
])
def test_igemm2_split_plan_edges(K, B, Cin, H, W, Cout, R, pad, split):
    stride = 2 if R == 2 else 1
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    v2, bm, bn, tiles, splits, kps = igemm_plan(torch.bfloat16, Cin, Cout, B * Ho * Wo, R, R, split)
    with knobs(IGEMM_SPLIT=split, IGEMM_HALO=0, IGEMM_PACKED=0):
        note = conv_case(K, B, Cin, H, W, Cout, R, R, pad, stride, seed=B * Cin + H, what="igemm2 split")
    assert igemm_note(note) == ("igemm2", tiles, splits, kps), (note, tiles, splits, kps)


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout", [
    (8, 64, 254, 254, 64),      # cfg2's second first-level convolution: 252 x 252 outputs, ragged last patch row and column
    (4, 128, 83, 147, 128),     # 128-channel tile, odd extents: 81 x 145 outputs (one-row / one-column patch remainders)
    (3, 192, 98, 130, 256),     # three channel slices, two channel tiles, exact patch cover
])
def test_igemm3m_plan_edges(K, B, Cin, H, W, Cout):
    """The shared-halo kernel (8 x 16 output patches) on ragged patch grids; the plan note names it and its block count."""
    Ho, Wo = H - 2, W - 2
    bn = 128 if Cout % 128 == 0 else 64
    blocks = B * cdiv(Ho, 8) * cdiv(Wo, 16) * (Cout // bn)
    assert igemm_plan(torch.bfloat16, Cin, Cout, B * Ho * Wo, 3, 3)[4] == 1 and blocks >= 400
    note = conv_case(K, B, Cin, H, W, Cout, seed=Cin + H, what="igemm3m")
    m = re.match(r"igemm3m shared-halo 8x16 patches x (\d+) ch: (\d+) blocks", note)
    assert m and (int(m.group(1)), int(m.group(2))) == (bn, blocks), note


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout,split", [
    (1, 272, 12, 12, 64, -1),     # 1 tile, 153 K-steps: 16 splits of 10 (last 3)
    (1, 256, 12, 12, 128, -1),    # 144 K-steps: 16 splits of 9
    (1, 144, 12, 12, 64, -1),     # 81 K-steps: 14 effective splits of 6 (last 3)
    (2, 64, 40, 40, 128, -1),     # 23 tiles, 36 K-steps: 9 splits of 4
    (2, 32, 30, 30, 64, 11),      # forced 11: 18 K-steps -> 9 splits of 2
])
def test_igemm_fp32_split_plan_edges(K, B, Cin, H, W, Cout, split):
    v2, bm, bn, tiles, splits, kps = igemm_plan(torch.float32, Cin, Cout, B * (H - 2) * (W - 2), 3, 3, split)
    with knobs(IGEMM_SPLIT=split):
        note = conv_case(K, B, Cin, H, W, Cout, dtype=torch.float32, seed=Cin + H, what="igemm fp32 split")
    assert igemm_note(note) == ("igemm", tiles, splits, kps), (note, tiles, splits, kps)


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout,xcd", [
    (100, 576, 13, 13, 128, 1),    # 9 channel slices in 2 splits of 5 + 4
    (60, 896, 13, 13, 128, 1),     # 14 slices in 3 splits of 5, 5, 4
    (60, 896, 13, 13, 128, 2),     # ... dealt XCD by XCD (180 blocks: 180 % 8 = 4)
    (40, 1024, 13, 13, 256, 1),    # the centre's 1024 input channels: 16 slices in 3 splits of 6, 6, 4
    (20, 704, 27, 27, 128, 1),     # five tiles per image (5 rows of 25), 11 slices in 2 splits of 6 + 5
])
def test_igemm3p_channel_split_plan_edges(K, B, Cin, H, W, Cout, xcd):
    pp = packed_plan(B, H - 2, W - 2, Cin, Cout)
    assert pp is not None and pp[2] > 1, pp
    PR, tpi, splits, cps = pp
    with knobs(IGEMM_XCD=xcd):
        note = conv_case(K, B, Cin, H, W, Cout, seed=Cin + B, what="igemm3p")
    m = re.match(r"igemm3p packed rows \((\d+) rows of (\d+) px per 128-px tile\): (\d+) x (\d+) blocks x (\d+) channel-slice splits", note)
    assert m and (int(m.group(1)), int(m.group(3)), int(m.group(5))) == (PR, B * tpi, splits), (note, pp)


@gpu
@pytest.mark.parametrize("B,Cin,H,W,Cout,split,xcd", [
    (1, 128, 12, 12, 128, 1, 1), (1, 128, 12, 12, 128, 1, 2),           # 1 block: below 16, natural grid
    (1, 128, 34, 34, 256, 1, 1), (1, 128, 34, 34, 256, 1, 2),           # exactly 16 blocks
    (1, 128, 22, 22, 128, 5, 1), (1, 128, 22, 22, 128, 5, 2),           # 4 tiles x 5 splits = 20: 20 % 8 = 4
    (1, 448, 20, 20, 128, 7, 1), (1, 448, 20, 20, 128, 7, 2),           # 3 tiles x 7 splits = 21
    (2, 64, 40, 40, 128, 1, 2),                                         # 23 tiles, activations outweigh the weights: forced order only
])
def test_xcd_grid_edges(K, B, Cin, H, W, Cout, split, xcd):
    """xcd_grid deals the blocks of a weights-heavy per-tap layer XCD by XCD (DCT_TUNE_IGEMM_XCD 1; 2: every layer) over a grid rounded
    up to a multiple of 8: totals below 16 keep the natural grid, the ragged last round must still run every block."""
    v2, bm, bn, tiles, splits, kps = igemm_plan(torch.bfloat16, Cin, Cout, B * (H - 2) * (W - 2), 3, 3, split)
    with knobs(IGEMM_SPLIT=split, IGEMM_HALO=0, IGEMM_PACKED=0, IGEMM_XCD=xcd):
        note = conv_case(K, B, Cin, H, W, Cout, seed=Cin + H + xcd, what=f"xcd {xcd}")
    assert igemm_note(note) == ("igemm2", tiles, splits, kps), note


def wgrad_case(K, p_shape, q_shape, R=3, S=3, stride=1, pad=0, dtype=torch.bfloat16, with_db=False, acc=False, seed=0, what="",
               keep=None):
    """One dense conv2d_wgrad on exact-integer data, checked bit for bit; returns the plan note."""
    D = Data("int", seed)
    p, q = D.grad(p_shape, dtype), D.act(q_shape, dtype)
    Cp, Cq = p_shape[3], q_shape[3]
    seed_w = ints(D.g, (Cp, R, S, Cq), -64, 64, torch.float32) if acc else None
    dw = seed_w.clone() if acc else torch.full((Cp, R, S, Cq), float("nan"), device=DEV)
    db = None
    if with_db:
        seed_b = ints(D.g, (Cp,), -64, 64, torch.float32)
        db = seed_b.clone() if acc else torch.full((Cp,), float("nan"), device=DEV)
    K.conv2d_wgrad(p, q, dw, R=R, S=S, stride=stride, pad_h=pad, pad_w=pad, accumulate=acc, db=db)
    note = plan_note()
    torch.cuda.synchronize()
    ref = wgrad_ref(p.double(), q.double(), R, S, stride, 1, pad, pad)
    assert_exact_range(wgrad_ref(p.double().abs(), q.double(), R, S, stride, 1, pad, pad) + 64, what)
    if acc:
        ref = ref + seed_w.double()
    same_bits(dw, ref.float(), f"{what} [{note}]: dw")
    if with_db:
        same_bits(db, (p.double().sum((0, 1, 2)) + (seed_b.double() if acc else 0)).float(), f"{what} [{note}]: db")
    return note


def wgrad_note(note):
    """(kernel, pixel chunks, direct, loop form: "plain" | "lean" | "lean + skip") of a weight-gradient plan note."""
    m = re.match(r"(wgrad3 filter-row|wgrad2 per-tap|wgrad) \d+ x \d+ tile: \d+ x \d+ x \d+ taps, (\d+) pixel chunks( \((narrow|wide) rows\))?(, direct)?"
                 r"(, (lean|lean \+ skip))?$", note)
    assert m, note
    return m.group(1).split()[0], int(m.group(2)), bool(m.group(5)), m.group(7) or "plain"


@gpu
@pytest.mark.parametrize("p_shape,R,stride,chunks,target,acc,db", [
    ((2, 30, 30, 512), 3, 1, 1, 256, False, True),       # one chunk: the direct path (no slab) ...
    ((2, 30, 30, 512), 3, 1, 1, 256, True, True),        # ... adding to the gradient
    ((3, 33, 29, 256), 3, 1, -1, 256, True, False),      # 36 tiles: 7 chunks, ragged last chunk
    ((2, 21, 23, 256), 3, 1, 3, 256, False, True),       # forced 3 chunks
    ((4, 60, 60, 128), 3, 1, -1, 256, False, True),      # 9 tiles: 28 chunks (28 % 8 = 4), dealt XCD by XCD
    ((2, 37, 41, 128), 3, 1, 13, 256, True, False),      # forced 13 chunks: 13 % 8 = 5, ragged last chunk
    ((8, 64, 64, 64), 1, 1, -1, 256, False, True),       # 1x1: 1 tile, 128 chunks by the pixel floor -> the 64-chunk cap
    ((8, 22, 22, 1024), 3, 1, -1, 8192, False, True),    # 1024 x 1024: 14 chunks wanted, the 192 MiB slab cap allows 5
    ((8, 9, 9, 1024), 3, 1, -1, 256, False, True),       # cfg2's centre 1024 -> 1024 at its shape: direct
])
def test_wgrad2_plan_edges(K, p_shape, R, stride, chunks, target, acc, db):
    n, Hp, Wp, Cp = p_shape
    q_shape = (n, (Hp - 1) * stride + R, (Wp - 1) * stride + R, Cp)
    pl = wgrad_plan(torch.bfloat16, p_shape, q_shape, R, R, stride, chunks_knob=chunks, rows=0, target=target)
    assert pl["kind"] == "wgrad2"
    with knobs(WGRAD_CHUNKS=chunks, WGRAD_ROWS=0, WGRAD_TARGET=target):
        note = wgrad_case(K, p_shape, q_shape, R, R, stride, with_db=db, acc=acc, seed=Cp + Hp, what="wgrad2")
    assert wgrad_note(note) == ("wgrad2", pl["chunks"], pl["direct"], "lean"), (note, pl)
    if p_shape == (8, 64, 64, 64):
        assert pl["chunks"] == 64 and cdiv(8 * 64 * 64, 4 * 64) == 128, pl
    if p_shape == (8, 22, 22, 1024):
        assert pl["chunks"] == 5 and 14 * 1024 * 1024 * 9 * 4 > (192 << 20)


@gpu
@pytest.mark.parametrize("p_shape,Cq,pad,chunks,target3", [
    ((2, 40, 130, 64), 64, 0, -1, 768),     # wide rows: 3 segments per row, a 2-pixel tail
    ((3, 31, 200, 128), 64, 0, -1, 768),    # wide rows, 8-pixel tail, two P tiles
    ((2, 33, 200, 64), 128, 2, -1, 768),    # wide rows, padded (the non-lean form), 8-pixel tail
    ((5, 21, 20, 64), 64, 0, -1, 768),      # narrow rows: pitch 22, 3 rows per step
    ((4, 45, 48, 64), 64, 0, 7, 768),       # narrow rows: pitch 50, one row per step; 7 chunks of a ragged segment split
    ((3, 50, 130, 64), 64, 0, 11, 768),     # forced 11 chunks over 450 segments: 41 per chunk, the last ragged
    ((8, 256, 254, 64), 64, 0, -1, 4096),   # cfg2's first-level width and batch, a larger target: the 256-chunk cap
])
def test_wgrad3_plan_edges(K, p_shape, Cq, pad, chunks, target3):
    n, Hp, Wp, Cp = p_shape
    q_shape = (n, Hp + 2 - 2 * pad, Wp + 2 - 2 * pad, Cq)
    pl = wgrad_plan(torch.bfloat16, p_shape, q_shape, 3, 3, pad=pad, chunks_knob=chunks, target3=target3)
    assert pl["kind"] == "wgrad3", pl
    with knobs(WGRAD_CHUNKS=chunks, WGRAD3_TARGET=target3):
        note = wgrad_case(K, p_shape, q_shape, pad=pad, with_db=True, seed=Hp + Wp, what="wgrad3")
    # the lean loop (buffer descriptors, empty sub-steps skipped) takes the layers without padding; the padded one runs the plain loop
    assert wgrad_note(note) == ("wgrad3", pl["chunks"], pl["direct"], "plain" if pad else "lean + skip"), (note, pl)
    if target3 == 4096:
        assert pl["chunks"] == 256, pl
    if chunks == 11:
        assert pl["nseg"] % pl["spc"] != 0, pl


@gpu
@pytest.mark.parametrize("p_shape,Cq,R,stride,dtype", [
    ((2, 30, 30, 64), 64, 3, 1, torch.float32),       # fp32: the v1 kernel
    ((2, 62, 62, 128), 128, 3, 1, torch.float32),
    ((4, 33, 35, 64), 128, 2, 2, torch.float32),      # 2x2 stride 2 (up-convolution form)
])
def test_wgrad_v1_plan_edges(K, p_shape, Cq, R, stride, dtype):
    n, Hp, Wp, Cp = p_shape
    q_shape = (n, (Hp - 1) * stride + R, (Wp - 1) * stride + R, Cq)
    pl = wgrad_plan(dtype, p_shape, q_shape, R, R, stride)
    note = wgrad_case(K, p_shape, q_shape, R, R, stride, dtype=dtype, seed=Hp + Cq, what="wgrad v1")
    assert wgrad_note(note) == ("wgrad", pl["chunks"], False, "plain"), (note, pl)


@gpu
@pytest.mark.parametrize("p_shape,rows,chunks,lean,form", [
    ((5, 21, 20, 64), 1, -1, 0, "plain"),      # filter-row, narrow rows: the plain loop ...
    ((5, 21, 20, 64), 1, -1, 1, "lean"),       # ... and the lean one without the skipping
    ((2, 21, 23, 256), 0, 3, 0, "plain"),      # per-tap, forced 3 chunks
])
def test_wgrad_loop_forms(K, p_shape, rows, chunks, lean, form):
    """DCT_TUNE_LEAN picks the loop form of the two LDS-DMA kernels, the plan note names it, and every form gives the same bits (those of
    the float64 reference on exact-integer data) on cases that test_wgrad3_plan_edges / test_wgrad2_plan_edges run in the shipped form."""
    n, Hp, Wp, Cp = p_shape
    q_shape = (n, Hp + 2, Wp + 2, Cp)
    pl = wgrad_plan(torch.bfloat16, p_shape, q_shape, 3, 3, chunks_knob=chunks, rows=rows, lean=lean)
    with knobs(WGRAD_CHUNKS=chunks, WGRAD_ROWS=rows, LEAN=lean):
        note = wgrad_case(K, p_shape, q_shape, with_db=True, seed=Hp + Wp, what=f"LEAN={lean}")
    assert wgrad_note(note) == ("wgrad3" if rows else "wgrad2", pl["chunks"], pl["direct"], form), (note, pl)


# ================================================================================================ 3. the 32-bit addressing guards
def banded(D, shape, dtype, gen_fn, band):
    """Zeros, with data (gen_fn) in the first and last image -- or, for a single image, the first and last ``band`` rows."""
    t = torch.zeros(shape, dtype=dtype, device=DEV)
    if shape[0] > 1:
        t[0] = gen_fn(shape[1:], dtype)
        t[-1] = gen_fn(shape[1:], dtype)
    else:
        t[0, :band] = gen_fn((band,) + tuple(shape[2:]), dtype)
        t[0, -band:] = gen_fn((band,) + tuple(shape[2:]), dtype)
    return t


@gpu
@pytest.mark.parametrize("B,below", [(252, True), (253, False)])
def test_conv_lean_x_bytes_guard(K, B, below):
    """igemm2's lean loop (buffer descriptors) takes activations under 2 GiB (x_bytes < 2^31); the plain loop above.  x [B, 258, 258, 64]
    bf16 with data in the first and last image; every other image's output must be relu(bias).  The plan note does not name the loop
    form, so this pair shows that both sides of the guard compute correctly -- the case above it would catch a guard that let the lean
    form's 32-bit buffer range wrap -- but not which form ran below it."""
    H = W = 258
    x_bytes = B * H * W * 64 * 2
    assert (x_bytes < 2 ** 31) == below
    D = Data("int", B)
    x = banded(D, (B, H, W, 64), torch.bfloat16, D.act, 0)
    w = D.grad((64, 3, 3, 64), torch.bfloat16)
    bias = ints(D.g, (64,), -64, 64, torch.float32)
    y = torch.full((B, H - 2, W - 2, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    with knobs(IGEMM_HALO=0, IGEMM_PACKED=0):
        K.conv2d(x, w.reshape(-1), bias, y, relu=True)
        note = plan_note()
        torch.cuda.synchronize()
    assert note.startswith("igemm2 per-tap"), note
    for i in (0, B - 1):
        ref = (conv_ref(x[i:i + 1].double(), w.double(), 3, 3) + bias.double()).clamp_min(0)
        same_bits(y[i:i + 1], ref.float().to(torch.bfloat16), f"image {i} [{note}]")
    mid = bias.clamp_min(0).to(torch.bfloat16)
    ok = (y[1:B - 1].view(torch.int16) == mid.view(torch.int16)).all()
    assert bool(ok), f"images 1..{B - 2}: not relu(bias) [{note}]"
    del x, y
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("B,kind", [(63, "wgrad3"), (65, "wgrad")])
def test_wgrad_fits32_guard(K, B, kind):
    """wgrad.hip's 32-bit element offsets (fits32: n * sn < 2^30 for p and q; M < 2^24 pixels): p [B, 510, 510, 64], q [B, 512, 512, 64]
    bf16.  63 images: the filter-row kernel at its largest; 65: the wide-offset v1 kernel.  Data in the first and last image only."""
    Hp = Wp = 510
    pl = wgrad_plan(torch.bfloat16, (B, Hp, Wp, 64), (B, Hp + 2, Wp + 2, 64), 3, 3)
    assert pl["kind"] == kind, pl
    D = Data("int", B)
    p = banded(D, (B, Hp, Wp, 64), torch.bfloat16, D.grad, 0)
    q = banded(D, (B, Hp + 2, Wp + 2, 64), torch.bfloat16, D.act, 0)
    dw = torch.full((64, 3, 3, 64), float("nan"), device=DEV)
    K.conv2d_wgrad(p, q, dw)
    note = plan_note()
    torch.cuda.synchronize()
    assert wgrad_note(note)[:2] == (kind, pl["chunks"]), (note, pl)
    idx = [0, B - 1]
    ref = wgrad_ref(p[idx].double(), q[idx].double(), 3, 3)
    same_bits(dw, ref.float(), f"B={B} [{note}]")
    del p, q
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("Hp,Wp,kind", [(2890, 2894, "wgrad3"), (2898, 2898, "wgrad2")])
def test_wgrad3_row_offset_guard(K, Hp, Wp, kind):
    """wgrad3 takes views with h * sh < 2^29 elements per image (p and q); above, the per-tap kernel.  One image of ~2^29 elements, data
    in the first and last 8 rows."""
    assert ((Hp + 2) * (Wp + 2) * 64 < 2 ** 29) == (kind == "wgrad3")
    pl = wgrad_plan(torch.bfloat16, (1, Hp, Wp, 64), (1, Hp + 2, Wp + 2, 64), 3, 3)
    assert pl["kind"] == kind, pl
    D = Data("int", Hp)
    p = banded(D, (1, Hp, Wp, 64), torch.bfloat16, D.grad, 8)
    q = banded(D, (1, Hp + 2, Wp + 2, 64), torch.bfloat16, D.act, 10)
    dw = torch.full((64, 3, 3, 64), float("nan"), device=DEV)
    K.conv2d_wgrad(p, q, dw)
    note = plan_note()
    torch.cuda.synchronize()
    assert wgrad_note(note)[:2] == (kind, pl["chunks"]), (note, pl)
    # only the p rows with data contribute: the first 8 rows read q rows 0..9, the last 8 the last 10
    ref = wgrad_ref(p[:, :8].double(), q[:, :10].double(), 3, 3) + wgrad_ref(p[:, -8:].double(), q[:, -10:].double(), 3, 3)
    same_bits(dw, ref.float(), f"{Hp}x{Wp} [{note}]")
    del p, q
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("which,below", [("x", True), ("x", False), ("y", True), ("y", False)])
def test_igemm3m_x32_y16_guard(K, which, below):
    """igemm3m addresses x and y with 32-bit element offsets: the host admits it only while n * sn < 2^31 elements for x (x32) and for y
    (y16); above, the per-tap kernel runs.  A two-image view whose image stride is just below (2^30 - 8) or at 2^30 elements -- about
    2 GiB of buffer, the other tensor small and dense; both images carry data and the gap between them must stay unwritten."""
    B, H, W, C = 2, 130, 258, 64
    Ho, Wo = H - 2, W - 2
    sn = 2 ** 30 - 8 if below else 2 ** 30
    assert (B * sn < 2 ** 31) == below
    D = Data("int", 7 + below)
    w = D.grad((C, 3, 3, C), torch.bfloat16)
    bias = ints(D.g, (C,), -64, 64, torch.float32)
    img_x, img_y = H * W * C, Ho * Wo * C
    if which == "x":
        xbase = torch.zeros(sn + img_x, dtype=torch.bfloat16, device=DEV)
        x = xbase.as_strided((B, H, W, C), (sn, W * C, C, 1))
        ybase = torch.full((B * img_y,), float("nan"), dtype=torch.bfloat16, device=DEV)
        y = ybase.view(B, Ho, Wo, C)
    else:
        xbase = torch.zeros(B * img_x, dtype=torch.bfloat16, device=DEV)
        x = xbase.view(B, H, W, C)
        ybase = torch.full((sn + img_y,), float("nan"), dtype=torch.bfloat16, device=DEV)
        y = ybase.as_strided((B, Ho, Wo, C), (sn, Wo * C, C, 1))
    for i in range(B):
        x[i] = D.act((H, W, C), torch.bfloat16)
    K.conv2d(x, w.reshape(-1), bias, y, relu=True)
    note = plan_note()
    torch.cuda.synchronize()
    assert note.startswith("igemm3m shared-halo" if below else "igemm2 per-tap"), note
    for i in range(B):
        ref = (conv_ref(x[i:i + 1].double(), w.double(), 3, 3) + bias.double()).clamp_min(0)
        same_bits(y[i:i + 1], ref.float().to(torch.bfloat16), f"{which} {'below' if below else 'above'}: image {i} [{note}]")
    if which == "y":
        nanbits = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item()
        assert bool((ybase[img_y:sn].view(torch.int16) == nanbits).all()), f"y: written between the images [{note}]"
    del xbase, ybase, x, y
    torch.cuda.empty_cache()
