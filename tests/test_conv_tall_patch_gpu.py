"""The 16 x 16-patch form of the shared-halo 3x3 kernel (igemm3m_tall_kernel, DCT_TUNE_IGEMM_HALO_TALL = knob 40): one halo stage for
any number of channel slices, re-staged in the open between two barriers at every slice change; a wave owns four patch rows.

Every case runs with knob 40 = 2 (every layer the form can run) and is compared
  * bit for bit with the same call under knob 40 = 0 -- the 8 x 16 patches, whose MFMA sequence per output element it repeats --
  * and with F.conv2d in fp32 on the CPU, with the comparison and tolerance of test_kernels_gpu.test_conv2d_3x3_shared_halo.
The plan note (dct_debug_last_plan) of every launch is asserted, so that neither side silently runs another kernel: the shapes are
the smallest at which each mechanism can go wrong, far below the planner's thresholds, so the tests also set knob 19 (fewest blocks
of the shared-halo kernel) to 1, knob 20 (least cover of its patches) to 1 and knob 1 (split-K factor of the per-tap plan, which a
shared-halo layer must not want) to 1 -- without the last two the knob-0 side of the ragged shapes would be the per-tap kernel, whose
tap-major K order differs in the last bits.  All four are restored afterwards.
"""
import ctypes
import functools
import math
import os
from contextlib import contextmanager

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = torch.bfloat16
KNOB_SPLIT, KNOB_MIN_BLOCKS, KNOB_COVER, KNOB_TALL = 1, 19, 20, 40
DEFAULTS = {KNOB_SPLIT: -1, KNOB_MIN_BLOCKS: 400, KNOB_COVER: 75, KNOB_TALL: 1}      # csrc/igemm.hip
_RACE_LAUNCHES = 200 if os.environ.get("DCT_LONG_TESTS") else 50

SHAPES = [
    (2, 64, 34, 34, 128, 0),      # exact 16 x 16 cover, one slice: no re-stage
    (2, 128, 35, 21, 128, 0),     # Ho = 33: the last patch row holds ONE image row (three of four pixel waves dead, staging and
                                  # taking the barriers); Wo = 19: ragged columns; one re-stage
    (1, 192, 27, 40, 256, 2),     # data-gradient form (halo outside the image reads zeros); two re-stages: both weight-buffer
                                  # parities at a slice change; two Cout tiles
    (3, 256, 20, 20, 128, 0),     # four slices, image stride
]
EPILOGUE_SHAPES = SHAPES[1:3]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _lib():
    from dct_amd import _lib
    return _lib.load()


@contextmanager
def tall(value):
    lib = _lib()
    try:
        for k, v in ((KNOB_SPLIT, 1), (KNOB_MIN_BLOCKS, 1), (KNOB_COVER, 1), (KNOB_TALL, value)):
            assert lib.dct_tune_set(k, v) == 0
        yield
    finally:
        for k, v in DEFAULTS.items():
            lib.dct_tune_set(k, v)


def _note():
    f = _lib().dct_debug_last_plan
    f.restype = ctypes.c_char_p
    return f().decode()


def _conv(ops, value, *args, **kw):
    """ops.conv2d under knob 40 = value; the launch must have taken the patch height that value stands for"""
    with tall(value):
        ops.conv2d(*args, **kw)
        note = _note()
    want = "igemm3m shared-halo %s patches x 128 ch" % ("16x16" if value else "8x16")
    assert note.startswith(want), (value, note)


def q(t):
    return t.to(DT).float()


def to_dev(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(DT).to(DEV)


def to_cpu(t_nhwc):
    return t_nhwc.float().cpu().permute(0, 3, 1, 2).contiguous()


def close(got, ref, what, rtol=2e-2):
    """test_kernels_gpu.close for bf16"""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, what
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs()
    bad = err > rtol * scale + rtol * ref.abs()
    assert not bad.any() and torch.isfinite(got).all(), f"{what}: {int(bad.sum())}/{bad.numel()} off; max err {err.max().item():.3e}; ref scale {scale:.3e}"


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16) if a.dtype == DT else a, b.view(torch.int16) if b.dtype == DT else b)


def _pack_bits(t_nhwc):
    pos = (t_nhwc.float() > 0).to(torch.int32)
    n, h, w, c = pos.shape
    return (pos.view(n, h, w, c // 8, 8) << torch.arange(8, device=pos.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs and the fp32 CPU reference of a shape: computed once, shared by the tests, never written to."""
    B, Cin, H, W, Cout, pad = shape
    g = torch.Generator().manual_seed(11)
    x = q(torch.randn(B, Cin + 64, H, W, generator=g))           # the kernels see channels 64.. of a wider buffer
    w = q(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9))
    b = torch.randn(Cout, generator=g)
    plain = F.conv2d(x[:, 64:], w, padding=pad)
    Ho, Wo = plain.shape[2], plain.shape[3]
    maskt = q(torch.randn(B, Cout, Ho, Wo, generator=g))
    old = q(torch.randn(B, Cout + 64, Ho, Wo, generator=g))
    wd = w.permute(0, 2, 3, 1).contiguous().to(DT).to(DEV)
    return dict(x=x, w=w, b=b, plain=plain, maskt=maskt, old=old, Ho=Ho, Wo=Wo,
                xd=to_dev(x)[..., 64:], wd=wd, bd=b.to(DEV), maskd=to_dev(maskt))


@pytest.mark.parametrize("shape", SHAPES)
def test_tall_patch_matches_8x16_patches_and_cpu(ops, shape):
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    ys = {}
    for value in (2, 0):
        y = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        _conv(ops, value, c["xd"], c["wd"], c["bd"], y, pad_h=pad, pad_w=pad, relu=True)
        ys[value] = y
    assert same(ys[2], ys[0]), "16 x 16 patches differ from the 8 x 16 patches"
    close(to_cpu(ys[2]), F.relu(c["plain"] + c["b"].view(1, -1, 1, 1)), "tall-patch conv fwd")


def _masked_accumulate(ops, c, shape, value, fill=None):
    """mask (ReLU gate of the destination, first 64 channels) + mask_scale + accumulate, x and y channel slices of wider buffers"""
    B, Cin, H, W, Cout, pad = shape
    yd = to_dev(c["old"]) if fill is None else torch.full((B, c["Ho"], c["Wo"], Cout + 64), fill, dtype=DT, device=DEV)
    _conv(ops, value, c["xd"], c["wd"], None, yd[..., :Cout], pad_h=pad, pad_w=pad, mask=c["maskd"], mask_channels=64,
          mask_scale=2.0, accumulate=True)
    return yd


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES)
def test_tall_patch_mask_accumulate_views(ops, shape):
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    got, want = _masked_accumulate(ops, c, shape, 2), _masked_accumulate(ops, c, shape, 0)
    assert same(got, want)
    masked = c["plain"].clone()
    masked[:, :64] = torch.where(c["maskt"][:, :64] > 0, c["plain"][:, :64] * 2.0, torch.zeros(()))
    ref = c["old"].clone()
    ref[:, :Cout] += masked
    close(to_cpu(got), ref, "tall-patch conv mask/accumulate/views")


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES)
def test_tall_patch_gate_bits(ops, shape):
    """mask_bits (the one-bit image of the mask) and relu_bits_out"""
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    mbits = _pack_bits(c["maskd"])
    outs = {}
    for value in (2, 0):
        plain = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        _conv(ops, value, c["xd"], c["wd"], None, plain, pad_h=pad, pad_w=pad, mask=c["maskd"], mask_scale=2.0)
        gated = torch.full_like(plain, float("nan"))
        _conv(ops, value, c["xd"], c["wd"], None, gated, pad_h=pad, pad_w=pad, mask=c["maskd"], mask_scale=2.0, mask_bits=mbits)
        y = torch.full_like(plain, float("nan"))
        bits = ops.relu_bits_like(y)
        bits.fill_(0xA5)
        _conv(ops, value, c["xd"], c["wd"], c["bd"], y, pad_h=pad, pad_w=pad, relu=True, relu_bits_out=bits)
        outs[value] = (plain, gated, y, bits)
    for a, b in zip(outs[2], outs[0]):
        assert same(a, b)
    plain, gated, y, bits = outs[2]
    assert same(plain, gated) and torch.equal(bits, _pack_bits(y))
    assert 0.2 < (y > 0).float().mean().item() < 0.8
    masked = torch.where(c["maskt"] > 0, c["plain"] * 2.0, torch.zeros(()))
    close(to_cpu(gated), masked, "tall-patch conv mask_bits")


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES)
def test_tall_patch_pooling(ops, shape):
    """pool_out + pool_codes and pool_only out of the 256-row tile; odd extents: ceil-mode windows of one row / one column / one pixel"""
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    Hp, Wp = (c["Ho"] + 1) // 2, (c["Wo"] + 1) // 2
    outs = {}
    for value in (2, 0):
        y = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        pooled = torch.full((B, Hp, Wp, Cout), float("nan"), dtype=DT, device=DEV)
        codes = torch.full((B, Hp, Wp, Cout), 255, dtype=torch.uint8, device=DEV)
        bits = ops.relu_bits_like(y)
        bits.fill_(0xA5)
        _conv(ops, value, c["xd"], c["wd"], c["bd"], y, pad_h=pad, pad_w=pad, relu=True, relu_bits_out=bits, pool_out=pooled, pool_codes=codes)
        pooled2 = torch.full_like(pooled, float("nan"))
        codes2 = torch.full_like(codes, 255)
        _conv(ops, value, c["xd"], c["wd"], c["bd"], torch.empty_like(y), pad_h=pad, pad_w=pad, relu=True, pool_out=pooled2, pool_codes=codes2,
              pool_only=True)
        outs[value] = (y, pooled, codes, bits, pooled2, codes2)
    for a, b in zip(outs[2], outs[0]):
        assert same(a, b)
    y, pooled, codes, bits, pooled2, codes2 = outs[2]
    assert same(pooled, pooled2) and torch.equal(codes, codes2) and (codes < 16).all()
    ref = F.max_pool2d(y.float().permute(0, 3, 1, 2), 2, 2, ceil_mode=True).permute(0, 2, 3, 1)
    assert torch.equal(pooled.float(), ref)
    close(to_cpu(y), F.relu(c["plain"] + c["b"].view(1, -1, 1, 1)), "tall-patch conv fwd with pooling")


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES)
def test_tall_patch_is_reproducible(ops, shape):
    """The re-stage of the single halo buffer is the one new synchronisation of the kernel: repeat launches of the two- and three-slice
    shapes, with and without the mask / accumulate epilogue, into prefilled outputs (NaN; ones where the epilogue adds to them) must
    all equal the first."""
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    first = None
    for _ in range(_RACE_LAUNCHES):
        y = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        _conv(ops, 2, c["xd"], c["wd"], c["bd"], y, pad_h=pad, pad_w=pad, relu=True)
        z = _masked_accumulate(ops, c, shape, 2, fill=1.0)
        if first is None:
            first = (y, z)
            assert torch.isfinite(y.float()).all() and torch.isfinite(z.float()).all()
        else:
            assert same(y, first[0]) and same(z, first[1])


def test_tall_patch_planners_choice_threshold(ops):
    """Knob 40 = 1, every other knob at its default: a layer of 128 x 128 outputs x 128 channels takes the 16 x 16 patches from the
    512 blocks of eight images on (csrc/igemm.hip g_tune_igemm_halo_tall_min_blocks) and keeps the 8 x 16 patches at seven; same bits."""
    lib = _lib()
    g = torch.Generator().manual_seed(12)
    x = to_dev(q(torch.randn(8, 64, 130, 130, generator=g)))
    wd = q(torch.randn(128, 64, 3, 3, generator=g) / 24).permute(0, 2, 3, 1).contiguous().to(DT).to(DEV)
    notes, ys = {}, {}
    try:
        for B, value in ((8, 1), (7, 1), (8, 0)):
            assert lib.dct_tune_set(KNOB_TALL, value) == 0
            y = torch.full((B, 128, 128, 128), float("nan"), dtype=DT, device=DEV)
            ops.conv2d(x[:B], wd, None, y)
            notes[B, value], ys[B, value] = _note(), y
    finally:
        lib.dct_tune_set(KNOB_TALL, DEFAULTS[KNOB_TALL])
    assert notes[8, 1].startswith("igemm3m shared-halo 16x16 patches x 128 ch: 512 blocks"), notes
    assert notes[7, 1].startswith("igemm3m shared-halo 8x16 patches x 128 ch: 896 blocks"), notes
    assert notes[8, 0].startswith("igemm3m shared-halo 8x16 patches x 128 ch: 1024 blocks"), notes
    assert same(ys[8, 1], ys[8, 0]) and same(ys[7, 1], ys[8, 0][:7])
