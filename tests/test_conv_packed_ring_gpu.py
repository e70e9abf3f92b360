"""The weight ring of the packed-rows 3x3 kernel (igemm3p_kernel RING, DCT_TUNE_IGEMM_PACKED_RING = knob 41): ONE halo stage and three
weight stages; the weight stage of round k + 2 is issued in round k behind a raw barrier and a counted vmcnt, the halo of the next
channel slice is re-staged in the open behind tap 8.

Every case runs with knob 41 = 1 and is compared
  * bit for bit with the same call under knob 41 = 0 -- today's loop on two halo and two weight stages, whose LDS images, reads and MFMA
    order it repeats --
  * and with F.conv2d in fp32 on the CPU, with the comparison and tolerance of test_kernels_gpu.test_conv2d_3x3_shared_halo.
The plan note (dct_debug_last_plan) of every launch is asserted to start with "igemm3p packed rows" and to name the ring exactly when
knob 41 is set, so that neither side silently runs another kernel.  The shapes are the smallest at which each mechanism can go wrong, far
below the planner's thresholds, so the tests also set knob 23 (fewest blocks of an unsplit packed-rows layer) and knob 24 (least fill of
its tiles) to 1, knob 1010 (fewest channel slices a block keeps; 4 in the shipped planner) to 1, and knob 1011 (channel-slice splits,
forced) where a case says so.  All are restored afterwards.
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
KNOB_PACKED_SPLIT, KNOB_PACKED_FILL, KNOB_RING, KNOB_MIN_SLICES, KNOB_SPLITS = 23, 24, 41, 1010, 1011
DEFAULTS = {KNOB_PACKED_SPLIT: 160, KNOB_PACKED_FILL: 50, KNOB_RING: 1, KNOB_MIN_SLICES: 4, KNOB_SPLITS: -1}      # csrc/igemm.hip
_RACE_LAUNCHES = 200 if os.environ.get("DCT_LONG_TESTS") else 50

# (B, Cin, H, W of the input, Cout, pad)
ONE_SLICE = (2, 64, 13, 13, 128, 0)        # 11 x 11 outputs, one slice: nine rounds, the prologue and the ring with no slice change
DEAD_WAVE = (2, 128, 11, 11, 128, 0)       # 9 x 9: 81 of 128 pixel slots, the fourth pixel wave is dead (stages, takes every barrier); one re-stage
DGRAD = (1, 192, 11, 13, 256, 2)           # data-gradient form, 13 x 15 outputs: halo lanes outside the image, two re-stages (every ring slot meets
                                           # a slice change), a ragged last tile (8 + 5 rows), two Cout tiles
SPLIT = (3, 256, 27, 27, 128, 0)           # 25 x 25, four slices: the split cases below
SPLIT5 = (3, 320, 27, 27, 128, 0)          # five slices: forced 2 -> blocks of 3 + 2 slices, forced 3 -> 2 + 2 + 1 (uneven; a one-slice block beside longer ones)
NINE = (1, 576, 11, 11, 128, 0)            # nine slices
# (shape, forced channel-slice splits or -1, splits the plan note must report)
CASES = [(ONE_SLICE, -1, 1), (DEAD_WAVE, -1, 1), (DGRAD, -1, 1),
         (SPLIT, 2, 2), (SPLIT, 3, 2),     # forced 3 of four slices is two slices per block: two blocks again (the planner has no 2 + 1 + 1)
         (SPLIT5, 2, 2), (SPLIT5, 3, 3),
         (NINE, -1, 1)]
EPILOGUE_SHAPES = [DEAD_WAVE, DGRAD]
RACE_CASES = [(DGRAD, -1), (SPLIT, 2)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _lib():
    from dct_amd import _lib
    return _lib.load()


@contextmanager
def ring(value, splits=-1):
    lib = _lib()
    try:
        for k, v in ((KNOB_PACKED_SPLIT, 1), (KNOB_PACKED_FILL, 1), (KNOB_MIN_SLICES, 1), (KNOB_SPLITS, splits), (KNOB_RING, value)):
            assert lib.dct_tune_set(k, v) == 0
        yield
    finally:
        for k, v in DEFAULTS.items():
            lib.dct_tune_set(k, v)


def _note():
    f = _lib().dct_debug_last_plan
    f.restype = ctypes.c_char_p
    return f().decode()


def _conv(ops, value, splits, *args, want_splits=None, **kw):
    """ops.conv2d under knob 41 = value; the launch must have been the packed-rows kernel in the loop form that value stands for"""
    with ring(value, splits):
        ops.conv2d(*args, **kw)
        note = _note()
    assert note.startswith("igemm3p packed rows"), (value, note)
    assert ("weight ring" in note) == bool(value), (value, note)
    if want_splits is not None:
        assert f" x {want_splits} channel-slice splits" in note, (want_splits, note)


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


@pytest.mark.parametrize("shape,splits,want_splits", CASES)
def test_ring_matches_two_stage_loop_and_cpu(ops, shape, splits, want_splits):
    """bias + ReLU; the split cases go through the fp32 slabs and splitk_epilogue_kernel"""
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    ys = {}
    for value in (1, 0):
        y = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        _conv(ops, value, splits, c["xd"], c["wd"], c["bd"], y, want_splits=want_splits, pad_h=pad, pad_w=pad, relu=True)
        ys[value] = y
    assert same(ys[1], ys[0]), "the weight ring differs from the two-stage loop"
    close(to_cpu(ys[1]), F.relu(c["plain"] + c["b"].view(1, -1, 1, 1)), "packed-rows ring conv fwd")


def _masked_accumulate(ops, c, shape, value, splits=-1, fill=None):
    """mask (ReLU gate of the destination, first 64 channels) + mask_scale + accumulate, x and y channel slices of wider buffers"""
    B, Cin, H, W, Cout, pad = shape
    yd = to_dev(c["old"]) if fill is None else torch.full((B, c["Ho"], c["Wo"], Cout + 64), fill, dtype=DT, device=DEV)
    _conv(ops, value, splits, c["xd"], c["wd"], None, yd[..., :Cout], pad_h=pad, pad_w=pad, mask=c["maskd"], mask_channels=64,
          mask_scale=2.0, accumulate=True)
    return yd


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES)
def test_ring_mask_accumulate_views(ops, shape):
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    got, want = _masked_accumulate(ops, c, shape, 1), _masked_accumulate(ops, c, shape, 0)
    assert same(got, want)
    masked = c["plain"].clone()
    masked[:, :64] = torch.where(c["maskt"][:, :64] > 0, c["plain"][:, :64] * 2.0, torch.zeros(()))
    ref = c["old"].clone()
    ref[:, :Cout] += masked
    close(to_cpu(got), ref, "packed-rows ring conv mask/accumulate/views")


@pytest.mark.parametrize("shape", EPILOGUE_SHAPES)
def test_ring_gate_bits(ops, shape):
    """mask_bits (the one-bit image of the mask) and relu_bits_out"""
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    mbits = _pack_bits(c["maskd"])
    outs = {}
    for value in (1, 0):
        plain = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        _conv(ops, value, -1, c["xd"], c["wd"], None, plain, pad_h=pad, pad_w=pad, mask=c["maskd"], mask_scale=2.0)
        gated = torch.full_like(plain, float("nan"))
        _conv(ops, value, -1, c["xd"], c["wd"], None, gated, pad_h=pad, pad_w=pad, mask=c["maskd"], mask_scale=2.0, mask_bits=mbits)
        y = torch.full_like(plain, float("nan"))
        bits = ops.relu_bits_like(y)
        bits.fill_(0xA5)
        _conv(ops, value, -1, c["xd"], c["wd"], c["bd"], y, pad_h=pad, pad_w=pad, relu=True, relu_bits_out=bits)
        outs[value] = (plain, gated, y, bits)
    for a, b in zip(outs[1], outs[0]):
        assert same(a, b)
    plain, gated, y, bits = outs[1]
    assert same(plain, gated) and torch.equal(bits, _pack_bits(y))
    assert 0.2 < (y > 0).float().mean().item() < 0.8
    masked = torch.where(c["maskt"] > 0, c["plain"] * 2.0, torch.zeros(()))
    close(to_cpu(gated), masked, "packed-rows ring conv mask_bits")


@pytest.mark.parametrize("shape,splits", RACE_CASES)
def test_ring_is_reproducible(ops, shape, splits):
    """The counted waits, the raw barriers and the re-stage of the single halo buffer are the new synchronisation: repeat launches of the
    three-slice data-gradient shape and of the split shape, with and without the mask / accumulate epilogue, into prefilled outputs (NaN;
    ones where the epilogue adds to them) must all equal the first, and the first the two-stage loop's."""
    B, Cin, H, W, Cout, pad = shape
    c = case(shape)
    y0 = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
    _conv(ops, 0, splits, c["xd"], c["wd"], c["bd"], y0, pad_h=pad, pad_w=pad, relu=True)
    z0 = _masked_accumulate(ops, c, shape, 0, splits, fill=1.0)
    assert torch.isfinite(y0.float()).all() and torch.isfinite(z0.float()).all()
    for _ in range(_RACE_LAUNCHES):
        y = torch.full((B, c["Ho"], c["Wo"], Cout), float("nan"), dtype=DT, device=DEV)
        _conv(ops, 1, splits, c["xd"], c["wd"], c["bd"], y, pad_h=pad, pad_w=pad, relu=True)
        z = _masked_accumulate(ops, c, shape, 1, splits, fill=1.0)
        assert same(y, y0) and same(z, z0)


def test_ring_knob_default_and_range():
    """Knob 41 takes 0 and 1 only; the shipped value is restored by every test above (DEFAULTS)."""
    lib = _lib()
    try:
        assert lib.dct_tune_set(KNOB_RING, 2) != 0 and lib.dct_tune_set(KNOB_RING, -1) != 0
        assert lib.dct_tune_set(KNOB_RING, 1) == 0
    finally:
        assert lib.dct_tune_set(KNOB_RING, DEFAULTS[KNOB_RING]) == 0
