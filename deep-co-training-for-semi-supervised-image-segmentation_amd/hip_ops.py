"""Functional wrappers over the C ABI (one per kernel family), operating on physical-NHWC
torch tensors that only provide device memory and the stream.  Used by the networks
(arch/), the loss modules, the optimizer and the parity tests.  HIP only."""
from __future__ import annotations

import ctypes as C
import threading
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import BF16, DTYPE_OF, F32, EnetTf, call, conv_desc, ptr, stream, view


# The open pass group / leaf side of THIS thread (the library keeps its recording state per thread too: csrc/enet.hip g_grp)
_tls = threading.local()


def _group():
    return getattr(_tls, "group", None)


_WS_CACHE = {}      # (device index, stream handle) -> uint8 workspace, grown geometrically


def _ws(nbytes: int, device) -> Optional[torch.Tensor]:
    """Scratch for one launch (split-K slabs, partial sums).  Eager launches reuse ONE buffer per stream -- launches of a
    stream run in order, so the next one may overwrite it -- instead of hitting the allocator per call.  Under stream
    capture the buffer comes from the graph's private pool as before: a cached buffer baked into a graph could be
    replaced (and freed) by a later, larger request while the graph still replays."""
    nbytes = max(int(nbytes), 16)
    if _group() is not None:        # recorded launches of different members run at the same time: scratch of their own, kept until then
        return keep(torch.empty(nbytes, dtype=torch.uint8, device=device))
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 2 * buf.numel() if buf is not None else 1 << 20), dtype=torch.uint8, device=dev)
        _WS_CACHE[key] = buf
    return buf


class PassGroup(object):
    """Records the Enet launches of ``members`` independent passes and issues them as one chain of grouped launches
    (include/dct.h "grouped passes").  Use::

        with K.PassGroup(n) as grp:
            for m in range(n):
                grp.member(m)
                ... plan_forward / plan_backward of pass m ...
        # leaving the block launches on the current stream

    Everything a member allocates while recording (`keep`) -- activations, scratch -- stays referenced until the launches
    are issued: the caching allocator would otherwise hand member m + 1 the blocks member m has already "freed" although
    none of m's kernels has run."""

    def __init__(self, members: int):
        self.n = int(members)
        self.kept: list = []
        self.grouped = self.single = 0

    def __enter__(self):
        assert _group() is None, "pass groups do not nest"
        call("dct_group_begin", self.n)
        _tls.group = self
        _lib.set_group_open(True)
        return self

    def member(self, m: int) -> None:
        call("dct_group_member", int(m))

    def __exit__(self, et, ev, tb):
        _tls.group = None
        _lib.set_group_open(False)
        if et is not None:
            _lib.load().dct_group_abort()
            self.kept.clear()
            return False
        g, s = C.c_int(0), C.c_int(0)
        call("dct_group_end", stream(), C.byref(g), C.byref(s))
        self.grouped, self.single = g.value, s.value
        self.kept.clear()
        return False


class LeafSide(object):
    """Holds back the weight- and bias-gradient launches of a backward pass (the leaves of its data-gradient chain) so that
    they can be issued on ANOTHER queue (include/dct.h dct_leaves_*)::

        with K.LeafSide() as side:
            net.plan_backward(..., leaf_hook=hook)     # hook(): event on the chain's stream; side stream waits; side.flush() there
        keep = side.kept                                # stays referenced until the side stream has been joined

    ``flush`` issues what is held so far on the CURRENT stream.  Leaving the block issues any rest on the current stream."""

    def __init__(self):
        self.kept: list = []
        self.launches = 0

    def __enter__(self):
        assert _group() is None, "pass groups / leaf sides do not nest"
        call("dct_leaves_begin")
        _tls.group = self
        return self

    def flush(self) -> None:
        n = C.c_int(0)
        call("dct_leaves_flush", stream(), C.byref(n))
        self.launches += n.value

    def __exit__(self, et, ev, tb):
        _tls.group = None
        if et is not None:
            _lib.load().dct_group_abort()
            return False
        n = C.c_int(0)
        call("dct_leaves_end", stream(), C.byref(n))
        self.launches += n.value
        return False



def keep(t):
    """Tensor ``t`` (allocated by a pass that may be recording into a PassGroup) -> t, referenced until the group launches."""
    if _group() is not None:
        _group().kept.append(t)
    return t


def group_max() -> int:
    return int(_lib.load().dct_group_max())


def _dt(t: torch.Tensor) -> int:
    try:
        return DTYPE_OF[t.dtype]
    except KeyError:
        raise RuntimeError(f"dct_amd: unsupported dtype {t.dtype}")


# ------------------------------------------------------------------------------ conv family
def relu_bits_like(t: torch.Tensor):
    """Buffer for the ReLU-gate bits of a dense bf16 NHWC tensor (one bit per element), or None where bits do not apply."""
    if t.dtype != torch.bfloat16 or t.shape[3] % 8 or not t.is_contiguous():
        return None
    return torch.empty(t.shape[0], t.shape[1], t.shape[2], t.shape[3] // 8, dtype=torch.uint8, device=t.device)


def _bits_ok(bits, of):
    if bits is None:
        return None
    assert of is not None and bits.dtype == torch.uint8 and bits.is_contiguous() and of.is_contiguous()
    assert tuple(bits.shape) == (of.shape[0], of.shape[1], of.shape[2], of.shape[3] // 8), (bits.shape, of.shape)
    return bits


class StemFusionUnsupported(RuntimeError):
    """conv2d(..., stem=...) on a layer whose kernel cannot take the stem's weight gradient along (the caller runs the two launches instead)."""


def conv2d(x, w_packed, bias, y, *, R=3, S=3, stride=1, dil=1, pad_h=0, pad_w=0, relu=False, mask=None,
           mask_channels=0, mask_scale=1.0, accumulate=False, scatter2x2=False, mask_bits=None, relu_bits_out=None,
           pool_out=None, pool_codes=None, pool_only=False, stem=None):
    """y (NHWC view, written in place) = epilogue(conv(x, w_packed)); see include/dct.h dct_conv2d.

    ``relu_bits_out`` (uint8 [N,H,W,C/8], dense y): the launch also leaves the ReLU-gate bits of y there (`relu_bits_like`);
    ``mask_bits``: such bits of ``mask`` -- the data gradient then reads 1/16 of the bytes where its epilogue can.
    ``pool_out`` (dense [N,(H+1)//2,(W+1)//2,C], y's dtype) / ``pool_codes`` (uint8, same shape): the 2x2 ceil-mode max pooling of y
    (and its routing codes) in the same call -- `maxpool_fwd(y, pool_out, codes=pool_codes)` bit for bit; ``pool_only``: the caller
    reads the pooled tensor alone -- y may be left unwritten.
    ``stem`` = (x, dw, db, accumulate): the UNet stem's weight / bias gradient from this data gradient's output tile (dct_conv_desc.stem_*);
    y is then NOT written.  Raises ``StemFusionUnsupported`` when the layer does not take the kernel that can."""
    if pool_out is not None:
        want = (y.shape[0], (y.shape[1] + 1) // 2, (y.shape[2] + 1) // 2, y.shape[3])
        assert tuple(pool_out.shape) == want and pool_out.is_contiguous() and pool_out.dtype == y.dtype, "pool_out: dense ceil-mode half of y"
        assert pool_codes is None or (pool_codes.dtype == torch.uint8 and pool_codes.is_contiguous() and tuple(pool_codes.shape) == want)
        assert not accumulate and not scatter2x2 and mask is None and mask_bits is None, "pool_out is a forward-pass feature"
    else:
        assert pool_codes is None and not pool_only
    d = conv_desc(R, S, stride, dil, pad_h, pad_w, relu, scatter2x2, accumulate, mask_channels, mask_scale,
                  _bits_ok(mask_bits, mask), _bits_ok(relu_bits_out, y), pool_out, pool_codes, pool_only, stem)
    if stem is not None:
        sx, sdw, sdb, _ = stem
        assert sx.dtype == torch.float32 and sx.is_contiguous() and sx.numel() == y.shape[0] * (y.shape[1] + 2) * (y.shape[2] + 2)
        assert sdw.dtype == torch.float32 and sdw.numel() == 64 * 9 and sdb.dtype == torch.float32 and sdb.numel() == 64
    vx, vy = view(x), view(y)
    lib = _lib.load()
    dt = _dt(x)
    need = lib.dct_conv2d_workspace_bytes(C.byref(vx), C.byref(vy), C.byref(d), dt)
    ws = _ws(need, x.device)
    vm = view(mask) if mask is not None else None
    rc = lib.dct_conv2d(C.byref(vx), ptr(w_packed), ptr(bias), C.byref(vm) if vm is not None else None,
                        C.byref(vy), C.byref(d), dt, ptr(ws), ws.numel(), stream())
    if stem is not None and rc == _lib.ERR_UNSUPPORTED:
        raise StemFusionUnsupported()
    _lib.check(rc, "dct_conv2d")
    return y


def conv2d_wgrad(p, q, dw, *, R=3, S=3, stride=1, dil=1, pad_h=0, pad_w=0, accumulate=False, db=None):
    """dw[p.c][R][S][q.c] (fp32, dense) (+)= sum_m p[m] (x) q[shifted m]; with ``db`` (bf16 only) also
    db[p.c] (+)= sum_m p[m] in the same launch."""
    d = conv_desc(R, S, stride, dil, pad_h, pad_w, accumulate=accumulate)
    vp, vq = view(p), view(q)
    lib = _lib.load()
    dt = _dt(p)
    need = lib.dct_conv2d_wgrad_workspace_bytes(C.byref(vp), C.byref(vq), C.byref(d), dt)
    if need == 0:
        raise RuntimeError("dct_amd: conv2d_wgrad unsupported shape")
    ws = _ws(need, p.device)
    name = "dct_conv2d_wgrad_bias" if db is not None else "dct_conv2d_wgrad"
    args = (C.byref(vp), C.byref(vq), ptr(dw)) + ((ptr(db),) if db is not None else ()) + (C.byref(d), dt, ptr(ws), ws.numel(), stream())
    call(name, *args)
    return dw


def bias_grad(dy, db, accumulate=False):
    vd = view(dy)
    need = _lib.load().dct_bias_grad_workspace_bytes(C.byref(vd))
    ws = _ws(need, dy.device)
    call("dct_bias_grad", C.byref(vd), ptr(db), int(accumulate), _dt(dy), ptr(ws), ws.numel(), stream())
    return db


def bias_grad_batched(dys, dbs, accumulate=False):
    """db_k (+)= column sums of dy_k for up to eight (dy, db) pairs of one dtype in ONE launch pair (dct_bias_grad_batched)."""
    n = len(dys)
    if n == 1:
        return bias_grad(dys[0], dbs[0], accumulate)
    assert 1 < n <= 8 and len(dbs) == n and all(d.dtype == dys[0].dtype for d in dys)
    views = (_lib.View * n)(*[view(d) for d in dys])
    ptrs = (C.c_void_p * n)(*[int(b.data_ptr()) for b in dbs])
    need = _lib.load().dct_bias_grad_batched_workspace_bytes(views, n)
    ws = _ws(need, dys[0].device)
    call("dct_bias_grad_batched", views, ptrs, n, int(accumulate), _dt(dys[0]), ptr(ws), ws.numel(), stream())


def pack_weight(src_f32, dst, P, T, Q, transpose=False, flip_taps=False):
    call("dct_pack_weight", ptr(src_f32), ptr(dst), P, T, Q, int(transpose), int(flip_taps), _dt(dst), stream())
    return dst


def pack_jobs_table(jobs, device):
    """Device table for pack_weights_batched.  jobs: list of (src fp32 or bf16 tensor, dst tensor, P, T, Q, mode, flip) with
    mode 1 -> dst[Q][T'][P], mode 2 -> dst[T'][Q][P] (dct_pack_weight's transpose codes).  Returns (table, n, tiles, edge):
    edge 64 when every job is 16-bit -> 16-bit with P, Q multiples of 64 (the vectorised kernel), else 32."""
    import struct
    wide = all(src.dtype == dst.dtype and src.element_size() == 2 and P % 64 == 0 and Q % 64 == 0 and
               src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 for src, dst, P, T, Q, mode, flip in jobs)
    edge = 64 if wide else 32
    buf, tiles = bytearray(), 0
    for src, dst, P, T, Q, mode, flip in jobs:
        assert P % 32 == 0 and Q % 32 == 0 and mode in (1, 2)
        dq, dt = (T * P, P) if mode == 1 else (P, Q * P)
        assert src.dtype in (torch.float32, torch.bfloat16)
        buf += struct.pack("<QQiiiiqqii", src.data_ptr(), dst.data_ptr(), P, T, Q, int(bool(flip)), dq, dt, tiles,
                           int(src.dtype == torch.bfloat16))
        tiles += (P // edge) * (Q // edge) * T
    table = torch.frombuffer(buf, dtype=torch.uint8).clone().to(device)
    return table, len(jobs), tiles, edge


def pack_weights_batched(table, njobs, tiles, dtype, edge=32):
    if edge == 64:
        call("dct_pack_weights_batched64", ptr(table), int(njobs), int(tiles), stream())
    else:
        call("dct_pack_weights_batched", ptr(table), int(njobs), int(tiles), DTYPE_OF[dtype], stream())


def bn_running_table(layers, device):
    """Device record table for bn_running_update.  layers: list of (running_mean, running_var, num_batches_tracked or None, c,
    mean_off, var_off) -- offsets in elements into the flat statistics buffer of a forward pass."""
    import struct
    buf = bytearray()
    for rm, rv, nbt, c, moff, voff in layers:
        assert rm.dtype == torch.float32 and rv.dtype == torch.float32 and rm.is_contiguous() and rv.is_contiguous()
        assert nbt is None or nbt.dtype == torch.int64
        buf += struct.pack("<QQQiiii", rm.data_ptr(), rv.data_ptr(), nbt.data_ptr() if nbt is not None else 0, int(c), int(moff), int(voff), 0)
    return torch.frombuffer(buf, dtype=torch.uint8).clone().to(device)


def bn_running_update(table, n_layers, stats, momentum):
    call("dct_bn_running_update", ptr(table), int(n_layers), ptr(stats), float(momentum), stream())


def flat_sum(out, a, b, c=None):
    """out = a + b (+ c): flat fp32 buffers of equal length (multiple of 4 elements)."""
    call("dct_flat_sum", ptr(out), ptr(a), ptr(b), ptr(c), out.numel(), stream())
    return out


def flat_scale(x, scale):
    """x *= scale in place: a dense fp32 buffer (or slice of one) of any length."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    if x.numel():
        call("dct_flat_scale", ptr(x), float(scale), x.numel(), stream())
    return x


def conv_cin1_fwd(x, w, bias, y, *, R=3, S=3, stride=1, dil=1, pad_h=0, pad_w=0, relu=False, relu_bits_out=None):
    d = conv_desc(R, S, stride, dil, pad_h, pad_w, relu, relu_bits_out=_bits_ok(relu_bits_out, y))
    vx, vy = view(x), view(y)
    call("dct_conv_cin1_fwd", C.byref(vx), ptr(w), ptr(bias), C.byref(vy), C.byref(d), _dt(y), stream())
    return y


def conv_cin1_dgrad(dy, w, dx, *, R=3, S=3, stride=1, dil=1, pad_h=0, pad_w=0):
    d = conv_desc(R, S, stride, dil, pad_h, pad_w)
    vdy, vdx = view(dy), view(dx)
    call("dct_conv_cin1_dgrad", C.byref(vdy), ptr(w), C.byref(vdx), C.byref(d), _dt(dy), stream())
    return dx


def conv_cin1_wgrad(x, dy, dw, db, *, R=3, S=3, stride=1, dil=1, pad_h=0, pad_w=0, accumulate=False):
    d = conv_desc(R, S, stride, dil, pad_h, pad_w)
    vx, vdy = view(x), view(dy)
    need = _lib.load().dct_conv_cin1_wgrad_workspace_bytes(C.byref(vdy), C.byref(d))
    ws = _ws(need, x.device)
    call("dct_conv_cin1_wgrad", C.byref(vx), C.byref(vdy), ptr(dw), ptr(db), C.byref(d), int(accumulate), _dt(dy),
         ptr(ws), ws.numel(), stream())


def head_fwd(x, w, bias, y):
    vx, vy = view(x), view(y)
    call("dct_conv1x1_head_fwd", C.byref(vx), ptr(w), ptr(bias), C.byref(vy), _dt(x), stream())
    return y


def head_bwd(x, dy, w, dx, dw, db, relu_mask=True, accumulate=False):
    vx, vdy = view(x), view(dy)
    vdx = view(dx) if dx is not None else None
    need = _lib.load().dct_conv1x1_head_bwd_workspace_bytes(C.byref(vx), dy.shape[3])
    ws = _ws(need, x.device)
    call("dct_conv1x1_head_bwd", C.byref(vx), C.byref(vdy), ptr(w), C.byref(vdx) if vdx is not None else None,
         ptr(dw), ptr(db), int(relu_mask), int(accumulate), _dt(x), ptr(ws), ws.numel(), stream())


# ------------------------------------------------------------------------------ pointwise
def maxpool_fwd(x, y, codes=None):
    """``codes`` (uint8, dense, y's shape): also keep the routing decision (window position of the first maximum + its ReLU
    gate) for `maxpool_bwd(codes=...)`, which then does not re-read x."""
    vx, vy = view(x), view(y)
    if codes is not None:
        assert codes.dtype == torch.uint8 and codes.is_contiguous() and tuple(codes.shape) == tuple(y.shape)
        call("dct_maxpool2x2_fwd_codes", C.byref(vx), C.byref(vy), ptr(codes), _dt(x), stream())
    else:
        call("dct_maxpool2x2_fwd", C.byref(vx), C.byref(vy), _dt(x), stream())
    return y


def maxpool_bwd(x, dy, dx, relu_mask=False, scale=1.0, codes=None, skip=None):
    """``skip`` (with codes): the gradient at a bilinearly resized copy of the pooled tensor; its bilinear backward is added to dy on the way."""
    vdy, vdx = view(dy), view(dx)
    if codes is not None and skip is not None:
        assert codes.dtype == torch.uint8 and codes.is_contiguous() and tuple(codes.shape) == tuple(dy.shape)
        vs = view(skip)
        rc = _lib.load().dct_maxpool2x2_bwd_codes_skip(ptr(codes), C.byref(vdy), C.byref(vs), C.byref(vdx), int(relu_mask), float(scale),
                                                       _dt(dy), stream())
        if rc == _lib.ERR_UNSUPPORTED:
            # views the 16-byte kernel cannot take (channel counts / slice offsets off the vector width): the sum formed in memory,
            # as before the fusion -- bilinear backward (which has a scalar form) accumulating onto a copy of dy (the sum formed in fp32 and
            # rounded to the storage type once), then the plain un-pooling, which has a scalar form too
            total = bilinear_bwd(skip, dy.clone(), accumulate=True)
            vt = view(total)
            call("dct_maxpool2x2_bwd_codes", ptr(codes), C.byref(vt), C.byref(vdx), int(relu_mask), float(scale), _dt(dy), stream())
            return dx
        _lib.check(rc, "dct_maxpool2x2_bwd_codes_skip")
        return dx
    assert skip is None
    if codes is not None:
        assert codes.dtype == torch.uint8 and codes.is_contiguous() and tuple(codes.shape) == tuple(dy.shape)
        call("dct_maxpool2x2_bwd_codes", ptr(codes), C.byref(vdy), C.byref(vdx), int(relu_mask), float(scale), _dt(dy), stream())
        return dx
    vx = view(x)
    call("dct_maxpool2x2_bwd", C.byref(vx), C.byref(vdy), C.byref(vdx), int(relu_mask), float(scale), _dt(x), stream())
    return dx


def bilinear_fwd(x, y):
    vx, vy = view(x), view(y)
    call("dct_bilinear_fwd", C.byref(vx), C.byref(vy), _dt(x), _dt(y), stream())
    return y


def bilinear_fwd_batched(xs, ys):
    """ys[k] = bilinear_fwd(xs[k]) for up to eight pairs of one dtype in ONE launch (dct_bilinear_fwd_batched); views off the 16-byte vector width
    fall back to one launch per tensor."""
    n = len(xs)
    assert n == len(ys) and 1 <= n <= 8 and all(_dt(x) == _dt(xs[0]) == _dt(y) for x, y in zip(xs, ys))
    vx = (_lib.View * n)(*[view(x) for x in xs])
    vy = (_lib.View * n)(*[view(y) for y in ys])
    rc = _lib.load().dct_bilinear_fwd_batched(vx, vy, n, _dt(xs[0]), stream())
    if rc == _lib.ERR_UNSUPPORTED:
        for x, y in zip(xs, ys):
            bilinear_fwd(x, y)
        return ys
    _lib.check(rc, "dct_bilinear_fwd_batched")
    return ys


def bilinear_bwd(dy, dx, accumulate=False):
    vdy, vdx = view(dy), view(dx)
    call("dct_bilinear_bwd", C.byref(vdy), C.byref(vdx), _dt(dy), _dt(dx), int(accumulate), stream())
    return dx


def dropout_fwd(x, y, p, seed, offset, mask_out=None, calls_dev=None, parity=0):
    """``calls_dev`` (int64[2] device tensor): the call counter lives on the device -- the launch reads word ``parity``, is call number that + 1
    (offset = number << 40; ``offset`` is ignored) and stores the number to the other word; the caller alternates ``parity`` from call to call.
    The graph-replayable form."""
    vx, vy = view(x), view(y)
    if calls_dev is not None:
        assert calls_dev.dtype == torch.int64 and calls_dev.numel() >= 2
        call("dct_dropout_fwd_dev", C.byref(vx), C.byref(vy), ptr(mask_out), float(p), int(seed), ptr(calls_dev), int(parity), _dt(x), stream())
        return y
    call("dct_dropout_fwd", C.byref(vx), C.byref(vy), ptr(mask_out), float(p), int(seed), int(offset), _dt(x), stream())
    return y


def dropout_maxpool_fwd(x, y, codes, p, seed, calls_dev, parity):
    """y, codes = maxpool_fwd(dropout_fwd(x, calls_dev=..., parity=...), codes=...) in one pass, without the dropped tensor
    (dct_dropout_maxpool2x2_fwd_codes; bit for bit the two launches)."""
    assert calls_dev.dtype == torch.int64 and calls_dev.numel() >= 2
    assert codes.dtype == torch.uint8 and codes.is_contiguous() and tuple(codes.shape) == tuple(y.shape)
    vx, vy = view(x), view(y)
    call("dct_dropout_maxpool2x2_fwd_codes", C.byref(vx), C.byref(vy), ptr(codes), float(p), int(seed), ptr(calls_dev), int(parity), _dt(x), stream())
    return y


def dropout_apply(x, y, mask_u8, p):
    vx, vy = view(x), view(y)
    call("dct_dropout_apply", C.byref(vx), C.byref(vy), ptr(mask_u8), float(p), _dt(x), stream())
    return y


def relu_bwd(g, a, y, scale=1.0):
    vg, va, vy = view(g), view(a), view(y)
    call("dct_relu_bwd", C.byref(vg), C.byref(va), C.byref(vy), float(scale), _dt(g), stream())
    return y


def cast(x, y):
    vx, vy = view(x), view(y)
    call("dct_cast", C.byref(vx), C.byref(vy), _dt(x), _dt(y), stream())
    return y


# ------------------------------------------------------------------------------ losses etc.
def _loss_ws(device):
    return torch.empty(_lib.load().dct_loss_workspace_bytes(0), dtype=torch.uint8, device=device)


def _ptr_array(ts: Sequence[torch.Tensor]):
    arr = (C.c_void_p * len(ts))(*[ptr(t) for t in ts])
    return arr


def ce_fwd(logits_pc, targets, C_, ignore_index=255):
    """logits_pc: fp32 [P, C] dense; targets int64 [P].  Returns device tensor [2] = (mean loss, count)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_ce_fwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(out),
         ptr(ws), ws.numel(), stream())
    return out


def ce_bwd(logits_pc, targets, C_, count, dlogits, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    call("dct_ce_bwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(count),
         ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), stream())
    return dlogits


def ce_step(logits_pc, targets, C_, dlogits, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """ce_fwd + ce_bwd of the same logits in two launches instead of three (dct_ce_step; bit for bit the two calls).  Returns the device
    tensor [2] = (mean loss, count); ``dlogits`` is written (added to)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_ce_step", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(out), ptr(gscale), float(gmul),
         ptr(dlogits), int(accumulate), ptr(ws), ws.numel(), stream())
    return out


CE_MEAN, CE_SUM = 0, 1      # the ``reduction`` argument of dct_ce_weighted_*


def ce_weighted_fwd(logits_pc, targets, C_, weight=None, reduction=CE_MEAN, ignore_index=255):
    """``weight``: fp32 [C] on the device, or None (all ones).  Returns the device tensor [2] = (sum w l / sum w | sum w l, sum w)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_ce_weighted_fwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), int(reduction),
         ptr(out), ptr(ws), ws.numel(), stream())
    return out


def ce_weighted_bwd(logits_pc, targets, C_, denom, dlogits, weight=None, reduction=CE_MEAN, gscale=None, gmul=1.0, ignore_index=255,
                    accumulate=False):
    """``denom``: ``out[1:2]`` of ce_weighted_fwd (not read under CE_SUM, where it may be None)."""
    call("dct_ce_weighted_bwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), int(reduction),
         ptr(denom), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), stream())
    return dlogits


def ce_weighted_step(logits_pc, targets, C_, dlogits, weight=None, reduction=CE_MEAN, gscale=None, gmul=1.0, ignore_index=255,
                     accumulate=False):
    """ce_weighted_fwd + ce_weighted_bwd of the same logits in two launches (dct_ce_weighted_step; bit for bit the two calls).  Returns the
    device tensor [2]; ``dlogits`` is written (added to)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_ce_weighted_step", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), int(reduction),
         ptr(out), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), ptr(ws), ws.numel(), stream())
    return out


def ce_map_fwd(logits_pc, targets, C_, weight=None, ignore_index=255):
    """-> fp32 [P]: w_t * (logsumexp(x) - x_t) per pixel, 0 where the target is ignored."""
    m = torch.empty(logits_pc.numel() // C_, dtype=torch.float32, device=logits_pc.device)
    call("dct_ce_map_fwd", ptr(logits_pc), ptr(targets), m.numel(), C_, int(ignore_index), ptr(weight), ptr(m), stream())
    return m


def ce_map_bwd(logits_pc, targets, C_, dmap, dlogits, weight=None, gmul=1.0, ignore_index=255, accumulate=False):
    call("dct_ce_map_bwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), ptr(dmap), float(gmul),
         ptr(dlogits), int(accumulate), stream())
    return dlogits


def focal_fwd(logits_pc, targets, C_, weight=None, gamma=2.0, reduction=CE_MEAN, ignore_index=255):
    """Focal loss (dct_focal_fwd): ``weight``: fp32 [C] on the device, or None (all ones); ``gamma``: a host float, finite and >= 0.
    Returns the device tensor [2] = (sum f / sum w | sum f, sum w) with f = w_t (1 - p_t)^gamma (-log p_t)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_focal_fwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), float(gamma),
         int(reduction), ptr(out), ptr(ws), ws.numel(), stream())
    return out


def focal_bwd(logits_pc, targets, C_, denom, dlogits, weight=None, gamma=2.0, reduction=CE_MEAN, gscale=None, gmul=1.0, ignore_index=255,
              accumulate=False):
    """``denom``: ``out[1:2]`` of focal_fwd (not read under CE_SUM, where it may be None)."""
    call("dct_focal_bwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), float(gamma),
         int(reduction), ptr(denom), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), stream())
    return dlogits


def focal_step(logits_pc, targets, C_, dlogits, weight=None, gamma=2.0, reduction=CE_MEAN, gscale=None, gmul=1.0, ignore_index=255,
               accumulate=False):
    """focal_fwd + focal_bwd of the same logits in two launches (dct_focal_step; bit for bit the two calls).  Returns the device tensor
    [2]; ``dlogits`` is written (added to)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_focal_step", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), float(gamma),
         int(reduction), ptr(out), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), ptr(ws), ws.numel(), stream())
    return out


def focal_map_fwd(logits_pc, targets, C_, weight=None, gamma=2.0, ignore_index=255):
    """-> fp32 [P]: w_t (1 - p_t)^gamma (-log p_t) per pixel, 0 where the target is ignored."""
    m = torch.empty(logits_pc.numel() // C_, dtype=torch.float32, device=logits_pc.device)
    call("dct_focal_map_fwd", ptr(logits_pc), ptr(targets), m.numel(), C_, int(ignore_index), ptr(weight), float(gamma), ptr(m), stream())
    return m


def focal_map_bwd(logits_pc, targets, C_, dmap, dlogits, weight=None, gamma=2.0, gmul=1.0, ignore_index=255, accumulate=False):
    call("dct_focal_map_bwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), float(gamma),
         ptr(dmap), float(gmul), ptr(dlogits), int(accumulate), stream())
    return dlogits


def _topk_ce_bufs(P, device):
    """(out2, counts4, vmap, workspace) of one dct_topk_ce_* call: fresh tensors, so that a captured graph owns them."""
    return (torch.empty(2, dtype=torch.float32, device=device), torch.empty(4, dtype=torch.int64, device=device),
            torch.empty(P, dtype=torch.float32, device=device),
            torch.empty(_lib.load().dct_topk_ce_workspace_bytes(P), dtype=torch.uint8, device=device))


def topk_ce_fwd(logits_pc, targets, C_, weight=None, k_percent=10.0, ignore_index=255):
    """Top-k cross entropy (dct_topk_ce_fwd; the rule: include/dct.h): the mean of w_t l over the hardest ``k_percent`` % of the counted
    pixels.  ``weight``: fp32 [C] on the device, or None (all ones); ``k_percent``: a host float, 0 < k <= 100.  Returns the device
    tensors ``out2`` = (value, tau), ``counts4`` = int64 (K, N, n_gt, n_eq) and ``vmap`` [P], the stored map the selection compared."""
    P = logits_pc.numel() // C_
    out2, counts4, vmap, ws = _topk_ce_bufs(P, logits_pc.device)
    call("dct_topk_ce_fwd", ptr(logits_pc), ptr(targets), P, C_, int(ignore_index), ptr(weight), float(k_percent), ptr(out2), ptr(counts4),
         ptr(vmap), ptr(ws), ws.numel(), stream())
    return out2, counts4, vmap


def topk_ce_bwd(logits_pc, targets, C_, vmap, out2, counts4, dlogits, weight=None, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """``vmap``, ``out2`` and ``counts4``: those of topk_ce_fwd under the same arguments."""
    call("dct_topk_ce_bwd", ptr(logits_pc), ptr(targets), logits_pc.numel() // C_, C_, int(ignore_index), ptr(weight), ptr(vmap), ptr(out2),
         ptr(counts4), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), stream())
    return dlogits


def topk_ce_step(logits_pc, targets, C_, dlogits, weight=None, k_percent=10.0, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """topk_ce_fwd + topk_ce_bwd of the same logits (dct_topk_ce_step; bit for bit the two calls).  Returns (out2, counts4, vmap);
    ``dlogits`` is written (added to)."""
    P = logits_pc.numel() // C_
    out2, counts4, vmap, ws = _topk_ce_bufs(P, logits_pc.device)
    call("dct_topk_ce_step", ptr(logits_pc), ptr(targets), P, C_, int(ignore_index), ptr(weight), float(k_percent), ptr(out2), ptr(counts4),
         ptr(vmap), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), ptr(ws), ws.numel(), stream())
    return out2, counts4, vmap


def _i64_dense(t):
    """int64, contiguous and on the 16-byte grid (a dense view that starts inside its storage gets a copy of its own)."""
    if t.dtype != torch.int64 or not t.is_contiguous():
        t = t.to(torch.int64).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def signed_distance(targets_bhw, C_, classes=None, spacing=(1., 1.)):
    """targets [B, H, W] (int64 made if needed), spacing (sy, sx) -> fp32 [B, H, W, C]: the signed distance of every pixel to the contour
    of every class in ``classes`` (None: all), negative inside, 0 for a class that is absent from its image, fills it or is not in
    ``classes`` (dct_signed_distance; the rule: include/dct.h).  Every element is written."""
    ptr(targets_bhw)                    # (refuses a CPU tensor before anything is sized or copied)
    B, H, W = targets_bhw.shape
    mask = (1 << C_) - 1 if classes is None else sum(1 << int(c) for c in set(classes))
    sy, sx = (float(s) for s in spacing)
    t = _i64_dense(targets_bhw)
    need = _lib.load().dct_signed_distance_workspace_bytes(B, H, W, C_)
    ws = _ws(need, t.device)
    phi = torch.empty(B, H, W, C_, dtype=torch.float32, device=t.device)
    call("dct_signed_distance", ptr(t), B, H, W, C_, mask, sy, sx, ptr(phi), ptr(ws), ws.numel(), stream())
    return phi


def boundary_fwd(logits_pc, targets, phi, C_, class_mask=None, ignore_index=255):
    """Boundary loss (dct_boundary_fwd).  ``logits_pc`` and ``phi``: fp32 [..., C] dense, one row per pixel; ``targets``: int64, one per
    pixel; ``class_mask``: bit c = class c is in the loss (None: all).  Returns the device tensor [2] = (loss, counted pixels)."""
    out = torch.empty(2, dtype=torch.float32, device=logits_pc.device)
    ws = _loss_ws(logits_pc.device)
    call("dct_boundary_fwd", ptr(logits_pc), ptr(targets), ptr(phi), logits_pc.numel() // C_, C_, int(ignore_index),
         (1 << C_) - 1 if class_mask is None else int(class_mask), ptr(out), ptr(ws), ws.numel(), stream())
    return out


def boundary_bwd(logits_pc, targets, phi, C_, count, dlogits, class_mask=None, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """``count``: ``out[1:2]`` of boundary_fwd under the same arguments."""
    call("dct_boundary_bwd", ptr(logits_pc), ptr(targets), ptr(phi), logits_pc.numel() // C_, C_, int(ignore_index),
         (1 << C_) - 1 if class_mask is None else int(class_mask), ptr(count), ptr(gscale), float(gmul), ptr(dlogits), int(accumulate), stream())
    return dlogits


# The overlap criteria (dct_ce_dice_*, dct_ce_tversky_*): one argument list, in which a family's own parameters (``rule``: none for Dice;
# alpha, beta, gamma for Tversky) stand between ``smooth`` and ``per_image``.
def _overlap_args(logits_bpc, C_, class_mask, per_image):
    """(B, pixels per image, mask, G) of fp32 logits [B, ..., C] (dense; the first dimension counts the images)."""
    B = logits_bpc.shape[0]
    return B, logits_bpc.numel() // (B * C_), (1 << C_) - 1 if class_mask is None else int(class_mask), B if per_image else 1


def _overlap_ws(B, C_, per_image, device):
    return torch.empty(_lib.load().dct_ce_dice_workspace_bytes(B, C_, int(per_image)), dtype=torch.uint8, device=device)


def _overlap_outputs(G, C_, device):
    """(out4, index_gc [G, C], sums [G, C, 3])"""
    return (torch.empty(4, dtype=torch.float32, device=device), torch.empty(G, C_, dtype=torch.float32, device=device),
            torch.empty(G, C_, 3, dtype=torch.float32, device=device))


def _overlap_fwd(family, rule, logits_bpc, targets, C_, weight, class_mask, smooth, per_image, ce_coef, coef, ignore_index):
    B, ppi, mask, G = _overlap_args(logits_bpc, C_, class_mask, per_image)
    out4, index_gc, sums = _overlap_outputs(G, C_, logits_bpc.device)
    ws = _overlap_ws(B, C_, per_image, logits_bpc.device)
    call(f"dct_ce_{family}_fwd", ptr(logits_bpc), ptr(targets), B, ppi, C_, int(ignore_index), ptr(weight), mask, float(smooth),
         *(float(v) for v in rule), int(per_image), float(ce_coef), float(coef), ptr(out4), ptr(index_gc), ptr(sums), ptr(ws), ws.numel(), stream())
    return out4, index_gc, sums


def _overlap_bwd(family, rule, logits_bpc, targets, C_, out4, sums, dlogits, weight, class_mask, smooth, per_image, ce_coef, coef, gscale, gmul,
                 ignore_index, accumulate):
    B, ppi, mask, _ = _overlap_args(logits_bpc, C_, class_mask, per_image)
    call(f"dct_ce_{family}_bwd", ptr(logits_bpc), ptr(targets), B, ppi, C_, int(ignore_index), ptr(weight), mask, float(smooth),
         *(float(v) for v in rule), int(per_image), float(ce_coef), float(coef), ptr(out4), ptr(sums), ptr(gscale), float(gmul), ptr(dlogits),
         int(accumulate), stream())
    return dlogits


def _overlap_step(family, rule, logits_bpc, targets, C_, dlogits, weight, class_mask, smooth, per_image, ce_coef, coef, gscale, gmul,
                  ignore_index, accumulate):
    B, ppi, mask, G = _overlap_args(logits_bpc, C_, class_mask, per_image)
    out4, index_gc, sums = _overlap_outputs(G, C_, logits_bpc.device)
    ws = _overlap_ws(B, C_, per_image, logits_bpc.device)
    call(f"dct_ce_{family}_step", ptr(logits_bpc), ptr(targets), B, ppi, C_, int(ignore_index), ptr(weight), mask, float(smooth),
         *(float(v) for v in rule), int(per_image), float(ce_coef), float(coef), ptr(out4), ptr(index_gc), ptr(sums), ptr(gscale), float(gmul),
         ptr(dlogits), int(accumulate), ptr(ws), ws.numel(), stream())
    return out4, index_gc, sums


def ce_dice_fwd(logits_bpc, targets, C_, weight=None, class_mask=None, smooth=1e-5, per_image=False, ce_coef=1.0, dice_coef=1.0,
                ignore_index=255):
    """Soft Dice / CE + Dice (dct_ce_dice_fwd; the rule: include/dct.h).  ``logits_bpc``: fp32 [B, ..., C] dense; ``targets``: int64, one per
    pixel; ``class_mask``: bit c = class c is in the Dice mean (None: all).  Returns device tensors ``out4`` = (total, ce, sum w, dice),
    ``dice_gc`` [G, C] and ``sums`` [G, C, 3] (G = B under ``per_image``, else 1)."""
    return _overlap_fwd("dice", (), logits_bpc, targets, C_, weight, class_mask, smooth, per_image, ce_coef, dice_coef, ignore_index)


def ce_dice_bwd(logits_bpc, targets, C_, out4, sums, dlogits, weight=None, class_mask=None, smooth=1e-5, per_image=False, ce_coef=1.0,
                dice_coef=1.0, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """``out4`` and ``sums``: those of ce_dice_fwd under the same arguments."""
    return _overlap_bwd("dice", (), logits_bpc, targets, C_, out4, sums, dlogits, weight, class_mask, smooth, per_image, ce_coef, dice_coef,
                        gscale, gmul, ignore_index, accumulate)


def ce_dice_step(logits_bpc, targets, C_, dlogits, weight=None, class_mask=None, smooth=1e-5, per_image=False, ce_coef=1.0, dice_coef=1.0,
                 gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """ce_dice_fwd + ce_dice_bwd of the same logits in two launches (dct_ce_dice_step; bit for bit the two calls).  Returns
    (out4, dice_gc, sums); ``dlogits`` is written (added to)."""
    return _overlap_step("dice", (), logits_bpc, targets, C_, dlogits, weight, class_mask, smooth, per_image, ce_coef, dice_coef, gscale, gmul,
                         ignore_index, accumulate)


def ce_tversky_fwd(logits_bpc, targets, C_, weight=None, class_mask=None, smooth=1e-5, alpha=0.3, beta=0.7, gamma=1.0, per_image=False,
                   ce_coef=1.0, tversky_coef=1.0, ignore_index=255):
    """Tversky / focal Tversky / CE + Tversky (dct_ce_tversky_fwd; the rule: include/dct.h).  ``logits_bpc``: fp32 [B, ..., C] dense;
    ``targets``: int64, one per pixel; ``class_mask``: bit c = class c is in the mean (None: all).  Returns device tensors ``out4`` =
    (total, ce, sum w, tversky), ``tversky_gc`` [G, C] (the index T_gc) and ``sums`` [G, C, 3] (G = B under ``per_image``, else 1)."""
    return _overlap_fwd("tversky", (alpha, beta, gamma), logits_bpc, targets, C_, weight, class_mask, smooth, per_image, ce_coef, tversky_coef,
                        ignore_index)


def ce_tversky_bwd(logits_bpc, targets, C_, out4, sums, dlogits, weight=None, class_mask=None, smooth=1e-5, alpha=0.3, beta=0.7, gamma=1.0,
                   per_image=False, ce_coef=1.0, tversky_coef=1.0, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """``out4`` and ``sums``: those of ce_tversky_fwd under the same arguments."""
    return _overlap_bwd("tversky", (alpha, beta, gamma), logits_bpc, targets, C_, out4, sums, dlogits, weight, class_mask, smooth, per_image,
                        ce_coef, tversky_coef, gscale, gmul, ignore_index, accumulate)


def ce_tversky_step(logits_bpc, targets, C_, dlogits, weight=None, class_mask=None, smooth=1e-5, alpha=0.3, beta=0.7, gamma=1.0,
                    per_image=False, ce_coef=1.0, tversky_coef=1.0, gscale=None, gmul=1.0, ignore_index=255, accumulate=False):
    """ce_tversky_fwd + ce_tversky_bwd of the same logits in two launches (dct_ce_tversky_step; bit for bit the two calls).  Returns
    (out4, tversky_gc, sums); ``dlogits`` is written (added to)."""
    return _overlap_step("tversky", (alpha, beta, gamma), logits_bpc, targets, C_, dlogits, weight, class_mask, smooth, per_image, ce_coef,
                         tversky_coef, gscale, gmul, ignore_index, accumulate)


def softmax_fwd(logits_pc, C_):
    probs = torch.empty_like(logits_pc)
    call("dct_softmax_fwd", ptr(logits_pc), ptr(probs), logits_pc.numel() // C_, C_, stream())
    return probs


def softmax_bwd(probs, dprobs, C_, dlogits=None, accumulate=False):
    if dlogits is None:
        dlogits = torch.empty_like(probs)
    call("dct_softmax_bwd", ptr(probs), ptr(dprobs), ptr(dlogits), probs.numel() // C_, C_, int(accumulate), stream())
    return dlogits


def entropy_fwd(probs, C_):
    out = torch.empty(probs.numel() // C_, dtype=torch.float32, device=probs.device)
    call("dct_entropy_fwd", ptr(probs), ptr(out), probs.numel() // C_, C_, stream())
    return out


def entropy_bwd(probs, dmap, C_):
    out = torch.empty_like(probs)
    call("dct_entropy_bwd", ptr(probs), ptr(dmap), ptr(out), probs.numel() // C_, C_, stream())
    return out


def jsd_map_fwd(probs: List[torch.Tensor], C_):
    P = probs[0].numel() // C_
    out = torch.empty(P, dtype=torch.float32, device=probs[0].device)
    call("dct_jsd_map_fwd", _ptr_array(probs), len(probs), ptr(out), P, C_, stream())
    return out


def jsd_map_bwd(probs: List[torch.Tensor], dmap, C_):
    outs = [torch.empty_like(p) for p in probs]
    call("dct_jsd_map_bwd", _ptr_array(probs), len(probs), ptr(dmap), _ptr_array(outs), probs[0].numel() // C_, C_, stream())
    return outs


def kl_map_fwd(p, y, C_, eps=1e-10):
    out = torch.empty(p.numel() // C_, dtype=torch.float32, device=p.device)
    call("dct_kl_map_fwd", ptr(p), ptr(y), ptr(out), p.numel() // C_, C_, float(eps), stream())
    return out


def kl_map_bwd(p, y, dmap, C_, eps=1e-10):
    dp = torch.empty_like(p)
    call("dct_kl_map_bwd", ptr(p), ptr(y), ptr(dmap), ptr(dp), p.numel() // C_, C_, float(eps), stream())
    return dp


def jsd_logits_fwd(logits: List[torch.Tensor], C_):
    out = torch.empty(1, dtype=torch.float32, device=logits[0].device)
    ws = _loss_ws(out.device)
    call("dct_jsd_logits_fwd", _ptr_array(logits), len(logits), logits[0].numel() // C_, C_, ptr(out), ptr(ws), ws.numel(), stream())
    return out


def jsd_logits_bwd(logits: List[torch.Tensor], C_, dlogits: List[torch.Tensor], gscale=None, gmul=1.0, accumulate=False):
    call("dct_jsd_logits_bwd", _ptr_array(logits), len(logits), logits[0].numel() // C_, C_, ptr(gscale), float(gmul),
         _ptr_array(dlogits), int(accumulate), stream())
    return dlogits


def jsd_logits_step(logits: List[torch.Tensor], C_, dlogits: List[torch.Tensor] = None, want_probs: bool = True, gscale=None, gmul=1.0,
                    accumulate=False):
    """-> (mean JSD [1], [softmax(logits_s)] or None): `jsd_logits_fwd`, the S `softmax_fwd` maps and `jsd_logits_bwd` into ``dlogits`` (None:
    no gradients) as ONE pass over the logits + the finalize -- bit for bit what the separate launches give (dct_jsd_logits_step)."""
    dev = logits[0].device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _loss_ws(dev)
    probs = [torch.empty_like(lp) for lp in logits] if want_probs else None
    call("dct_jsd_logits_step", _ptr_array(logits), len(logits), logits[0].numel() // C_, C_, ptr(out),
         _ptr_array(probs) if probs is not None else None, ptr(gscale), float(gmul),
         _ptr_array(dlogits) if dlogits is not None else None, int(accumulate), ptr(ws), ws.numel(), stream())
    return out, probs


PL_CROSS, PL_ENSEMBLE = 0, 1        # include/dct.h DCT_PL_*
PL_TEACHERS = {"cross": PL_CROSS, "ensemble": PL_ENSEMBLE}


# The three view-consistency families (hard pseudo-labels dct_pl_*, sharpened soft pseudo-labels dct_spl_*, softmax-MSE dct_mse_*) differ
# in the entry point's name and in the rule's scalars, which follow (S, teacher, tau) in every signature.
def _cons_map_fwd(entry, probs, C_, teacher, tau, scalars, want_kept):
    P = probs[0].numel() // C_
    out = torch.empty(P, dtype=torch.float32, device=probs[0].device)
    kept = torch.empty_like(out) if want_kept else None
    call(entry, _ptr_array(probs), len(probs), int(teacher), float(tau), *map(float, scalars), ptr(out), ptr(kept), P, C_, stream())
    return out, kept


def _cons_map_bwd(entry, probs, dmap, C_, teacher, tau, scalars):
    outs = [torch.empty_like(p) for p in probs]
    call(entry, _ptr_array(probs), len(probs), int(teacher), float(tau), *map(float, scalars), ptr(dmap), _ptr_array(outs),
         probs[0].numel() // C_, C_, stream())
    return outs


def _cons_logits_step(entry, logits, C_, dlogits, want_probs, gscale, gmul, accumulate, teacher, tau, scalars):
    dev = logits[0].device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    ws = _loss_ws(dev)
    probs = [torch.empty_like(lp) for lp in logits] if want_probs else None
    call(entry, _ptr_array(logits), len(logits), int(teacher), float(tau), *map(float, scalars), logits[0].numel() // C_, C_, ptr(out),
         _ptr_array(probs) if probs is not None else None, ptr(gscale), float(gmul),
         _ptr_array(dlogits) if dlogits is not None else None, int(accumulate), ptr(ws), ws.numel(), stream())
    return out, probs


def pl_map_fwd(probs: List[torch.Tensor], C_, teacher=PL_CROSS, tau=0.0, eps=1e-10, want_kept: bool = True):
    """-> (map [P], kept map [P] or None) of the pseudo-label consistency term over S probability maps (the rule: include/dct.h, dct_pl_*)."""
    return _cons_map_fwd("dct_pl_map_fwd", probs, C_, teacher, tau, (eps,), want_kept)


def pl_map_bwd(probs: List[torch.Tensor], dmap, C_, teacher=PL_CROSS, tau=0.0, eps=1e-10):
    return _cons_map_bwd("dct_pl_map_bwd", probs, dmap, C_, teacher, tau, (eps,))


def pl_logits_step(logits: List[torch.Tensor], C_, dlogits: List[torch.Tensor] = None, want_probs: bool = True, gscale=None, gmul=1.0,
                   accumulate=False, teacher=PL_CROSS, tau=0.0, eps=1e-10):
    """-> (out2 = (mean loss over all pixels, kept fraction), [softmax(logits_s)] or None): the pseudo-label consistency term of the step from
    logits, its S softmax maps and its logit gradients into ``dlogits`` (None: no gradients) in ONE pass + the finalize (dct_pl_logits_step)."""
    return _cons_logits_step("dct_pl_logits_step", logits, C_, dlogits, want_probs, gscale, gmul, accumulate, teacher, tau, (eps,))


def spl_map_fwd(probs: List[torch.Tensor], C_, teacher=PL_CROSS, tau=0.0, temperature=0.5, eps=1e-10, want_kept: bool = True):
    """-> (map [P], kept map [P] or None) of the soft pseudo-label consistency term (sharpened teachers) over S probability maps (the rule:
    include/dct.h, dct_spl_*)."""
    return _cons_map_fwd("dct_spl_map_fwd", probs, C_, teacher, tau, (temperature, eps), want_kept)


def spl_map_bwd(probs: List[torch.Tensor], dmap, C_, teacher=PL_CROSS, tau=0.0, temperature=0.5, eps=1e-10):
    return _cons_map_bwd("dct_spl_map_bwd", probs, dmap, C_, teacher, tau, (temperature, eps))


def spl_logits_step(logits: List[torch.Tensor], C_, dlogits: List[torch.Tensor] = None, want_probs: bool = True, gscale=None, gmul=1.0,
                    accumulate=False, teacher=PL_CROSS, tau=0.0, temperature=0.5, eps=1e-10):
    """`pl_logits_step` with sharpened soft teachers: -> (out2 = (mean loss over all pixels, kept fraction), [softmax(logits_s)] or None), the
    logit gradients into ``dlogits`` (None: no gradients), in ONE pass + the finalize (dct_spl_logits_step)."""
    return _cons_logits_step("dct_spl_logits_step", logits, C_, dlogits, want_probs, gscale, gmul, accumulate, teacher, tau, (temperature, eps))


def mse_map_fwd(probs: List[torch.Tensor], C_, teacher=PL_CROSS, tau=0.0, want_kept: bool = True):
    """-> (map [P], kept map [P] or None) of the softmax-MSE consistency term over S probability maps (the rule: include/dct.h, dct_mse_*)."""
    return _cons_map_fwd("dct_mse_map_fwd", probs, C_, teacher, tau, (), want_kept)


def mse_map_bwd(probs: List[torch.Tensor], dmap, C_, teacher=PL_CROSS, tau=0.0):
    return _cons_map_bwd("dct_mse_map_bwd", probs, dmap, C_, teacher, tau, ())


def mse_logits_step(logits: List[torch.Tensor], C_, dlogits: List[torch.Tensor] = None, want_probs: bool = True, gscale=None, gmul=1.0,
                    accumulate=False, teacher=PL_CROSS, tau=0.0):
    """`pl_logits_step` with the squared distance between the softmax outputs: -> (out2 = (mean loss over all pixels, kept fraction),
    [softmax(logits_s)] or None), the logit gradients into ``dlogits`` (None: no gradients), in ONE pass + the finalize (dct_mse_logits_step)."""
    return _cons_logits_step("dct_mse_logits_step", logits, C_, dlogits, want_probs, gscale, gmul, accumulate, teacher, tau, ())


def kl_logits_fwd(p_logits, y_logits, C_, eps=1e-10):
    out = torch.empty(1, dtype=torch.float32, device=p_logits.device)
    ws = _loss_ws(out.device)
    call("dct_kl_logits_fwd", ptr(p_logits), ptr(y_logits), p_logits.numel() // C_, C_, float(eps), ptr(out), ptr(ws), ws.numel(), stream())
    return out


def kl_logits_bwd(p_logits, y_logits, C_, dp, gscale=None, gmul=1.0, eps=1e-10, accumulate=False):
    call("dct_kl_logits_bwd", ptr(p_logits), ptr(y_logits), p_logits.numel() // C_, C_, float(eps), ptr(gscale), float(gmul),
         ptr(dp), int(accumulate), stream())
    return dp


def argmax(x_pc, C_):
    out = torch.empty(x_pc.numel() // C_, dtype=torch.int64, device=x_pc.device)
    call("dct_argmax", ptr(x_pc), ptr(out), x_pc.numel() // C_, C_, stream())
    return out


def fgsm_step(x, g, eps, want_noise=True):
    xa = torch.empty_like(x)
    noise = torch.empty_like(x) if want_noise else None
    call("dct_fgsm_step", ptr(x), ptr(g), float(eps), ptr(xa), ptr(noise), x.numel(), stream())
    return xa, noise


def _vat_shape(t):
    assert t.dim() >= 2 and t.dtype == torch.float32 and t.is_contiguous(), "dct_amd: VAT launches take dense fp32 [N, ...] tensors"
    return int(t.shape[0]), t.numel() // int(t.shape[0])


def vat_workspace(N, per, device):
    """The float64 block partials of N samples of ``per`` elements (dct_vat_workspace_bytes): written by vat_noise / vat_sumsq, read by the
    vat_perturb launches behind them.  A tensor of its own, not the per-stream scratch: it lives across other launches."""
    nbytes = _lib.load().dct_vat_workspace_bytes(int(N), int(per))
    if nbytes == 0:
        raise ValueError(f"dct_amd: VAT over {N} samples of {per} elements is out of range")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def vat_noise(d, seed, calls=None, offset=0, workspace=None):
    """d (dense fp32 [N, ...], overwritten) = Gaussian noise of draw number ``calls[0] + 1`` (``calls``: int64[1] on the device, only read:
    the graph-replayable form) or ``offset``, and every sample's sum-of-squares partials into ``workspace``.  -> (d, workspace)"""
    N, per = _vat_shape(d)
    ws = workspace if workspace is not None else vat_workspace(N, per, d.device)
    if calls is not None:
        assert calls.dtype == torch.int64 and calls.numel() >= 1 and calls.device == d.device
    call("dct_vat_noise", ptr(d), N, per, int(seed) & ((1 << 64) - 1), ptr(calls), int(offset), ptr(ws), ws.numel() * 8, stream())
    return d, ws


def vat_sumsq(g, workspace=None):
    """Every sample's sum-of-squares partials of g (dense fp32 [N, ...]) into ``workspace``.  -> workspace"""
    N, per = _vat_shape(g)
    ws = workspace if workspace is not None else vat_workspace(N, per, g.device)
    call("dct_vat_sumsq", ptr(g), N, per, ptr(ws), ws.numel() * 8, stream())
    return ws


def vat_perturb(x, d, radius, workspace, want_r=True, want_norms=False, calls_advance=None):
    """x + (radius / ||d||_n) * d per sample n, with the norms from ``workspace`` (the partials of d: vat_noise / vat_sumsq); a sample whose
    norm is 0 or not finite comes back unchanged.  ``calls_advance`` (int64[1] on the device): the launch adds 1 to it -- for the first
    perturb launch behind a vat_noise launch that read it.  -> (x_out, r or None, float64 norms [N] or None)"""
    N, per = _vat_shape(x)
    assert _vat_shape(d) == (N, per) and d.device == x.device
    xo = torch.empty_like(x)
    r = torch.empty_like(x) if want_r else None
    norms = torch.empty(N, dtype=torch.float64, device=x.device) if want_norms else None
    if calls_advance is not None:
        assert calls_advance.dtype == torch.int64 and calls_advance.numel() >= 1 and calls_advance.device == x.device
    call("dct_vat_perturb", ptr(x), ptr(d), float(radius), N, per, ptr(workspace), workspace.numel() * 8, ptr(xo), ptr(r), ptr(norms),
         ptr(calls_advance), stream())
    return xo, r, norms


def adam_flat(p, g, m, v, step_size, bc2_sqrt, beta1, beta2, eps, weight_decay, bf16_shadow=None, grad_scale=1.0):
    call("dct_adam_flat", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(step_size), float(bc2_sqrt), float(beta1),
         float(beta2), float(eps), float(weight_decay), float(grad_scale), ptr(bf16_shadow), stream())


def adam_flat_dev(p, g, m, v, state, table, beta1, beta2, eps, weight_decay, bf16_shadow=None, grad_scale=1.0):
    """Adam with {step count, lr, table base, table length} in the float64[4] device tensor ``state`` and the
    host-computed {1 - beta1^t, sqrt(1 - beta2^t)} pairs for t = base + 1 ... base + length in the float64 device tensor ``table``
    (the kernel divides lr by the first in double; past the table it forms both itself).  The kernel adds 1 to state[0] first
    (dct_adam_flat_dev)."""
    call("dct_adam_flat_dev", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(state), ptr(table), float(beta1), float(beta2),
         float(eps), float(weight_decay), float(grad_scale), ptr(bf16_shadow), stream())
    return p


GUARD_WORDS = 5     # dct_adam_guard (include/dct.h) as five 64-bit words: norm, max_norm, {coef, skip}, skipped, clipped


def grad_sumsq_workspace(n, device):
    """Workspace of grad_sumsq / adam_flat_dev_guarded for an n-element buffer: one float64 partial per block."""
    return torch.empty(_lib.load().dct_grad_sumsq_workspace_bytes(int(n)) // 8, dtype=torch.float64, device=device)


def adam_guard_record(device, max_norm=0.0):
    """A zeroed dct_adam_guard on ``device`` (an int64[5] tensor; read it through guard_fields) with ``max_norm`` set."""
    rec = torch.zeros(GUARD_WORDS, dtype=torch.int64, device=device)
    rec[1:2].view(torch.float64).fill_(float(max_norm))
    return rec


def guard_fields(rec):
    """Views of a dct_adam_guard record: norm, max_norm (float64[1]), coef (float32[1]), skip (int32[1]), skipped, clipped (int64[1])."""
    return dict(norm=rec[0:1].view(torch.float64), max_norm=rec[1:2].view(torch.float64), coef=rec[2:3].view(torch.float32)[0:1],
                skip=rec[2:3].view(torch.int32)[1:2], skipped=rec[3:4], clipped=rec[4:5])


def grad_sumsq(g, workspace=None):
    """The float64 per-block partial sums of g^2 (dct_grad_sumsq): their sum is ||g||^2, non-finite iff g holds an inf or a NaN."""
    if workspace is None:
        workspace = grad_sumsq_workspace(g.numel(), g.device)
    call("dct_grad_sumsq", ptr(g), g.numel(), ptr(workspace), workspace.numel() * workspace.element_size(), stream())
    return workspace


def adam_flat_dev_guarded(p, g, m, v, state, table, beta1, beta2, eps, weight_decay, workspace, guard, bf16_shadow=None, grad_scale=1.0,
                          skip_nonfinite=False, clip=False):
    """adam_flat_dev behind the guard (dct_adam_flat_dev_guarded): the gradient norm is taken on the device, ``guard`` (adam_guard_record)
    receives it with the decision, and the update is clipped to the record's max_norm (``clip``) or left out altogether when the
    gradient holds an inf or a NaN (``skip_nonfinite``) -- the step count in state[0] then stays too."""
    call("dct_adam_flat_dev_guarded", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(state), ptr(table), float(beta1), float(beta2),
         float(eps), float(weight_decay), float(grad_scale), ptr(bf16_shadow), ptr(workspace),
         workspace.numel() * workspace.element_size(), ptr(guard), int(bool(skip_nonfinite)), int(bool(clip)), stream())
    return p


def dice_counts(logits_bpc, gt_bp, B, C_):
    """logits [B, pix, C] fp32 dense, gt [B, pix] int64 -> (inter, psum, gsum) int32 [B, C]."""
    dev = logits_bpc.device
    cnt = torch.zeros(3, B, C_, dtype=torch.int32, device=dev)
    ppi = logits_bpc.numel() // (B * C_)
    call("dct_dice_counts", ptr(logits_bpc), ptr(gt_bp), B, ppi, C_, ptr(cnt[0]), ptr(cnt[1]), ptr(cnt[2]), stream())
    return cnt[0], cnt[1], cnt[2]


def dice_update(inter, psum, gsum, method3d, axes_mask, smooth, acc):
    """Dice rows of one DiceMeter.add + the meter's running moments (acc: float64 [2, C+1]) in one launch."""
    B, C_ = inter.shape
    rows = 1 if method3d else B
    dice = torch.empty(rows, C_, dtype=torch.float32, device=inter.device)
    call("dct_dice_update", ptr(inter), ptr(psum), ptr(gsum), B, C_, int(method3d), int(axes_mask), float(smooth), ptr(dice), ptr(acc),
         stream())
    return dice


def hausdorff(logits_bhwc, gt_bhw, method3d=False, spacing=(1., 1., 1.)):
    """logits [B, H, W, C] fp32 dense, gt [B, H, W] int64, spacing (sz, sy, sx) -> SQUARED Hausdorff distance fp32 [rows, C]
    (rows = 1 for the batch as a volume, else B), NaN where the class is absent from the prediction or from gt (include/dct.h)."""
    B, H, W, C_ = logits_bhwc.shape
    # the kernels read 16 bytes at a time: a dense view that starts inside its storage (a slice of a larger batch) gets a copy of its own
    if logits_bhwc.data_ptr() % 16:
        logits_bhwc = logits_bhwc.clone()
    if gt_bhw.data_ptr() % 16:
        gt_bhw = gt_bhw.clone()
    sz, sy, sx = (float(s) for s in spacing)
    need = _lib.load().dct_hausdorff_workspace_bytes(B, H, W, C_, int(bool(method3d)))
    ws = _ws(need, logits_bhwc.device)
    hd2 = torch.empty(1 if method3d else B, C_, dtype=torch.float32, device=logits_bhwc.device)
    call("dct_hausdorff", ptr(logits_bhwc), ptr(gt_bhw), B, H, W, C_, int(bool(method3d)), sz, sy, sx, ptr(hd2), ptr(ws), ws.numel(),
         stream())
    return hd2


def largest_component(logits_bhwc, method3d=False, full=False, classes=None, background=0, want_cls=False):
    """logits [B, H, W, C] fp32 dense -> (onehot fp32 [B, H, W, C], cls int64 [B, H, W] or None, stats int32 [rows, C, 3]): the
    argmax map with only the largest connected component of every class in ``classes`` kept (None: every class but ``background``),
    the rest of those classes moved to ``background``; rows = 1 for the batch as a volume, else B; ``full``: 8- / 26- instead of
    4- / 6-connectivity; stats = {components, size of the largest, pixels} per class before cleaning (include/dct.h)."""
    ptr(logits_bhwc)                    # (refuses a CPU tensor before anything is sized or copied)
    B, H, W, C_ = logits_bhwc.shape
    background = int(background)
    classes = [c for c in range(C_) if c != background] if classes is None else [int(c) for c in classes]
    if C_ <= 8 and (not 0 <= background < C_ or any(not 0 <= c < C_ for c in classes) or background in classes):
        raise ValueError(f"largest_component: classes {classes} must lie in [0, {C_}) and may not hold the background class {background}")
    mask = sum(1 << c for c in set(classes)) if C_ <= 8 else 0
    # the kernels read 16 bytes at a time: a dense view that starts inside its storage (a slice of a larger batch) gets a copy of its own
    if logits_bhwc.data_ptr() % 16:
        logits_bhwc = logits_bhwc.clone()
    dev = logits_bhwc.device
    need = _lib.load().dct_components_workspace_bytes(B, H, W, C_, int(bool(method3d)))
    ws = _ws(need, dev)
    onehot = torch.empty(B, H, W, C_, dtype=torch.float32, device=dev)
    cls = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_cls else None
    stats = torch.empty(1 if method3d else B, C_, 3, dtype=torch.int32, device=dev)
    call("dct_largest_component", ptr(logits_bhwc), B, H, W, C_, int(bool(method3d)), int(bool(full)), mask, background, ptr(onehot),
         ptr(cls), ptr(stats), ptr(ws), ws.numel(), stream())
    return onehot, cls, stats


def confusion_counts(logits: List[torch.Tensor], gt: Optional[torch.Tensor] = None):
    """logits: S fp32 tensors [B, pix, C] (or [B, H, W, C]), the predictions of S raters on one batch; gt [B, pix] (or [B, H, W])
    int64 or None -> int32 [B, P, C, C]: the confusion matrix of every pair of raters per image, gt being the last rater, pairs
    (i, j), i < j, in lexicographic order (``dct_confusion_counts``, include/dct.h)."""
    if not isinstance(logits, (list, tuple)) or len(logits) < 1:
        raise ValueError("confusion_counts needs a list of at least one logits tensor")
    shape = logits[0].shape
    if len(shape) not in (3, 4) or any(t.shape != shape for t in logits):
        raise ValueError(f"confusion_counts needs tensors of one shape [B, pix, C] or [B, H, W, C], got {[tuple(t.shape) for t in logits]}")
    B, C_ = shape[0], shape[-1]
    ppi = 1
    for d in shape[1:-1]:
        ppi *= d
    if gt is not None and gt.numel() != B * ppi:
        raise ValueError(f"confusion_counts: gt {tuple(gt.shape)} does not match logits {tuple(shape)}")

    def dense(t, dtype):
        ptr(t)                              # (refuses a CPU tensor before anything is copied)
        if t.dtype != dtype or not t.is_contiguous():
            t = t.to(dtype).contiguous()
        # the kernel reads a pixel at a time, 16 bytes at C = 4: a dense view that starts inside its storage gets a copy of its own
        return t.clone() if t.data_ptr() % 16 else t

    ls = [dense(t.detach(), torch.float32) for t in logits]
    g = dense(gt, torch.int64) if gt is not None else None
    R = len(ls) + (g is not None)
    cnt = torch.zeros(B, R * (R - 1) // 2, C_, C_, dtype=torch.int32, device=ls[0].device)
    call("dct_confusion_counts", _ptr_array(ls), len(ls), ptr(g), B, ppi, C_, ptr(cnt), stream())
    return cnt


def calibration_counts(probs: List[torch.Tensor], gt: torch.Tensor, n_bins: int = 15, classes=None, with_ensemble: bool = False,
                       from_logits: bool = False):
    """probs: S fp32 tensors [B, pix, C] (or [B, H, W, C]), the probabilities (``from_logits``: the logits) of S views on one batch;
    gt [B, pix] (or [B, H, W]) int64 -> (bins int64 [B, R, n_bins, 3], scores int64 [B, R, 2]), R = S + with_ensemble, the last rater
    being the mean of the views' probabilities: per image, rater and confidence bin {pixels, correct pixels, sum of conf * 2^24}, and
    per image and rater {sum of brier * 2^24, sum of nll * 2^24}, over the pixels whose gt lies in ``classes`` (None: every class)
    (``dct_calibration_counts``, include/dct.h)."""
    if not isinstance(probs, (list, tuple)) or len(probs) < 1:
        raise ValueError("calibration_counts needs a list of at least one tensor")
    shape = probs[0].shape
    if len(shape) not in (3, 4) or any(t.shape != shape for t in probs):
        raise ValueError(f"calibration_counts needs tensors of one shape [B, pix, C] or [B, H, W, C], got {[tuple(t.shape) for t in probs]}")
    B, C_ = shape[0], shape[-1]
    ppi = 1
    for d in shape[1:-1]:
        ppi *= d
    if gt is None or gt.numel() != B * ppi:
        raise ValueError(f"calibration_counts: gt {None if gt is None else tuple(gt.shape)} does not match the predictions {tuple(shape)}")
    classes = list(range(min(C_, 32))) if classes is None else [int(c) for c in classes]
    if any(not 0 <= c < C_ for c in classes):
        raise ValueError(f"calibration_counts: classes {classes} must lie in [0, {C_})")
    mask = sum(1 << c for c in set(classes))

    def dense(t, dtype):
        ptr(t)                              # (refuses a CPU tensor before anything is copied)
        if t.dtype != dtype or not t.is_contiguous():
            t = t.to(dtype).contiguous()
        # the kernel reads a pixel at a time, 16 bytes at C = 4: a dense view that starts inside its storage gets a copy of its own
        return t.clone() if t.data_ptr() % 16 else t

    ps = [dense(t.detach(), torch.float32) for t in probs]
    g = dense(gt, torch.int64)
    R = len(ps) + int(bool(with_ensemble))
    n_bins = int(n_bins)
    if not 1 <= n_bins <= 32:
        raise ValueError(f"calibration_counts: n_bins {n_bins} must lie in [1, 32]")
    # one allocation, one zeroing launch: bins in front, scores behind (both int64)
    nb = B * R * n_bins * 3
    buf = torch.zeros(nb + B * R * 2, dtype=torch.int64, device=ps[0].device)
    bins, scores = buf[:nb].view(B, R, n_bins, 3), buf[nb:].view(B, R, 2)
    call("dct_calibration_counts", _ptr_array(ps), len(ps), ptr(g), B, ppi, C_, n_bins, mask, int(bool(with_ensemble)),
         int(bool(from_logits)), ptr(bins), ptr(scores), stream())
    return bins, scores


def _temperature_views(what, logits):
    """The shape, dtype and alignment handling of ``calibration_counts`` -> (dense fp32 tensors, shape, B, pixels per image, C)."""
    if not isinstance(logits, (list, tuple)) or len(logits) < 1:
        raise ValueError(f"{what} needs a list of at least one tensor")
    shape = logits[0].shape
    if len(shape) not in (3, 4) or any(t.shape != shape for t in logits):
        raise ValueError(f"{what} needs tensors of one shape [B, pix, C] or [B, H, W, C], got {[tuple(t.shape) for t in logits]}")
    ppi = 1
    for d in shape[1:-1]:
        ppi *= d
    return shape, shape[0], ppi, shape[-1]


def _dense(t, dtype):
    ptr(t)                                  # (refuses a CPU tensor before anything is copied)
    if t.dtype != dtype or not t.is_contiguous():
        t = t.to(dtype).contiguous()
    # the kernels read a pixel at a time, 16 bytes at C = 4: a dense view that starts inside its storage gets a copy of its own
    return t.clone() if t.data_ptr() % 16 else t


def temperature_sums(logits: List[torch.Tensor], gt: torch.Tensor, betas: torch.Tensor, classes=None, with_ensemble: bool = False,
                     out=None):
    """logits: S fp32 tensors [B, pix, C] (or [B, H, W, C]), the logits of S views on one batch; gt [B, pix] (or [B, H, W]) int64;
    betas [R, K]: K candidate inverse temperatures per rater, R = S + with_ensemble, the last rater being the mean of the views'
    probabilities, scaled as log(p + 1e-10) -> (sums int64 [R, K, 2], counted int64 [1]): per rater and candidate {sum of nll * 2^20,
    sum of d nll / d beta * 2^20} over the pixels whose gt lies in ``classes`` (None: every class), and the number of those pixels
    (``dct_temperature_sums``, include/dct.h).  ``out``: a ``(sums, counted)`` pair of an earlier call, which this one adds to."""
    shape, B, ppi, C_ = _temperature_views("temperature_sums", logits)
    if gt is None or gt.numel() != B * ppi:
        raise ValueError(f"temperature_sums: gt {None if gt is None else tuple(gt.shape)} does not match the logits {tuple(shape)}")
    classes = list(range(min(C_, 32))) if classes is None else [int(c) for c in classes]
    if any(not 0 <= c < C_ for c in classes):
        raise ValueError(f"temperature_sums: classes {classes} must lie in [0, {C_})")
    mask = sum(1 << c for c in set(classes))
    R = len(logits) + int(bool(with_ensemble))
    if betas is None or betas.dim() != 2 or betas.shape[0] != R or not 1 <= betas.shape[1] <= 16:
        raise ValueError(f"temperature_sums: betas {None if betas is None else tuple(betas.shape)} must be [{R}, K], K in [1, 16]")
    zs = [_dense(t.detach(), torch.float32) for t in logits]
    g = _dense(gt, torch.int64)
    bt = _dense(betas.detach(), torch.float32)
    K_ = bt.shape[1]
    if out is None:
        # one allocation, one zeroing launch: the sums in front, the pixel count behind (both int64)
        buf = torch.zeros(R * K_ * 2 + 1, dtype=torch.int64, device=zs[0].device)
        sums, counted = buf[:R * K_ * 2].view(R, K_, 2), buf[R * K_ * 2:]
    else:
        sums, counted = out
        if (sums.dtype != torch.int64 or counted.dtype != torch.int64 or tuple(sums.shape) != (R, K_, 2) or counted.numel() != 1
                or not sums.is_contiguous()):
            raise ValueError(f"temperature_sums: out must be (int64 [{R}, {K_}, 2] contiguous, int64 [1])")
    call("dct_temperature_sums", _ptr_array(zs), len(zs), ptr(g), B, ppi, C_, mask, int(bool(with_ensemble)), ptr(bt), K_, ptr(sums),
         ptr(counted), stream())
    return sums, counted


def temperature_apply(logits: List[torch.Tensor], betas, with_ensemble: bool = False):
    """logits: S fp32 tensors [B, pix, C] (or [B, H, W, C]); betas: R = S + with_ensemble inverse temperatures (host numbers) -> a
    list of R fp32 tensors of the logits' shape: softmax(beta_r * z_r) for the views and, last, softmax(beta_R * log(p_ens + 1e-10))
    for the mean p_ens of the views' softmax at temperature 1 (``dct_temperature_apply``, include/dct.h)."""
    shape, B, ppi, C_ = _temperature_views("temperature_apply", logits)
    R = len(logits) + int(bool(with_ensemble))
    bs = [float(b) for b in (betas.tolist() if hasattr(betas, "tolist") else betas)]
    if len(bs) != R:
        raise ValueError(f"temperature_apply: {len(bs)} inverse temperatures for {R} raters")
    zs = [_dense(t.detach(), torch.float32) for t in logits]
    outs = [torch.empty(tuple(shape), dtype=torch.float32, device=zs[0].device) for _ in range(R)]
    call("dct_temperature_apply", _ptr_array(zs), len(zs), B, ppi, C_, (C.c_float * R)(*bs), int(bool(with_ensemble)), _ptr_array(outs),
         stream())
    return outs


# ------------------------------------------------------------------------------ Enet family
class Tf(object):
    """Producer transform act(scale*x + shift) applied by consumers on load (include/dct.h dct_enet_tf)."""
    NONE, AFFINE, PRELU, RELU = 0, 1, 2, 3

    def __init__(self, scale, shift, slope=None, mode=1):
        self.scale, self.shift, self.slope, self.mode = scale, shift, slope, mode

    def c(self):
        return EnetTf(ptr(self.scale), ptr(self.shift), ptr(self.slope), int(self.mode))


def _tfp(tf):
    if tf is None:
        return None, None
    s = tf.c()
    return s, C.byref(s)


_red_ws = {}


def _enet_ws(device, nbytes):
    """Reduction scratch, cached per (device, stream): kernels of two models queued on different streams must not
    share it.  While a HIP graph is being captured the buffer comes from the graph's own pool instead."""
    if _group() is not None:        # members of a pass group run at the same time: scratch of their own, kept until the launches
        return keep(torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device))
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    t = _red_ws.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _red_ws[key] = t
    return t


def _mixed(*ts):
    """(dtype code T, f32 mask) of a call whose view arguments are ``ts`` (None = absent): T is bf16 / f16 when any
    view is, and bit k of the mask marks view k as fp32 storage."""
    low = [t.dtype for t in ts if t is not None and t.dtype in (torch.bfloat16, torch.float16)]
    if len(set(low)) > 1:
        raise RuntimeError("dct_amd: bf16 and f16 views in one Enet call")
    mask = 0
    for k, t in enumerate(ts):
        if t is not None and t.dtype == torch.float32:
            mask |= 1 << k
        elif t is not None and t.dtype not in (torch.bfloat16, torch.float16):
            raise RuntimeError(f"dct_amd: unsupported dtype {t.dtype}")
    return (DTYPE_OF[low[0]] if low else F32), mask


def enet_conv(x, w, bias, tf, y, *, R, S, stride=1, dil=1, pad_h=0, pad_w=0, transposed=False, ws=(0, 0, 0),
              resid_grad=None, resid_mask=None, accumulate=False, compute=None):
    """``compute``: the net's compute dtype.  A forward conv reads a raw fp32 tensor and writes one, so no view says which mode
    the call belongs to; in bf16 / f16 mode the contraction's operands are rounded to that type (MFMA form, csrc/enet.hip)."""
    d = conv_desc(R, S, stride, dil, pad_h, pad_w, accumulate=accumulate)
    vx, vy = view(x), view(y)
    keep, tfp = _tfp(tf)
    vrg = view(resid_grad) if resid_grad is not None else None
    vrm = view(resid_mask) if resid_mask is not None else None
    dt, fm = _mixed(x, y, resid_grad, resid_mask)
    if dt == F32 and compute in (torch.bfloat16, torch.float16):
        dt = DTYPE_OF[compute]
    call("dct_enet_conv", C.byref(vx), ptr(w), ptr(bias), tfp, C.byref(vy), C.byref(d), int(transposed),
         int(ws[0]), int(ws[1]), int(ws[2]), C.byref(vrg) if vrg is not None else None,
         C.byref(vrm) if vrm is not None else None, fm, dt, stream())
    return y


def enet_conv_stats(x, w, bias, tf, y, stats, *, R, S, stride=1, dil=1, pad_h=0, pad_w=0, transposed=False, ws=(0, 0, 0), compute=None):
    """enet_conv with the consumer BatchNorm's partial sums written by the convolution's epilogue into ``stats`` (float64,
    >= tiles * C * 3 elements, tiles = ceil(pixels / 32)).  -> number of partial rows written, 0 when the call did not take the
    MFMA form (the statistics then need the usual reduction)."""
    d = conv_desc(R, S, stride, dil, pad_h, pad_w)
    vx, vy = view(x), view(y)
    keep, tfp = _tfp(tf)
    dt, fm = _mixed(x, y)
    if dt == F32 and compute in (torch.bfloat16, torch.float16):
        dt = DTYPE_OF[compute]
    rows = C.c_int(0)
    cap = stats.numel() // (3 * y.shape[3])
    call("dct_enet_conv_stats", C.byref(vx), ptr(w), ptr(bias), tfp, C.byref(vy), C.byref(d), int(transposed),
         int(ws[0]), int(ws[1]), int(ws[2]), fm, dt, ptr(stats), int(cap), C.byref(rows), stream())
    return int(rows.value)


def enet_bn_fwd_stats(raw, gamma, beta, eps, momentum, running_mean, running_var, training, scale, shift, mean, invstd,
                      dtype_hint=None, save_var=None, partial=None, partial_rows=0):
    vr = view(raw)
    dt, fm = _mixed(raw)
    if partial is not None and partial_rows > 0:          # rows written by enet_conv_stats: fold only
        call("dct_enet_bn_fwd_stats_rows", C.byref(vr), ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean),
             ptr(running_var), int(training), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(save_var), fm, dt, ptr(partial),
             partial.numel() * partial.element_size(), int(partial_rows), stream())
        return
    ws = _enet_ws(raw.device, _lib.load().dct_enet_reduce_workspace_bytes(raw.shape[3]))
    call("dct_enet_bn_fwd_stats", C.byref(vr), ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean),
         ptr(running_var), int(training), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(save_var), fm, dt, ptr(ws), ws.numel(),
         stream())


def enet_conv_bnbwd_stats(x, w, y, stats, rec_raw, rec_tf, rec_mean, rec_invstd, *, R, S, stride=1, dil=1, pad_h=0, pad_w=0,
                          transposed=False, ws=(0, 0, 0), compute=None):
    """Data-gradient convolution y = dgrad(x) (enet_conv without bias / transform / residual) whose epilogue also writes the
    BatchNorm-backward partial sums of the layer that produced y's tensor (raw output ``rec_raw``, consumer transform ``rec_tf``,
    saved statistics) into ``stats`` (float64, >= tiles * C * 3).  -> partial rows written (0: the usual reduction is needed)."""
    d = conv_desc(R, S, stride, dil, pad_h, pad_w)
    vx, vy, vr = view(x), view(y), view(rec_raw)
    dt, fm = _mixed(x, y)
    if dt == F32 and compute in (torch.bfloat16, torch.float16):
        dt = DTYPE_OF[compute]
    act = rec_tf.mode if rec_tf.mode in (2, 3) else 0
    rows = C.c_int(0)
    cap = stats.numel() // (3 * y.shape[3])
    call("dct_enet_conv_bnbwd_stats", C.byref(vx), ptr(w), C.byref(vy), C.byref(d), int(transposed), int(ws[0]), int(ws[1]), int(ws[2]),
         fm, dt, C.byref(vr), ptr(rec_tf.scale), ptr(rec_tf.shift), ptr(rec_tf.slope), int(act), ptr(rec_mean), ptr(rec_invstd),
         ptr(stats), int(cap), C.byref(rows), stream())
    return int(rows.value)


def enet_bn_bwd(raw, g, g_mask, tf, mean, invstd, dgamma, dbeta, dslope, c1c2, draw, training=True, partial=None, partial_rows=0):
    vr, vg, vd = view(raw), view(g), view(draw)
    vm = view(g_mask) if g_mask is not None else None
    act = tf.mode if tf.mode in (2, 3) else 0
    dt, fm = _mixed(raw, g, g_mask, draw)
    if partial is not None and partial_rows != 0:         # rows written by enet_conv_bnbwd_stats: fold + apply only
        call("dct_enet_bn_bwd_rows", C.byref(vr), C.byref(vg), None,
             ptr(tf.scale), ptr(tf.shift), ptr(tf.slope), int(act), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta), ptr(dslope),
             ptr(c1c2), int(training), C.byref(vd), fm, dt, ptr(partial), partial.numel() * partial.element_size(), int(partial_rows),
             stream())
        return draw
    ws = _enet_ws(raw.device, _lib.load().dct_enet_reduce_workspace_bytes(raw.shape[3]))
    call("dct_enet_bn_bwd", C.byref(vr), C.byref(vg), C.byref(vm) if vm is not None else None,
         ptr(tf.scale), ptr(tf.shift), ptr(tf.slope), int(act), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta), ptr(dslope),
         ptr(c1c2), int(training), C.byref(vd), fm, dt, ptr(ws), ws.numel(), stream())
    return draw


def enet_bn_bwd_sums(raw, g, g_mask, tf, mean, invstd, dgamma, dbeta, dslope, c1c2, training=True, partial=None, partial_rows=0):
    """The sums half of `enet_bn_bwd`: parameter gradients (+=) and the apply pass's two means (c1c2)."""
    vr, vg = view(raw), view(g)
    vm = view(g_mask) if g_mask is not None else None
    act = tf.mode if tf.mode in (2, 3) else 0
    dt, fm = _mixed(raw, g, g_mask)
    if partial is not None and partial_rows > 0:
        ws, nbytes = partial, partial.numel() * partial.element_size()
    else:
        ws = _enet_ws(raw.device, _lib.load().dct_enet_reduce_workspace_bytes(raw.shape[3]))
        nbytes, partial_rows = ws.numel(), 0
    call("dct_enet_bn_bwd_sums", C.byref(vr), C.byref(vg), C.byref(vm) if vm is not None else None,
         ptr(tf.scale), ptr(tf.shift), ptr(tf.slope), int(act), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta), ptr(dslope),
         ptr(c1c2), int(training), fm, dt, ptr(ws), nbytes, int(partial_rows), stream())


def enet_bn_bwd_apply(raw, g, g_mask, tf, mean, invstd, c1c2, draw, leaf=False):
    """The apply half: draw = BatchNorm-backward of g (elementwise, from raw / g / c1c2).  ``leaf``: only weight gradients read the
    result -- under a `LeafSide` the launch is held back with them."""
    vr, vg, vd = view(raw), view(g), view(draw)
    vm = view(g_mask) if g_mask is not None else None
    act = tf.mode if tf.mode in (2, 3) else 0
    dt, fm = _mixed(raw, g, g_mask, draw)
    call("dct_enet_bn_bwd_apply", C.byref(vr), C.byref(vg), C.byref(vm) if vm is not None else None,
         ptr(tf.scale), ptr(tf.shift), ptr(tf.slope), int(act), ptr(mean), ptr(invstd), ptr(c1c2), C.byref(vd), fm, dt, int(leaf), stream())
    return draw


def enet_conv_bwd_in(raw, w, tf, g, g_mask, mean, invstd, c1c2, y, *, R, S, stride=1, dil=1, pad_h=0, pad_w=0, transposed=False,
                     ws=(0, 0, 0), resid_grad=None, resid_mask=None, accumulate=False, compute=None, bn=None):
    """Data-gradient convolution whose input is the BatchNorm-backward result of the layer (raw, tf, saved mean / invstd) for the
    upstream gradient g [masked by g_mask], computed ON LOAD (include/dct.h dct_enet_conv_bwd_in).  ``bn`` = (stats, rec_raw, rec_tf,
    rec_mean, rec_invstd): also write the output side's BatchNorm-backward partial rows (as enet_conv_bnbwd_stats).
    -> None when the library has no on-load form for this call (the caller materialises the tensor), else the rows written (0 without
    ``bn``)."""
    d = conv_desc(R, S, stride, dil, pad_h, pad_w, accumulate=accumulate)
    vx, vy, vg = view(raw), view(y), view(g)
    vm = view(g_mask) if g_mask is not None else None
    keep_tf, tfp = _tfp(tf)
    vrg = view(resid_grad) if resid_grad is not None else None
    vrm = view(resid_mask) if resid_mask is not None else None
    dt, fm = _mixed(raw, y, resid_grad, resid_mask)
    if dt == F32 and compute in (torch.bfloat16, torch.float16):
        dt = DTYPE_OF[compute]
    b = _lib.EnetBwdIn(C.pointer(vg), C.pointer(vm) if vm is not None else None, ptr(mean), ptr(invstd), ptr(c1c2))
    rows = C.c_int(0)
    if bn is not None:
        stats, rec_raw, rec_tf, rec_mean, rec_invstd = bn
        vr = view(rec_raw)
        act = rec_tf.mode if rec_tf.mode in (2, 3) else 0
        extra = (C.byref(vr), ptr(rec_tf.scale), ptr(rec_tf.shift), ptr(rec_tf.slope), int(act), ptr(rec_mean), ptr(rec_invstd),
                 ptr(stats), int(stats.numel() // (3 * y.shape[3])), C.byref(rows))
    else:
        extra = (None, None, None, None, 0, None, None, None, 0, None)
    rc = getattr(_lib.load(), "dct_enet_conv_bwd_in")(
        C.byref(vx), ptr(w), tfp, C.byref(b), C.byref(vy), C.byref(d), int(transposed), int(ws[0]), int(ws[1]), int(ws[2]),
        C.byref(vrg) if vrg is not None else None, C.byref(vrm) if vrm is not None else None, fm, dt, *extra, stream())
    if rc == -2:            # DCT_ERR_UNSUPPORTED: no MFMA form for this call
        return None
    _lib.check(rc, "dct_enet_conv_bwd_in")
    return int(rows.value)


def bn_fwd(raw, gamma, beta, eps, momentum, running_mean, running_var, training, scale, shift, mean, invstd, y=None, relu=True):
    """Wide-channel BatchNorm2d (+ReLU) forward of unet_bn: statistics -> scale/shift (+ running statistics) -> y."""
    vr = view(raw)
    vy = view(y) if y is not None else None
    ws = _enet_ws(raw.device, _lib.load().dct_bn_workspace_bytes(raw.shape[3]))
    call("dct_bn_fwd", C.byref(vr), ptr(gamma), ptr(beta), float(eps), float(momentum), ptr(running_mean), ptr(running_var),
         int(training), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), C.byref(vy) if vy is not None else None, int(relu),
         _dt(raw), ptr(ws), ws.numel(), stream())
    return y


def bn_bwd(raw, g, scale, shift, mean, invstd, dgamma, dbeta, c1c2, draw, training=True, relu=True, accumulate=True):
    vr, vg, vd = view(raw), view(g), view(draw)
    ws = _enet_ws(raw.device, _lib.load().dct_bn_workspace_bytes(raw.shape[3]))
    call("dct_bn_bwd", C.byref(vr), C.byref(vg), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), ptr(dgamma), ptr(dbeta),
         int(accumulate), ptr(c1c2), int(training), int(relu), C.byref(vd), _dt(raw), ptr(ws), ws.numel(), stream())
    return draw


def enet_channel_sum(x, out):
    vx = view(x)
    ws = _enet_ws(x.device, _lib.load().dct_enet_reduce_workspace_bytes(x.shape[3]))
    dt, fm = _mixed(x)
    call("dct_enet_channel_sum", C.byref(vx), ptr(out), fm, dt, ptr(ws), ws.numel(), stream())


def enet_tail_fwd(raw, tf, main_in, rawm, tfm, idx, idx_channels, mode, out):
    vr, vo = view(raw), view(out)
    vmain = view(main_in) if main_in is not None else None
    vrm = view(rawm) if rawm is not None else None
    k1, tfp = _tfp(tf)
    k2, tfmp = _tfp(tfm)
    dt, fm = _mixed(raw, main_in, rawm, out)
    call("dct_enet_tail_fwd", C.byref(vr), tfp, C.byref(vmain) if vmain is not None else None,
         C.byref(vrm) if vrm is not None else None, tfmp, ptr(idx), int(idx_channels), int(mode), C.byref(vo), fm, dt, stream())
    return out


def enet_tail_bwd(dout, out_mask, idx, idx_channels, mode, dst, accumulate=False):
    vd, vm, vdst = view(dout), view(out_mask), view(dst)
    dt, fm = _mixed(dout, out_mask, dst)
    call("dct_enet_tail_bwd", C.byref(vd), C.byref(vm), ptr(idx), int(idx_channels), int(mode), int(accumulate), C.byref(vdst),
         fm, dt, stream())
    return dst


def enet_wgrad(a, tfa, b, tfb, dw, *, R, S, stride=1, dil=1, pad_h=0, pad_w=0):
    d = conv_desc(R, S, stride, dil, pad_h, pad_w)
    va, vb = view(a), view(b)
    need = _lib.load().dct_enet_wgrad_workspace_bytes(C.byref(va), C.byref(vb), C.byref(d))
    ws = _enet_ws(a.device, need)
    k1, tfap = _tfp(tfa)
    k2, tfbp = _tfp(tfb)
    dt, fm = _mixed(a, b)
    call("dct_enet_wgrad", C.byref(va), tfap, C.byref(vb), tfbp, ptr(dw), C.byref(d), fm, dt, ptr(ws), ws.numel(), stream())
    return dw
