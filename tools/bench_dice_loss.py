#!/usr/bin/env python3
"""dct_ce_dice_step (CE + soft Dice: value + logit gradient in two launches) beside (a) dct_ce_weighted_step on the same tensors -- the
floor: the same bytes move, 4 C + 8 read twice and 4 C written per pixel -- and (b) the same loss and gradient composed from torch device
ops with autograd (softmax, one-hot, three sums, the quotient, F.cross_entropy, backward): what a user had before.  Shapes: 16 x 256 x
256 x 4 and 16 x 200 x 200 x 2 (B x H x W x C), a quarter of the targets 255, weights {0.1, 1, 2.5, 0} cut to C, foreground classes,
smooth 1e-5, G = 1 and G = B.  Device time between events, arms alternating in one process: one call per window, and (library arms) a
captured graph of 20 calls per window.  Launch counts: the library's own launch counter (dct_prof_read) for its arms, torch.profiler's
kernel events for the composition."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
REPS, WARM, CHAIN = 200, 20, 20
IGN = 255


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def torch_ce_dice(x, t, w, mask, smooth, per_image):
    """The rule of include/dct.h from torch device ops; x: [B, PPI, C] requiring grad.  -> total"""
    B, PPI, C = x.shape
    keep = (t != IGN)
    k = keep[..., None].to(x.dtype)
    p = torch.softmax(x, -1) * k
    y = F.one_hot(torch.where(keep, t, torch.zeros_like(t)), C).to(x.dtype) * k
    dims = (1,) if per_image else (0, 1)
    inter, s, yy = (p * y).sum(dims), p.sum(dims), y.sum(dims)
    d = (2 * inter + smooth) / (s + yy + smooth)
    dice = 1 - d.reshape(-1, C)[:, mask].mean()
    ce = F.cross_entropy(x.reshape(-1, C), t.reshape(-1), weight=w, ignore_index=IGN)
    return ce + dice


def launches(fn):
    _lib.prof_read(True)
    _lib.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    return sum(v["launches"] for v in _lib.prof_read(True).values())


def torch_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else "not counted (the profiler recorded no kernel events)"
    except Exception as e:        # (no tracer in this torch build)
        return f"not counted ({type(e).__name__})"


for B, H, C in ((16, 256, 4), (16, 200, 2)):
    PPI = H * H
    P = B * PPI
    g = torch.Generator(device=dev).manual_seed(P + C)
    x = torch.randn(B, PPI, C, device=dev, generator=g) * 2
    t = torch.randint(0, C, (B, PPI), device=dev, generator=g)
    t[torch.rand(B, PPI, device=dev, generator=g) < 0.25] = IGN
    w = torch.tensor([0.1, 1.0, 2.5, 0.0][:C], device=dev)
    fg = (1 << C) - 2
    dl, out2, ws = torch.empty_like(x), torch.empty(2, device=dev), K._loss_ws(dev)
    out4, dgc, sums = torch.empty(4, device=dev), torch.empty(B, C, device=dev), torch.empty(B, C, 3, device=dev)
    wsd = K._overlap_ws(B, C, True, dev)
    p = K.ptr

    def floor():
        _lib.call("dct_ce_weighted_step", p(x), p(t), P, C, IGN, p(w), 0, p(out2), None, 1.0, p(dl), 0, p(ws), ws.numel(), _lib.stream())

    def dice(per_image):
        def run():
            _lib.call("dct_ce_dice_step", p(x), p(t), B, PPI, C, IGN, p(w), fg, 1e-5, per_image, 1.0, 1.0, p(out4), p(dgc), p(sums), None, 1.0,
                      p(dl), 0, p(wsd), wsd.numel(), _lib.stream())
        return run
    xr = x.clone().requires_grad_(True)
    maskt = torch.tensor([c for c in range(1, C)], device=dev)

    def composed(per_image):
        def run():
            xr.grad = None
            torch_ce_dice(xr, t, w, maskt, 1e-5, per_image).backward()
        return run
    lib_arms = (("dct_ce_weighted_step (floor)", floor), ("dct_ce_dice_step G=1", dice(0)), ("dct_ce_dice_step G=B", dice(1)))
    arms = lib_arms + (("torch composition G=1", composed(False)), ("torch composition G=B", composed(True)))
    for _ in range(WARM):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    # the composition and the kernels compute the same thing
    composed(False)()
    dice(0)()
    torch.cuda.synchronize()
    err = (xr.grad - dl).abs().max().item() / xr.grad.abs().max().item()
    assert err < 1e-3, err
    one = {name: [] for name, _ in arms}
    for _ in range(REPS):
        for name, fn in arms:
            one[name].append(timed(fn))
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in lib_arms:
        gr = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                for _ in range(CHAIN):
                    fn()
        graphs[name] = gr
    torch.cuda.synchronize()
    for _ in range(5):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    chain = {name: [] for name, _ in lib_arms}
    for _ in range(REPS // 4):
        for name, _ in lib_arms:
            chain[name].append(timed(graphs[name].replay) / CHAIN)
    mb = P * (2 * (4 * C + 8) + 4 * C) / 1e6
    for name, fn in arms:
        m1, lo1, hi1 = stats(one[name])
        line = f"B={B} HxW={H}x{H} C={C} {name}: one call between events: median {m1:.1f} us (min {lo1:.1f}, max {hi1:.1f}; {REPS} calls)"
        if name in chain:
            m2, lo2, hi2 = stats(chain[name])
            line += (f"; graph of {CHAIN} calls: median {m2:.2f} us per call (min {lo2:.2f}, max {hi2:.2f}; {REPS // 4} replays) = {mb / m2:.2f} TB/s of "
                     f"the {mb:.1f} MB the pair moves; launches per call: {launches(fn)}")
        else:
            line += f"; launches per call (forward + backward): {torch_launches(fn)}"
        print(line, flush=True)
    print(f"B={B} HxW={H}x{H} C={C}: max |torch gradient - dct_ce_dice_step gradient| / max |gradient| = {err:.2e} (G = 1)", flush=True)
