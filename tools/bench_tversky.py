#!/usr/bin/env python3
"""dct_ce_tversky_step (gamma = 1 and gamma = 4/3; alpha = 0.3, beta = 0.7) beside dct_ce_dice_step on the same tensors at the labeled
batches of cfg2 (8 x 256 x 256 = 524,288 pixels, C = 4) and cfg4 (8 x 200 x 200 = 320,000 pixels, C = 2), with G = 1 and G = B.  Both
families launch the same forward kernel and a backward kernel over the same bytes, so the expectation is level.  Device time between
events in one process: a captured graph of 20 calls per arm replayed between the events (device time only, per call), the arms
alternating.  Median (min-max) over the windows, and for each Tversky arm whether its median lies outside the Dice arm's min-max by more
than that range's width."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
REPS, WARM, CHAIN = 50, 5, 20


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


for B, H, C in ((8, 256, 4), (8, 200, 2)):
    PPI = H * H
    g = torch.Generator(device=dev).manual_seed(PPI + C)
    x = torch.randn(B, PPI, C, device=dev, generator=g) * 2
    t = torch.randint(0, C, (B, PPI), device=dev, generator=g)
    t[torch.rand(B, PPI, device=dev, generator=g) < 0.25] = 255
    w = torch.tensor([0.1, 1.0, 2.5, 0.0][:C], device=dev)
    fg = (1 << C) - 2
    dl, out4 = torch.empty_like(x), torch.empty(4, device=dev)
    gc, sums = torch.empty(B, C, device=dev), torch.empty(B, C, 3, device=dev)
    ws = K._overlap_ws(B, C, True, dev)
    p, st, call = K.ptr, _lib.stream, _lib.call
    head = (p(x), p(t), B, PPI, C, 255, p(w), fg)
    tail = (p(out4), p(gc), p(sums), None, 1.0, p(dl), 0, p(ws), ws.numel())

    def dice(per_image):
        return lambda: call("dct_ce_dice_step", *head, 1e-5, per_image, 1.0, 1.0, *tail, st())

    def tversky(per_image, gamma):
        return lambda: call("dct_ce_tversky_step", *head, 1e-5, 0.3, 0.7, gamma, per_image, 1.0, 1.0, *tail, st())
    arms = []
    for per_image, G in ((0, "G=1"), (1, "G=B")):
        arms += [(f"dct_ce_dice_step {G}", dice(per_image)), (f"dct_ce_tversky_step gamma=1 {G}", tversky(per_image, 1.0)),
                 (f"dct_ce_tversky_step gamma=4/3 {G}", tversky(per_image, 4.0 / 3.0))]
    for _ in range(WARM):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in arms:
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
    chain = {name: [] for name, _ in arms}
    for _ in range(REPS):
        for name, _ in arms:
            chain[name].append(timed(graphs[name].replay) / CHAIN)
    assert bool(torch.isfinite(out4).all()) and bool(torch.isfinite(dl).all())
    for name, _ in arms:
        m, lo, hi = stats(chain[name])
        line = f"B={B} HxW={H}x{H} C={C} {name}: graph of {CHAIN} calls: median {m:.2f} us per call ({lo:.2f}-{hi:.2f}; {REPS} replays, arms alternating)"
        if "tversky" in name:
            dm, dlo, dhi = stats(chain["dct_ce_dice_step " + name[-3:]])
            off = max(dlo - m, m - dhi, 0.0)
            line += f"; x{m / dm:.3f} of the Dice step's median; " + ("inside Dice's min-max" if off == 0.0 else
                                                                       f"{off:.2f} us outside Dice's min-max (its width: {dhi - dlo:.2f} us)")
        print(line, flush=True)
