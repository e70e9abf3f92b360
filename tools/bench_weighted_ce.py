#!/usr/bin/env python3
"""dct_ce_weighted_step beside dct_ce_step (both: value + logit gradient in two launches; 4 C + 8 bytes read twice and 4 C written per
pixel) at the labeled batches of cfg2 (P = 524,288, C = 4) and cfg5 (P = 1,638,400, C = 2): device time between events, the two arms
alternating in one process.  Two windows: one call between the events (the host's enqueue of the second launch is inside it), and a
captured graph of 20 calls per arm replayed between the events (device time only, per call).  Median, min and max over the windows."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
REPS, WARM, CHAIN = 200, 20, 20


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


for P, C in ((524288, 4), (1638400, 2)):
    g = torch.Generator(device=dev).manual_seed(P + C)
    x = torch.randn(P, C, device=dev, generator=g) * 2
    t = torch.randint(0, C, (P,), device=dev, generator=g)
    t[torch.rand(P, device=dev, generator=g) < 0.25] = 255
    w = torch.tensor([0.1, 1.0, 2.5, 0.0][:C], device=dev)
    dl, out, ws = torch.empty_like(x), torch.empty(2, device=dev), K._loss_ws(dev)
    p = K.ptr

    def plain():
        _lib.call("dct_ce_step", p(x), p(t), P, C, 255, p(out), None, 1.0, p(dl), 0, p(ws), ws.numel(), _lib.stream())

    def weighted():
        _lib.call("dct_ce_weighted_step", p(x), p(t), P, C, 255, p(w), 0, p(out), None, 1.0, p(dl), 0, p(ws), ws.numel(), _lib.stream())
    arms = (("dct_ce_step", plain), ("dct_ce_weighted_step", weighted))
    for _ in range(WARM):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    one = {name: [] for name, _ in arms}
    for _ in range(REPS):
        for name, fn in arms:
            one[name].append(timed(fn))
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
    for _ in range(REPS // 4):
        for name, _ in arms:
            chain[name].append(timed(graphs[name].replay) / CHAIN)
    mb = P * (2 * (4 * C + 8) + 4 * C) / 1e6
    for name, _ in arms:
        m1, lo1, hi1 = stats(one[name])
        m2, lo2, hi2 = stats(chain[name])
        print(f"P={P} C={C} {name}: one call between events: median {m1:.1f} us (min {lo1:.1f}, max {hi1:.1f}; {REPS} calls, arms alternating, "
              f"after {WARM} warm-up calls); graph of {CHAIN} calls: median {m2:.2f} us per call (min {lo2:.2f}, max {hi2:.2f}; {REPS // 4} replays, "
              f"arms alternating) = {mb / m2:.2f} TB/s of the {mb:.1f} MB the pair moves")
