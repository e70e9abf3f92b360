#!/usr/bin/env python3
"""dct_focal_* (gamma = 2, and the step at gamma = 0 and 0.5 too) beside dct_ce_weighted_* / dct_ce_map_* on the same tensors (the same bytes
move: the floor) at the labeled batches of cfg2 (P = 524,288, C = 4) and cfg4 (P = 320,000, C = 2): fwd, bwd, step, map fwd and map bwd.
Device time between events, the arms of one operation alternating in one process.  Two windows: one call between the events (the
host's enqueue of the later launches is inside it), and a captured graph of 20 calls per arm replayed between the events (device time
only, per call).  Median, min and max over the windows, and the ratio of the medians focal / weighted CE."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
REPS, WARM, CHAIN = 100, 20, 20


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


for P, C in ((524288, 4), (320000, 2)):
    g = torch.Generator(device=dev).manual_seed(P + C)
    x = torch.randn(P, C, device=dev, generator=g) * 2
    t = torch.randint(0, C, (P,), device=dev, generator=g)
    t[torch.rand(P, device=dev, generator=g) < 0.25] = 255
    w = torch.tensor([0.1, 1.0, 2.5, 0.0][:C], device=dev)
    dmap = torch.randn(P, device=dev, generator=g)
    dl, out, m, ws = torch.empty_like(x), torch.empty(2, device=dev), torch.empty(P, device=dev), K._loss_ws(dev)
    p, st, call = K.ptr, _lib.stream, _lib.call
    head = (p(x), p(t), P, C, 255, p(w))

    def focal(gamma):
        return {
            "fwd": lambda: call("dct_focal_fwd", *head, gamma, 0, p(out), p(ws), ws.numel(), st()),
            "bwd": lambda: call("dct_focal_bwd", *head, gamma, 0, p(out[1:2]), None, 1.0, p(dl), 0, st()),
            "step": lambda: call("dct_focal_step", *head, gamma, 0, p(out), None, 1.0, p(dl), 0, p(ws), ws.numel(), st()),
            "map_fwd": lambda: call("dct_focal_map_fwd", *head, gamma, p(m), st()),
            "map_bwd": lambda: call("dct_focal_map_bwd", *head, gamma, p(dmap), 1.0, p(dl), 0, st()),
        }
    ce = {
        "fwd": lambda: call("dct_ce_weighted_fwd", *head, 0, p(out), p(ws), ws.numel(), st()),
        "bwd": lambda: call("dct_ce_weighted_bwd", *head, 0, p(out[1:2]), None, 1.0, p(dl), 0, st()),
        "step": lambda: call("dct_ce_weighted_step", *head, 0, p(out), None, 1.0, p(dl), 0, p(ws), ws.numel(), st()),
        "map_fwd": lambda: call("dct_ce_map_fwd", *head, p(m), st()),
        "map_bwd": lambda: call("dct_ce_map_bwd", *head, p(dmap), 1.0, p(dl), 0, st()),
    }
    f2, f0, fh = focal(2.0), focal(0.0), focal(0.5)
    # bytes per pixel: the logits and targets read (twice by the step), the map / dmap, the gradient written
    mb = {"fwd": 4 * C + 8, "bwd": 4 * C + 8 + 4 * C, "step": 2 * (4 * C + 8) + 4 * C, "map_fwd": 4 * C + 8 + 4, "map_bwd": 4 * C + 8 + 4 + 4 * C}
    ce["fwd"]()                                 # (out[1] is the denominator the bwd arms read)
    for op in ("fwd", "bwd", "step", "map_fwd", "map_bwd"):
        arms = [("ce_weighted", ce[op]), ("focal gamma=2", f2[op])]
        if op == "step":
            arms += [("focal gamma=0", f0[op]), ("focal gamma=0.5", fh[op])]
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
        for _ in range(REPS // 2):
            for name, _ in arms:
                chain[name].append(timed(graphs[name].replay) / CHAIN)
        base = stats(chain["ce_weighted"])[0]
        for name, _ in arms:
            m1, lo1, hi1 = stats(one[name])
            m2, lo2, hi2 = stats(chain[name])
            megab = P * mb[op] / 1e6
            print(f"P={P} C={C} {op} {name}: one call between events: median {m1:.1f} us (min {lo1:.1f}, max {hi1:.1f}; {REPS} calls, arms "
                  f"alternating, after {WARM} warm-up calls); graph of {CHAIN} calls: median {m2:.2f} us per call (min {lo2:.2f}, max {hi2:.2f}; "
                  f"{REPS // 2} replays, arms alternating) = {megab / m2:.2f} TB/s of the {megab:.1f} MB it moves; x{m2 / base:.2f} of ce_weighted")
