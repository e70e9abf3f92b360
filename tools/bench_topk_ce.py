#!/usr/bin/env python3
"""dct_topk_ce_step (k = 1, 10, 100; and dct_topk_ce_fwd / _bwd at k = 10) beside dct_ce_weighted_step on the same tensors at the labeled
batches of cfg2 (P = 524,288, C = 4) and cfg4 (P = 320,000, C = 2).  Device time between events, the arms alternating in one process.
Two windows: one call between the events (the host's enqueue of the later launches is inside it), and a captured graph of 20 calls per
arm replayed between the events (device time only, per call).  Median, min and max over the windows, and the ratio of the medians
top-k / weighted CE.  The top-k step is one memset and five kernels (the weighted CE step: two kernels)."""
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
    dl, out, ws = torch.empty_like(x), torch.empty(2, device=dev), K._loss_ws(dev)
    out2, counts4, vmap, tws = K._topk_ce_bufs(P, dev)
    p, st, call = K.ptr, _lib.stream, _lib.call
    head = (p(x), p(t), P, C, 255, p(w))

    def step(k):
        return lambda: call("dct_topk_ce_step", *head, float(k), p(out2), p(counts4), p(vmap), None, 1.0, p(dl), 0, p(tws), tws.numel(), st())
    arms = [("ce_weighted step", lambda: call("dct_ce_weighted_step", *head, 0, p(out), None, 1.0, p(dl), 0, p(ws), ws.numel(), st()))]
    arms += [(f"topk step k={k}", step(k)) for k in (1, 10, 100)]
    arms += [("topk fwd k=10", lambda: call("dct_topk_ce_fwd", *head, 10.0, p(out2), p(counts4), p(vmap), p(tws), tws.numel(), st())),
             ("topk bwd k=10", lambda: call("dct_topk_ce_bwd", *head, p(vmap), p(out2), p(counts4), None, 1.0, p(dl), 0, st()))]
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
    base = stats(chain["ce_weighted step"])[0]
    call("dct_topk_ce_fwd", *head, 10.0, p(out2), p(counts4), p(vmap), p(tws), tws.numel(), st())
    torch.cuda.synchronize()
    print(f"P={P} C={C}: counts4 at k=10 (K, N, n_gt, n_eq) = {counts4.tolist()}, (value, tau) = {out2.tolist()}")
    for name, _ in arms:
        m1, lo1, hi1 = stats(one[name])
        m2, lo2, hi2 = stats(chain[name])
        print(f"P={P} C={C} {name}: one call between events: median {m1:.1f} us (min {lo1:.1f}, max {hi1:.1f}; {REPS} calls, arms "
              f"alternating, after {WARM} warm-up calls); graph of {CHAIN} calls: median {m2:.2f} us per call (min {lo2:.2f}, max {hi2:.2f}; "
              f"{REPS // 2} replays, arms alternating); x{m2 / base:.2f} of the ce_weighted step")
