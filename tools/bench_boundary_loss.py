#!/usr/bin/env python3
"""The boundary loss's device chain beside what it replaces and beside its floor, at B = 8 and 16, 256 x 256, C = 4, foreground classes,
on blob-structured labels (background plus one to three ellipses per foreground class):
  (a) dct_signed_distance: targets -> the fp32 [B, H, W, C] signed distance maps (three launches);
  (b) dct_boundary_fwd + dct_boundary_bwd on those maps (three launches);
  (c) dct_ce_weighted_step on the same logits and targets -- the floor of a loss pass over these tensors;
  (d) the route a user had: labels to the host, scipy.ndimage.distance_transform_edt per slice and class (Kervadec's one_hot2dist),
      the float maps back to the device.  Host wall time around a synchronised call, since the work is on the host.
Device time between events for (a) - (c), arms alternating in one process, one call per window and a captured graph of 20 calls per
window.  Also prints the maximum difference of the device maps to the scipy maps."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
REPS, WARM, CHAIN, HOST_REPS = 100, 10, 20, 5
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


def blob_labels(B, H, W, C, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    gt = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for c in range(1, C):
            for _ in range(rng.randint(1, 4)):
                cy, cx = rng.randint(H // 6, 5 * H // 6), rng.randint(W // 6, 5 * W // 6)
                ry, rx = rng.randint(H // 24, H // 6), rng.randint(W // 24, W // 6)
                gt[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = c
    return gt


def scipy_maps(gt, C, classes):
    """one_hot2dist per slice and class with the zero rule of include/dct.h -> float32 [B, H, W, C]"""
    from scipy.ndimage import distance_transform_edt as edt
    B, H, W = gt.shape
    out = np.zeros((B, H, W, C), np.float32)
    for b in range(B):
        for c in classes:
            m = gt[b] == c
            if 0 < m.sum() < m.size:
                out[b, :, :, c] = np.where(m, -(edt(m) - 1.0), edt(~m))
    return out


for B in (8, 16):
    H = W = 256
    C, classes = 4, [1, 2, 3]
    P = B * H * W
    mask = sum(1 << c for c in classes)
    t = torch.from_numpy(blob_labels(B, H, W, C, B)).to(dev)
    g = torch.Generator(device=dev).manual_seed(P)
    x = torch.randn(B, H, W, C, device=dev, generator=g) * 2
    w = torch.tensor([0.1, 1.0, 2.5, 1.5], device=dev)
    phi, dl, out2 = torch.empty(B, H, W, C, device=dev), torch.empty_like(x), torch.empty(2, device=dev)
    lib = _lib.load()
    wsd = torch.empty(lib.dct_signed_distance_workspace_bytes(B, H, W, C), dtype=torch.uint8, device=dev)
    ws = K._loss_ws(dev)
    p = K.ptr

    def chain():
        _lib.call("dct_signed_distance", p(t), B, H, W, C, mask, 1.0, 1.0, p(phi), p(wsd), wsd.numel(), _lib.stream())

    def pair():
        _lib.call("dct_boundary_fwd", p(x), p(t), p(phi), P, C, IGN, mask, p(out2), p(ws), ws.numel(), _lib.stream())
        _lib.call("dct_boundary_bwd", p(x), p(t), p(phi), P, C, IGN, mask, p(out2[1:2]), None, 1.0, p(dl), 0, _lib.stream())

    def floor():
        _lib.call("dct_ce_weighted_step", p(x), p(t), P, C, IGN, p(w), 0, p(out2), None, 1.0, p(dl), 0, p(ws), ws.numel(), _lib.stream())

    def host_route():
        return torch.from_numpy(scipy_maps(t.cpu().numpy(), C, classes)).to(dev)

    arms = (("dct_signed_distance (the chain)", chain), ("dct_boundary_fwd + _bwd", pair), ("dct_ce_weighted_step (floor)", floor))
    for _ in range(WARM):
        for _, fn in arms:
            fn()
    torch.cuda.synchronize()
    ref = host_route()
    diff = (phi - ref).abs().max().item()
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
    for _ in range(3):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    chained = {name: [] for name, _ in arms}
    for _ in range(REPS // 4):
        for name, _ in arms:
            chained[name].append(timed(graphs[name].replay) / CHAIN)
    host = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_route()
        torch.cuda.synchronize()
        host.append(1e6 * (time.perf_counter() - t0))
    for name, _ in arms:
        m1, lo1, hi1 = stats(one[name])
        m2, lo2, hi2 = stats(chained[name])
        print(f"B={B} {H}x{W} C={C} classes={classes} {name}: one call between events: median {m1:.1f} us (min {lo1:.1f}, max {hi1:.1f}; {REPS} calls); "
              f"graph of {CHAIN} calls: median {m2:.1f} us per call (min {lo2:.1f}, max {hi2:.1f}; {REPS // 4} replays)", flush=True)
    mh, loh, hih = stats(host)
    print(f"B={B} {H}x{W} C={C} classes={classes} labels to host + scipy edt per slice and class + maps to device: host wall median {mh:.0f} us "
          f"(min {loh:.0f}, max {hih:.0f}; {HOST_REPS} calls)", flush=True)
    print(f"B={B} {H}x{W} C={C}: max |device phi - scipy phi| = {diff:.3e} (unit spacing: expected 0)", flush=True)
