#!/usr/bin/env python3
"""dct_mse_logits_step (softmax-MSE consistency of the step: masks, value, kept fraction, softmax maps and logit gradients in one pass
+ a finalize) beside (a) dct_pl_logits_step, the hard pseudo-label step, and dct_jsd_logits_step on the same tensors -- the same bytes
move, S x 4 C read and 2 S x 4 C written per pixel; the MSE step has no logarithm and no division per class -- and (b) the same loss
and gradient composed from torch device ops with autograd (softmax, detach, max, mask, squared difference, backward): what a user had
before.  Shapes: 8 x 256 x 256 x 4 with S = 2 (cfg2's unlabeled batch) and 16 x 200 x 200 x 2 with S = 2 (B x H x W x C); both
teachers, threshold 0 and 0.6.  Method as tools/bench_soft_label.py: a captured graph of 20 calls per window between two events, arms
alternating in one process, 50 windows, median (min - max); launch counts from the library's own launch counter (dct_prof_read) for its
arms, torch.profiler's kernel events for the composition.  Every MSE arm's median is stated against the hard step's min - max of the
same teacher and threshold."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
WINDOWS, WARM, CHAIN = 50, 20, 20
EPS = 1e-10


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


def torch_mse(xs, teacher, tau):
    """The rule of include/dct.h from torch device ops; xs: S logit maps [P, C] requiring grad.  -> mean over all pixels"""
    S = len(xs)
    ps = [torch.softmax(x, -1) for x in xs]
    with torch.no_grad():
        ts = [p.detach() for p in ps] if teacher == K.PL_CROSS else [sum(ps) / S]
        ms = [(t.max(-1).values >= tau).to(t.dtype) for t in ts]
    total = 0.0
    for i in range(S):
        if teacher == K.PL_CROSS:
            li = sum(ms[j] * ((ps[i] - ts[j]) ** 2).mean(-1) for j in range(S) if j != i) / (S - 1)
        else:
            li = ms[0] * ((ps[i] - ts[0]) ** 2).mean(-1)
        total = total + li
    return (total / S).mean()


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


for B, H, C, S in ((8, 256, 4, 2), (16, 200, 2, 2)):
    P = B * H * H
    g = torch.Generator(device=dev).manual_seed(P + C)
    xs = [torch.randn(P, C, device=dev, generator=g) * 3 for _ in range(S)]
    dls = [torch.empty_like(x) for x in xs]
    prs = [torch.empty_like(x) for x in xs]
    out1, out2, ws = torch.empty(1, device=dev), torch.empty(2, device=dev), K._loss_ws(dev)
    xa, da, pa = K._ptr_array(xs), K._ptr_array(dls), K._ptr_array(prs)
    p = K.ptr

    def jsd():
        _lib.call("dct_jsd_logits_step", xa, S, P, C, p(out1), pa, None, 1.0, da, 0, p(ws), ws.numel(), _lib.stream())

    def pl(teacher, tau):
        def run():
            _lib.call("dct_pl_logits_step", xa, S, teacher, tau, EPS, P, C, p(out2), pa, None, 1.0, da, 0, p(ws), ws.numel(), _lib.stream())
        return run

    def mse(teacher, tau):
        def run():
            _lib.call("dct_mse_logits_step", xa, S, teacher, tau, P, C, p(out2), pa, None, 1.0, da, 0, p(ws), ws.numel(), _lib.stream())
        return run
    xr = [x.clone().requires_grad_(True) for x in xs]

    def composed(teacher, tau):
        def run():
            for x in xr:
                x.grad = None
            torch_mse(xr, teacher, tau).backward()
        return run
    modes = (("cross", K.PL_CROSS), ("ensemble", K.PL_ENSEMBLE))
    hard = {(n, tau): f"dct_pl_logits_step {n} tau={tau}" for n, _ in modes for tau in (0.0, 0.6)}
    lib_arms = (("dct_jsd_logits_step", jsd),) + tuple((hard[(n, tau)], pl(t, tau)) for n, t in modes for tau in (0.0, 0.6))
    new = {}
    for n, t in modes:
        for tau in (0.0, 0.6):
            name = f"dct_mse_logits_step {n} tau={tau}"
            new[name] = hard[(n, tau)]
            lib_arms += ((name, mse(t, tau)),)
    torch_arms = tuple((f"torch composition {n} tau=0.6", composed(t, 0.6)) for n, t in modes)
    for _ in range(WARM):
        for _, fn in lib_arms + torch_arms:
            fn()
    torch.cuda.synchronize()
    # the composition and the kernel compute the same thing.  torch's softmax and the kernel's differ in the last bits, so a teacher whose
    # confidence lies within rounding of the threshold is kept by one and masked by the other: counted apart from the rest, which must
    # agree to rounding.
    for n, t in modes:
        composed(t, 0.6)()
        mse(t, 0.6)()
        torch.cuda.synchronize()
        gmax = max(x.grad.abs().max().item() for x in xr)
        off = [((x.grad - d).abs().max(-1).values > 1e-3 * gmax) for x, d in zip(xr, dls)]
        flipped = int(torch.stack(off).any(0).sum())
        rest = max(((x.grad - d).abs().max(-1).values * (~o)).max().item() for x, d, o in zip(xr, dls, off)) / gmax
        assert flipped <= 8 and rest < 1e-3, (n, flipped, rest)
        print(f"B={B} HxW={H}x{H} C={C} S={S} {n} tau=0.6: value {out2[0].item():.6f} (at most 2 / C = {2.0 / C}); kept fraction "
              f"{out2[1].item():.3f}; pixels whose teacher the torch composition keeps and dct_mse_logits_step masks or the reverse: {flipped} "
              f"of {P}; elsewhere max |torch gradient - kernel gradient| / max |gradient| = {rest:.2e}", flush=True)
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
    one = {name: [] for name, _ in torch_arms}
    for _ in range(WINDOWS):
        for name, _ in lib_arms:
            chain[name].append(timed(graphs[name].replay) / CHAIN)
        for name, fn in torch_arms:
            one[name].append(timed(fn))
    mb = P * S * 3 * 4 * C / 1e6
    for name, fn in lib_arms:
        m2, lo2, hi2 = stats(chain[name])
        line = (f"B={B} HxW={H}x{H} C={C} S={S} {name}: graph of {CHAIN} calls: median {m2:.2f} us per call (min {lo2:.2f}, max {hi2:.2f}; "
                f"{WINDOWS} windows) = {mb / m2:.2f} TB/s of the {mb:.1f} MB a call moves; launches per call: {launches(fn)}")
        if name in new:
            hm, hlo, hhi = stats(chain[new[name]])
            where = "inside" if hlo <= m2 <= hhi else f"outside ({'above the max' if m2 > hhi else 'below the min'} by {abs(m2 - (hhi if m2 > hhi else hlo)):.2f} us)"
            line += f"; {m2 / hm:.3f} x the hard step's median {hm:.2f} us, {where} its min - max {hlo:.2f} - {hhi:.2f}"
        print(line, flush=True)
    for name, fn in torch_arms:
        m1, lo1, hi1 = stats(one[name])
        print(f"B={B} HxW={H}x{H} C={C} S={S} {name}: one call between events: median {m1:.1f} us (min {lo1:.1f}, max {hi1:.1f}; {WINDOWS} "
              f"calls); launches per call (forward + backward): {torch_launches(fn)}", flush=True)
