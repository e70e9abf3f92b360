#!/usr/bin/env python3
"""The VAT launches (dct_vat_noise, dct_vat_sumsq, dct_vat_perturb with and without r_out) beside dct_fgsm_step on the same tensors at
16 x 1 x 256 x 256 and 16 x 1 x 200 x 200: device time between events around a captured graph of 20 calls per arm, arms alternating,
median (min - max) per call and the bytes each moves.  With --step: a cfg3-shaped step (2 x UNet bf16, 256 x 256, C = 4, 8 + 8 images,
JSD + adversarial term) with generator 'vat' (ip = 1; expected: one more forward and one more input-gradient pass of model b) against
the same step with FGSM, trainers alternating (`profiles/vat.txt`)."""
import argparse
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from dct_amd import hip_ops as K

dev = "cuda:0"
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--step", action="store_true", help="also time the cfg3-shaped step with VAT against FGSM")
ap.add_argument("--steps", type=int, default=30)
args = ap.parse_args()
CHAIN = 20


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


for N, H in ((16, 256), (16, 200)):
    g = torch.Generator(device=dev).manual_seed(H)
    x = torch.rand(N, 1, H, H, device=dev, generator=g)
    gr_ = torch.randn(N, 1, H, H, device=dev, generator=g)
    d = torch.empty_like(x)
    calls = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = K.vat_workspace(N, H * H, dev)
    mb = x.numel() * 4 / 1e6
    arms = (("dct_vat_noise", lambda: K.vat_noise(d, 1234, calls=calls, workspace=ws), 1),
            ("dct_vat_sumsq", lambda: K.vat_sumsq(gr_, ws), 1),
            ("dct_vat_perturb (x_out)", lambda: K.vat_perturb(x, gr_, 7.68, ws, want_r=False), 3),
            ("dct_vat_perturb (x_out, r_out)", lambda: K.vat_perturb(x, gr_, 7.68, ws), 4),
            ("dct_fgsm_step (x_adv, noise)", lambda: K.fgsm_step(x, gr_, 0.03), 4))
    K.vat_sumsq(gr_, ws)
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn, _ in arms:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(gr, stream=side):
                for _ in range(CHAIN):
                    fn()
        graphs[name] = gr
    torch.cuda.synchronize()
    K.vat_sumsq(gr_, ws)                # (the noise arm's partials are d's: the perturb arms read gr_'s)
    for _ in range(5):
        for name, _, _ in arms[1:]:
            graphs[name].replay()
    torch.cuda.synchronize()
    chain = {name: [] for name, _, _ in arms}
    for _ in range(args.reps):
        for name, _, _ in arms[1:]:
            chain[name].append(timed(graphs[name].replay) / CHAIN)
    for _ in range(args.reps):          # the noise arm last: it overwrites the partials
        chain[arms[0][0]].append(timed(graphs[arms[0][0]].replay) / CHAIN)
    for name, _, tensors in arms:
        m, lo, hi = stats(chain[name])
        print(f"{N}x1x{H}x{H} {name}: median {m:.2f} us per call (min {lo:.2f}, max {hi:.2f}; graph of {CHAIN} calls, {args.reps} replays) "
              f"= {tensors * mb / m:.2f} TB/s of the {tensors * mb:.1f} MB it moves")

if args.step:
    import math
    import bench
    cfg = dict(bench.CONFIGS["cfg3"])
    e = 0.03 * math.sqrt(cfg["H"] * cfg["H"])
    trainers = {}
    # (FGSM's default route here is the adversarial-chain layout; "fgsm, sequential" is FGSM on the layout VAT takes)
    for name, dct in (("fgsm", {"eplision": 0.03}), ("fgsm, sequential", {"eplision": 0.03}),
                      ("vat", {"generator": "vat", "eplision": e, "xi": e, "ip": 1})):
        tr, lab, unl = bench.make_trainer(cfg, torch.bfloat16, torch.device(dev), 0, 1, None)
        tr.adv_training_dict = dct
        if name.endswith("sequential"):
            tr.adv_chain_layout = False
        trainers[name] = (tr, lab, unl)

    def step(name, k):
        tr, lab, unl = trainers[name]
        lb = [(lab[i][k % len(lab[i])][0][0], lab[i][k % len(lab[i])][0][1]) for i in range(cfg["S"])]
        u = unl[k % len(unl)][0]
        return tr._run_step(lb, (u[0], u[1]), True, True, (0, 1))
    for k in range(6):                  # warm-up, capture, first replays
        for name in trainers:
            step(name, k)
    torch.cuda.synchronize()
    times = {name: [] for name in trainers}
    for k in range(args.steps):
        for name in trainers:
            times[name].append(timed(lambda: step(name, k)) / 1e3)
    for name, (tr, _, _) in trainers.items():
        m, lo, hi = stats(times[name])
        sg = tr._step_graphs
        print(f"cfg3-shaped step, generator {name}: median {m:.3f} ms (min {lo:.3f}, max {hi:.3f}; {args.steps} steps, trainers alternating), "
              f"route {tr.last_route.kind}, captures {sg.captures if sg else 0}, replays {sg.replays if sg else 0}")
