#!/usr/bin/env python3
"""Where the in-step meters' time goes (diagnostic): DiceMeter.add / value on bench-shaped predictions, host and device time; then
one HausdorffMeter.add (2-D and 3-D) and one AgreementMeter.add (2 and 4 models with gt) beside one DiceMeter.add on the same
16 x 4 x 256 x 256 batch, device time between events; and the bare dct_confusion_counts launch for 2 models + gt beside the two
dct_dice_counts launches that read the same bytes."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from dct_amd import hip_ops as K
from dct_amd.metrics import AgreementMeter, DiceMeter, HausdorffMeter
dev = "cuda:0"
B, C, H = 8, 4, 256
pred = torch.randn(B, H, H, C, device=dev).permute(0, 3, 1, 2)
gt = torch.randint(0, C, (B, 1, H, H), device=dev)
m = DiceMeter(method="2d", report_axises=[1, 2, 3], C=C)
for _ in range(5):
    m.add(pred, gt)
torch.cuda.synchronize()
for n, what in ((200, "add"), (50, "add+value")):
    t0 = time.perf_counter()
    for _ in range(n):
        m.add(pred, gt)
        if what != "add":
            float(m.value()[0][0])
    th = time.perf_counter() - t0
    torch.cuda.synchronize()
    td = time.perf_counter() - t0
    print(f"{what}: host {1e6 * th / n:.1f} us/call, host+device {1e6 * td / n:.1f} us/call")

x = torch.zeros(4, device=dev)
torch.cuda.synchronize()
for what, fn in (("synchronize()", lambda: torch.cuda.synchronize()), (".item()", lambda: x[0].item()), (".cpu()", lambda: x.cpu()),
                 ("double ops + item", lambda: ((x.double() / 3).sqrt().float())[0].item())):
    t0 = time.perf_counter()
    for _ in range(50):
        x.add_(1.0)
        fn()
    print(f"{what}: {1e6 * (time.perf_counter() - t0) / 50:.1f} us per (tiny kernel + call)")


# ---- one add in isolation, device time (events around each call, warm-up first, median of 20) ----------------------------------
def blobs(B, C, H, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.randn(B, C, H, H, device=dev, generator=g)
    for _ in range(8):          # smoothed noise: the argmax is a map of blobs
        f = torch.nn.functional.avg_pool2d(f, 5, stride=1, padding=2, count_include_pad=False)
    return f


def event_us(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(1e3 * a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


B, C, H = 16, 4, 256
for name, preds, gt in (("blobs", [blobs(B, C, H, 1 + 10 * s) for s in range(4)], blobs(B, C, H, 2).max(1, keepdim=True)[1]),
                        ("noise", [torch.randn(B, C, H, H, device=dev) for _ in range(4)], torch.randint(0, C, (B, 1, H, H), device=dev))):
    pred = preds[0]
    legs = [("DiceMeter.add 2d", DiceMeter(method="2d", report_axises=[1, 2, 3], C=C), lambda m: m.add(pred, gt)),
            ("HausdorffMeter.add 2d", HausdorffMeter(method="2d", report_axises=[1, 2, 3], C=C), lambda m: m.add(pred, gt)),
            ("HausdorffMeter.add 3d", HausdorffMeter(method="3d", report_axises=[1, 2, 3], C=C), lambda m: m.add(pred, gt)),
            ("AgreementMeter.add 2d, 2 models + gt", AgreementMeter(method="2d", C=C, n_models=2), lambda m: m.add(preds[:2], gt)),
            ("AgreementMeter.add 2d, 4 models + gt", AgreementMeter(method="2d", C=C, n_models=4), lambda m: m.add(preds, gt))]
    for what, meter, add in legs:
        med, lo, hi = event_us(lambda: add(meter))
        meter.reset()
        print(f"{B}x{C}x{H}x{H} {name}: {what}: median {med:.1f} us (min {lo:.1f}, max {hi:.1f}; 20 calls, events, after 5 warm-up calls)")
    # the counting launches alone, on NHWC copies made beforehand: (16 S + 8) bytes per pixel in one launch against 24 in each of S
    nhwc = [p.permute(0, 2, 3, 1).contiguous() for p in preds]
    g = gt.reshape(B, -1).contiguous()
    for what, fn in (("dct_confusion_counts, 2 models + gt (1 launch + zeroing)", lambda: K.confusion_counts(nhwc[:2], g)),
                     ("dct_confusion_counts, 4 models + gt (1 launch + zeroing)", lambda: K.confusion_counts(nhwc, g)),
                     ("dct_dice_counts x 2 (2 launches + zeroing)", lambda: [K.dice_counts(x, g, B, C) for x in nhwc[:2]])):
        med, lo, hi = event_us(fn)
        print(f"{B}x{C}x{H}x{H} {name}: {what}: median {med:.1f} us (min {lo:.1f}, max {hi:.1f}; 20 calls, events, after 5 warm-up calls)")
