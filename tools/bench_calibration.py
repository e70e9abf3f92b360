#!/usr/bin/env python3
"""Device time of the bare dct_calibration_counts launch beside the bare dct_confusion_counts launch on the SAME inputs (the yardstick:
comparable traffic, (4 C S + 8) bytes per pixel, and the same wave-aggregation problem), at the eval shape 8 x 256 x 256, C = 4, two
views (+ their mean for the calibration tables; + gt for the confusion matrices): on noise (softmax of Gaussian logits, the
confidences spread over the bins) and on a peaked map (blobs, > 90 % of the pixels in the top bin).  Windows of N launches between
two events, the two kernels alternating window by window, output buffers zeroed outside the windows; prints the median window
per launch, the bytes moved and the achieved bandwidth."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
B, C, H, S, NB = 8, 4, 256, 2, 15
N, WINDOWS = 200, 7


def blobs(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.randn(B, C, H, H, device=dev, generator=g)
    for _ in range(8):          # smoothed noise: the argmax is a map of blobs
        f = torch.nn.functional.avg_pool2d(f, 5, stride=1, padding=2, count_include_pad=False)
    return f.permute(0, 2, 3, 1).contiguous()


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / N


torch.manual_seed(0)
cases = {}
cases["noise"] = ([torch.softmax(2 * torch.randn(B, H, H, C, device=dev), -1).contiguous() for _ in range(S)],
                  torch.randint(0, C, (B, H * H), device=dev))
hard = blobs(1).argmax(-1)      # both views say the blob map, confidently and rightly: the mean of the two lands in the top bin as well
cases["peaked"] = ([torch.softmax(9 * torch.nn.functional.one_hot(hard, C).float() + 0.5 * torch.randn(B, H, H, C, device=dev), -1).contiguous()
                    for _ in range(S)], hard.reshape(B, -1).contiguous())
nbytes = (4 * C * S + 8) * B * H * H
for name, (ps, gt) in cases.items():
    bins, _ = K.calibration_counts(ps, gt, n_bins=NB, with_ensemble=True)
    share = bins[:, :, NB - 1, 0].sum().item() / max(1, bins[..., 0].sum().item())
    arr = K._ptr_array(ps)
    cal_b = torch.zeros(B, S + 1, NB, 3, dtype=torch.int64, device=dev)
    cal_s = torch.zeros(B, S + 1, 2, dtype=torch.int64, device=dev)
    cnf = torch.zeros(B, (S + 1) * S // 2, C, C, dtype=torch.int32, device=dev)
    st = _lib.stream()
    legs = {"dct_calibration_counts": lambda: _lib.call("dct_calibration_counts", arr, S, gt.data_ptr(), B, H * H, C, NB, (1 << C) - 1, 1, 0,
                                                         cal_b.data_ptr(), cal_s.data_ptr(), st),
            "dct_confusion_counts": lambda: _lib.call("dct_confusion_counts", arr, S, gt.data_ptr(), B, H * H, C, cnf.data_ptr(), st)}
    times = {k: [] for k in legs}
    for k, fn in legs.items():      # warm-up
        window(fn)
    for _ in range(WINDOWS):
        for k, fn in legs.items():
            cal_b.zero_(); cal_s.zero_(); cnf.zero_()
            times[k].append(window(fn))
    for k, ts in times.items():
        ts.sort()
        med = ts[len(ts) // 2]
        print(f"{B}x{H}x{H} C={C} S={S} {name} (top-bin share {share:.3f}): {k}: median {med:.2f} us per launch (min {ts[0]:.2f}, max {ts[-1]:.2f}; "
              f"{WINDOWS} windows of {N} launches, events), {nbytes / 1e6:.2f} MB -> {nbytes / med / 1e3:.0f} GB/s")
