#!/usr/bin/env python3
"""Device time of the bare dct_temperature_sums launch at the eval shape 8 x 256 x 256, C = 4, two views + their mean, K = 16 candidates
per rater, beside (a) the torch composition on the SAME tensors -- F.cross_entropy(beta * z, y, reduction='sum') per rater and candidate,
48 calls, the mean's logits formed once outside the windows -- and (b) the bare dct_calibration_counts launch (from_logits, 15 bins), the
HBM-bound yardstick that reads the same (4 C S + 8) bytes per pixel.  Windows of N launches between two events, the arms alternating
window by window, output buffers zeroed outside the windows; prints the median window per launch (per pass of 48 calls for torch) and the
transcendentals per pixel."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from dct_amd import _lib, hip_ops as K

dev = "cuda:0"
B, C, H, S, NK, NB = 8, 4, 256, 2, 16, 15
R = S + 1
N, WINDOWS = 50, 7


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


torch.manual_seed(0)
zs = [(2 * torch.randn(B, H, H, C, device=dev)).contiguous() for _ in range(S)]
gt = torch.randint(0, C, (B, H * H), device=dev)
betas = torch.exp2(torch.linspace(-4, 4, NK, device=dev)).repeat(R, 1).contiguous()
arr = K._ptr_array(zs)
st = _lib.stream()
sums = torch.zeros(R, NK, 2, dtype=torch.int64, device=dev)
cnt = torch.zeros(1, dtype=torch.int64, device=dev)
cal_b = torch.zeros(B, R, NB, 3, dtype=torch.int64, device=dev)
cal_s = torch.zeros(B, R, 2, dtype=torch.int64, device=dev)
# the torch arm's inputs: [P, C] logits of the three raters (the mean's formed once, outside the timing) and the candidates on the host
p_ens = sum(torch.softmax(z, -1) for z in zs) / S
flat = [z.reshape(-1, C) for z in zs] + [torch.log(p_ens + 1e-10).reshape(-1, C)]
y = gt.reshape(-1)
host_betas = betas.cpu().tolist()
sink = [None] * (R * NK)


def torch_pass():
    for r in range(R):
        for k in range(NK):
            sink[r * NK + k] = F.cross_entropy(host_betas[r][k] * flat[r], y, reduction='sum')


legs = {"dct_temperature_sums": (lambda: _lib.call("dct_temperature_sums", arr, S, gt.data_ptr(), B, H * H, C, (1 << C) - 1, 1, betas.data_ptr(), NK,
                                                    sums.data_ptr(), cnt.data_ptr(), st), N),
        "torch cross_entropy x 48": (torch_pass, max(1, N // 10)),
        "dct_calibration_counts": (lambda: _lib.call("dct_calibration_counts", arr, S, gt.data_ptr(), B, H * H, C, NB, (1 << C) - 1, 1, 1,
                                                      cal_b.data_ptr(), cal_s.data_ptr(), st), N)}
# the two arms agree on what they compute
legs["dct_temperature_sums"][0]()
torch_pass()
torch.cuda.synchronize()
mine = sums[..., 0].double() / (1 << 20)
theirs = torch.stack(sink).reshape(R, NK).double()
print(f"largest relative difference of the NLL sums, kernel against torch: {float(((mine - theirs).abs() / theirs).max()):.2e}")
times = {k: [] for k in legs}
for k, (fn, n) in legs.items():      # warm-up
    window(fn, n)
for _ in range(WINDOWS):
    for k, (fn, n) in legs.items():
        sums.zero_(); cnt.zero_(); cal_b.zero_(); cal_s.zero_()
        times[k].append(window(fn, n))
nbytes = (4 * C * S + 8) * B * H * H
trans = R * NK * (C + 1) + (NK // 4) * (S * C + C)        # per pixel: C expf + 1 logf per rater and candidate; the mean once per chunk of four
for k, ts in times.items():
    ts.sort()
    med = ts[len(ts) // 2]
    print(f"{B}x{H}x{H} C={C} S={S}+mean K={NK}: {k}: median {med:.1f} us (min {ts[0]:.1f}, max {ts[-1]:.1f}; {WINDOWS} windows of {legs[k][1]}, events), "
          f"{nbytes / 1e6:.2f} MB -> {nbytes / med / 1e3:.0f} GB/s")
med = sorted(times["dct_temperature_sums"])[WINDOWS // 2]
print(f"transcendentals per pixel {trans}: {trans * B * H * H / med / 1e3:.1f} G per second over the launch")
