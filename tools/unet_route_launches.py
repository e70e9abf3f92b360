"""What one UNet forward + backward pass launches and computes under every layout setting: per-class launch counts of the library's
profiler (_lib.prof_read) and digests of the logits and of the flat gradient buffer, at 1x1x176x176, C = 3, bf16 and fp32.

It drives plan_forward / plan_backward and the switch attributes only, so it runs on any commit that has them: two commits compute
and launch the same when their outputs are equal line for line (profiles/unet_route_refactor.txt).

    python tools/unet_route_launches.py
"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dct_amd import _lib  # noqa: E402
from dct_amd.arch import get_arch  # noqa: E402

DEV = "cuda:0"
# the switches that are on by default, each turned off alone; wgrad_side_stream, off by default, is turned on alone
SWITCHES = ("relu_bits", "pool_codes", "fuse_pool", "pool_only", "fuse_drop_pool", "batch_skip_resize", "late_packs",
            "fuse_skip_grad", "fuse_stem_wgrad", "batch_bias_grads")


def digest(t):
    return hashlib.sha1(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def one(name, dtype, x, gl, attrs=(), train=True, need_dx=False, reuse=False):
    torch.manual_seed(41)
    net = get_arch("unet", {"num_classes": 3, "compute_dtype": dtype, "dropout_p": 0.5}).to(DEV)
    net.train(train)
    net.dropout_seed = 83
    for k, v in dict(attrs).items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    torch.cuda.synchronize()
    _lib.prof_read(reset=True)
    _lib.prof_enable(True)
    logits, tape = net.plan_forward(x, True, keep_predrop=reuse)
    if reuse:
        logits, tape = net.plan_forward(x, True, reuse=tape)
    dx = net.plan_backward(tape, gl, need_dx=need_dx, need_dw=True, overwrite=True)
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    counts = {k: v["launches"] for k, v in _lib.prof_read(reset=True).items()}
    line = f"{str(dtype).split('.')[1]:8s} {name:28s} | launches {counts} | logits {digest(logits)} grads {digest(net.flat_params.gflat)}"
    if dx is not None:
        line += f" dx {digest(dx)}"
    if "record_dropout_masks" in dict(attrs):
        line += f" masks {' '.join(digest(m) for m in net.last_dropout_masks)}"
    print(line, flush=True)


def main():
    assert torch.cuda.is_available(), "needs the HIP device"
    x = torch.rand(1, 1, 176, 176, generator=torch.Generator().manual_seed(86)).to(DEV)
    gl = torch.randn(1, 176, 176, 3, generator=torch.Generator().manual_seed(87)).to(DEV)
    for dtype in (torch.bfloat16, torch.float32):
        one("defaults", dtype, x, gl)
        for k in SWITCHES:
            one(f"{k}=0", dtype, x, gl, attrs={k: False})
        one("wgrad_side_stream=1", dtype, x, gl, attrs={"wgrad_side_stream": True})
        one("record_dropout_masks", dtype, x, gl, attrs={"record_dropout_masks": True})
        one("eval mode", dtype, x, gl, train=False)
        one("need_dx", dtype, x, gl, need_dx=True)
        one("reuse of a kept tape", dtype, x, gl, reuse=True)
        one("reuse of a kept tape, need_dx", dtype, x, gl, need_dx=True, reuse=True)


if __name__ == "__main__":
    main()
