"""``TopKCrossEntropyLoss2d`` without a device: registry, arguments, refusals, header and binding table; and tests/topk_ref.py checked
against itself -- the K formula at its edges against Python's ``int(N * k / 100)``, the reference and the header's tie rule against a
plain ``torch.topk(...).mean()`` on the planted inputs, and the plants being what their names say (the cluster's values exact in
float32, its keys apart in the last ten bits only).  The kernels: tests/test_topk_ce_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref
import topk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dct_topk_ce_fwd", "dct_topk_ce_bwd", "dct_topk_ce_step"]


def test_registry_and_arguments():
    from dct_amd import loss
    from dct_amd.loss import LOSS, TopKCrossEntropyLoss2d, get_loss_fn
    assert LOSS["topk_ce"] is TopKCrossEntropyLoss2d and loss.TopKCrossEntropyLoss2d is TopKCrossEntropyLoss2d
    w = [0.1, 1, 2.5, 0]
    crit = get_loss_fn("topk_ce", k=25, weight=w, ignore_index=7)
    assert type(crit) is TopKCrossEntropyLoss2d and crit.k == 25.0 and crit.weight is w and crit.ignore_index == 7
    d = TopKCrossEntropyLoss2d()
    assert d.k == 10.0 and d.weight is None and d.ignore_index == 255 and d.last_topk is None
    assert d.launch_args(4) == dict(k_percent=10.0) and TopKCrossEntropyLoss2d(k=100).launch_args(2) == dict(k_percent=100.0)
    assert TopKCrossEntropyLoss2d(k=0.1).launch_args(3) == dict(k_percent=0.1)
    assert TopKCrossEntropyLoss2d().device_weight("cuda:0") is None and TopKCrossEntropyLoss2d(weight=[1, 1.0]).device_weight("cuda:0", 2) is None


@pytest.mark.parametrize("k", [0, -1, 100.0001, float("nan"), float("inf"), "x", None])
def test_k_is_validated_at_construction(k):
    from dct_amd.loss import TopKCrossEntropyLoss2d, get_loss_fn
    with pytest.raises(ValueError, match="TopKCrossEntropyLoss2d: k must"):
        TopKCrossEntropyLoss2d(k=k)
    with pytest.raises(ValueError, match="TopKCrossEntropyLoss2d: k must"):
        get_loss_fn("topk_ce", k=k)


def test_weight_length_and_cpu_tensors_are_refused():
    from dct_amd.loss import TopKCrossEntropyLoss2d
    with pytest.raises(ValueError, match="TopKCrossEntropyLoss2d: 3 class weights for logits of 4 classes"):
        TopKCrossEntropyLoss2d(weight=[1, 2, 3]).device_weight("cuda:0", 4)
    for kw in (dict(), dict(k=100), dict(weight=[0.1, 1, 2.5, 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TopKCrossEntropyLoss2d(**kw)(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))


def test_header_and_binding_table_hold_the_four_functions():
    from dct_amd import _lib
    import ctypes
    with open(os.path.join(ROOT, "include", "dct.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bsize_t dct_topk_ce_workspace_bytes\s*\(\s*int64_t pixels\s*\);", code)
    assert _lib.SIGNATURES["dct_topk_ce_workspace_bytes"] == (_lib._sz, [_lib._i64])
    for name in NAMES:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, code)
        assert decl, name
        args = [a.strip() for a in decl.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib._i and len(args) == len(argtypes), (name, args)
        assert args[-1] == "dct_stream stream"
        if name != "dct_topk_ce_bwd":
            i = args.index("double k_percent")
            assert args[i - 1].startswith("const float* weight") and argtypes[i] is ctypes.c_double       # k_percent follows weight
            assert args[i + 1:i + 4] == ["float* out2", "int64_t* counts4", "float* vmap"]
        else:
            assert "double k_percent" not in args and args[6:9] == ["const float* vmap", "const float* out2", "const int64_t* counts4"]
    assert _lib.ABI_VERSION == 101 and "#define DCT_VERSION 101" in header
    for topic in ("per-image top-k", "top-k + Dice", "k_percent in device memory", "top-k of the focal map", "probabilities as"):
        assert topic in header, topic


@pytest.mark.parametrize("N", [1, 2, 9, 10, 999, 1000, 1001, 393216, 1572865, 2 ** 31 - 1])
def test_k_formula_at_the_edges(N):
    assert R.k_of(0, 10.0) == 0
    assert R.k_of(N, 100) == R.k_of(N, 100.0) == N
    assert R.k_of(N, 1e-9) == 1                               # the floor is 0: one pixel is kept
    for k in (0.1, 33.3, 10.0, 50.0, 99.999):
        K = R.k_of(N, k)
        assert K == min(N, max(1, int(N * k / 100))) and 1 <= K <= N
    if N == 1:
        assert all(R.k_of(1, k) == 1 for k in (0.1, 33.3, 100))
    if N == 1000:
        assert (R.k_of(N, 0.1), R.k_of(N, 33.3), R.k_of(N, 10)) == (1, 333, 100)
    K = max(1, N // 3)
    assert R.k_of(N, R.k_for(N, K)) == K


def _plain_topk_mean(x, t_ref, w, C, k):
    """nnU-Net's TopKLoss on the counted pixels, in float64 and independent of tests/focal_ref.py."""
    keep = t_ref != R.IGN
    v = F.cross_entropy(x.double()[keep], t_ref[keep], weight=w.double(), reduction="none")
    K = min(len(v), max(1, int(len(v) * k / 100)))
    return torch.topk(v, K).values.mean().item(), K


@pytest.mark.parametrize("P,C,k,stray,weighted,plant", [
    (257, 3, 10.0, True, True, None), (257, 4, 33.3, False, True, "tie"), (4099, 2, 10.0, False, False, "cluster"),
    (4099, 8, 100.0, True, True, None), (255, 2, 0.1, False, True, None), (300, 3, 50.0, False, True, "same"),
    (4099, 4, 10.0, False, False, "tie"), (1, 2, 10.0, False, True, None)])
def test_reference_is_the_plain_topk_mean(P, C, k, stray, weighted, plant):
    w = focal_ref.weights(C) if weighted else torch.ones(C)
    _, x, t, t_ref, sen, idx = R.inputs(P, C, w, stray, seed=3 + P + C, plant=plant, k=k)
    keep = t_ref != R.IGN
    if plant == "cluster":
        k = R.k_for(int(keep.sum()), len(sen) + R.CLUSTER // 2)
    r = R.Ref(x, t_ref, w, C, k)
    want, K = _plain_topk_mean(x, t_ref, w, C, k)
    assert (r.K, r.N) == (K, int(keep.sum()))
    np.testing.assert_allclose(r.value.item(), want, rtol=1e-12, atol=1e-12)
    # the header's value under its tie rule is that mean, whatever the ties are
    K2, N2, tau, n_gt, n_eq, a = R.selection(r.v, keep, k)
    assert (K2, N2) == (K, r.N) and tau.item() == r.tau
    v = r.v
    formula = (v[keep & (v > tau)].sum() + (K - n_gt) * tau) / K
    np.testing.assert_allclose(formula.item(), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a.sum().item(), K, rtol=1e-12)            # the ties share exactly what is left
    assert not a[~keep].any()
    if plant == "tie":
        assert n_eq == len(idx) >= 2 and 0 < K - n_gt < n_eq                 # the K-th falls strictly inside the group
        assert bool((a[idx] == (K - n_gt) / n_eq).all())
    if plant == "same":
        assert n_gt == 0 and n_eq == r.N == P and bool((a == K / P).all())
    if plant == "cluster":
        assert r.v[idx].min().item() < r.tau < r.v[idx].max().item()
    if weighted and k == 100.0:
        zero = keep & (r.r.wi == 0)
        assert zero.any() and tau.item() == 0.0 and n_eq == int(zero.sum()) and K - n_gt == n_eq     # the mass tie at 0 straddles K


def test_cluster_values_are_exact_in_float32_and_differ_in_the_last_digits():
    """v_j = D_j + log(1 + exp(-D_j)) = D_j: in float32 the softmax of (-D, 0) is (0, 1), log 1 = 0, and 0 - (-D) is exact.  The 300
    keys share their top 22 bits, so only the select's last pass tells them apart."""
    w = torch.ones(2)
    _, x, t, t_ref, sen, idx = R.inputs(4099, 2, w, False, seed=1, plant="cluster")
    f32, _, _, _ = focal_ref.restate32(x, t_ref, w, 0.0)
    D = 1000.0 + torch.arange(R.CLUSTER, dtype=torch.float64) * R.ULP_1000
    assert torch.equal(f32[idx].double(), D)
    l32 = torch.logsumexp(x[idx], 1) - x[idx, 0]
    assert torch.equal(l32.double(), D)
    bits = f32[idx].view(torch.int32)
    assert len(set((bits >> 10).tolist())) == 1 and len(set((bits & 1023).tolist())) == R.CLUSTER
    r = R.Ref(x, t_ref, w, 2, 10.0)
    np.testing.assert_allclose(r.v[idx].numpy(), D.numpy(), rtol=1e-15)


def test_k_100_without_weights_is_the_mean_cross_entropy():
    w = torch.ones(3)
    _, x, t, t_ref, _, _ = R.inputs(257, 3, w, True, seed=5)
    r = R.Ref(x, t_ref, w, 3, 100.0)
    want = F.cross_entropy(x.double(), t_ref, ignore_index=R.IGN)
    np.testing.assert_allclose(r.value.item(), want.item(), rtol=1e-12)
    # with weights it is sum w l / N, not / sum w
    w = focal_ref.weights(3)
    r = R.Ref(x, t_ref, w, 3, 100.0)
    np.testing.assert_allclose(r.value.item(), r.v.sum().item() / r.N, rtol=1e-12)
