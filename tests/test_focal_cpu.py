"""``FocalLoss2d`` without a device: registry, arguments, refusals, header and binding table; and tests/focal_ref.py checked against
itself -- the float64 reference against torch's cross entropy at gamma = 0, its autograd gradient against the closed form of
include/dct.h, and the derived bounds against the float32 restatement on the inputs of tests/test_focal_gpu.py (the pixel counts below
a million): a correct fp32 evaluation of the rule stays inside them.  The kernels: tests/test_focal_gpu.py."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dct_focal_fwd", "dct_focal_bwd", "dct_focal_step", "dct_focal_map_fwd", "dct_focal_map_bwd"]


def test_registry_and_arguments():
    from dct_amd import loss
    from dct_amd.loss import LOSS, FocalLoss2d, get_loss_fn
    assert LOSS["focal"] is FocalLoss2d and loss.FocalLoss2d is FocalLoss2d
    w = [0.1, 1, 2.5, 0]
    crit = get_loss_fn("focal", gamma=1.5, weight=w, ignore_index=7)
    assert type(crit) is FocalLoss2d and crit.gamma == 1.5 and crit.weight is w and crit.ignore_index == 7 and crit.reduction == "mean"
    d = FocalLoss2d()
    assert d.gamma == 2.0 and d.weight is None and d.ignore_index == 255 and d.reduction == "mean"
    assert FocalLoss2d(reduce=False).reduction == "none" and FocalLoss2d(reduce=False, size_average=False).reduction == "none"
    assert FocalLoss2d(size_average=False).reduction == "sum"
    assert FocalLoss2d(gamma=0).launch_args(4) == dict(gamma=0.0) and FocalLoss2d(gamma=5).launch_args(2) == dict(gamma=5.0)
    # the device copy of the weights is _ClassWeighted's: none before the first call, none at all for None / all ones
    assert FocalLoss2d().device_weight("cuda:0") is None and FocalLoss2d(weight=[1, 1.0]).device_weight("cuda:0", 2) is None


@pytest.mark.parametrize("gamma", [-1, float("nan"), float("inf"), "x"])
def test_gamma_is_validated_at_construction(gamma):
    from dct_amd.loss import FocalLoss2d, get_loss_fn
    with pytest.raises(ValueError, match="FocalLoss2d: gamma"):
        FocalLoss2d(gamma=gamma)
    with pytest.raises(ValueError, match="FocalLoss2d: gamma"):
        get_loss_fn("focal", gamma=gamma)


def test_weight_length_is_checked_against_the_logits():
    from dct_amd.loss import FocalLoss2d
    with pytest.raises(ValueError, match="FocalLoss2d: 3 class weights for logits of 4 classes"):
        FocalLoss2d(weight=[1, 2, 3]).device_weight("cuda:0", 4)
    with pytest.raises(ValueError, match="class weights"):
        FocalLoss2d(weight=[1, 1, 1]).device_weight("cuda:0", 4)


@pytest.mark.parametrize("kw", [dict(), dict(gamma=0), dict(weight=[0.1, 1, 2.5, 0]), dict(reduce=False), dict(size_average=False)])
def test_cpu_tensors_are_rejected(kw):
    from dct_amd.loss import FocalLoss2d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FocalLoss2d(**kw)(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))


def test_header_and_binding_table_hold_the_five_functions():
    from dct_amd import _lib
    with open(os.path.join(ROOT, "include", "dct.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, code)
        assert decl, name
        args = [a.strip() for a in decl.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(args) == len(argtypes), (name, args)
        i = args.index("float gamma")
        assert args[i - 1].startswith("const float* weight") and argtypes[i] is _lib._f        # gamma follows weight
        assert args[-1] == "dct_stream stream"
    assert _lib.ABI_VERSION == 101


@pytest.mark.parametrize("C", [2, 3, 8])
def test_reference_at_gamma_zero_is_torch_cross_entropy(C):
    w = R.weights(C)
    _, x, t, t_ref, _, _ = R.inputs(257, C, w, True, seed=3 + C)
    r = R.Ref(x, t_ref, w, C, 0.0)
    for red in (R.MEAN, R.SUM):
        want = F.cross_entropy(x.double(), t_ref, weight=w.double(), ignore_index=R.IGN, reduction=R.RED[red])
        np.testing.assert_allclose(r.value(red)[0].item(), want.item(), rtol=1e-12)
    want = F.cross_entropy(x.double(), t_ref, weight=w.double(), ignore_index=R.IGN, reduction="none")
    # (absolute at the planted confident pixels: there torch's logsumexp(x) - x_t is the one that is off, by ~1e-16 |x|)
    np.testing.assert_allclose(r.f.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    assert torch.equal(r.m, torch.ones_like(r.m)) and torch.equal(r.k, torch.ones_like(r.k))


@pytest.mark.parametrize("C,gamma", [(2, 0.0), (3, 0.5), (4, 1.0), (8, 2.0), (3, 5.0)])
def test_reference_gradient_is_the_closed_form(C, gamma):
    """autograd through q, l and q^gamma against w k (p - y); and the pieces are what the header says they are."""
    w = R.weights(C)
    _, x, t, t_ref, _, plants = R.inputs(257, C, w, False, seed=11 + C)
    r = R.Ref(x, t_ref, w, C, gamma)
    (d,) = torch.autograd.grad(r.fmap.sum(), r.xd)
    want = r.closed_form()
    err = (d - want).abs()
    # (autograd forms d q / d x as a difference that cancels to float64 roundoff where q is 1, and multiplies it by gamma l: the
    # sentinels' l is 1e4)
    slack = 1e-14 * (r.wi * (1 + gamma * r.l))[:, None]
    assert bool((err <= 1e-11 * want.abs() + slack).all()), err.max().item()
    pt = (r.p * r.onehot).sum(1)
    np.testing.assert_allclose((r.q + pt).numpy(), 1.0, rtol=1e-14)
    if gamma > 0:
        np.testing.assert_allclose(r.m.numpy(), r.q.numpy() ** gamma, rtol=1e-12)
        np.testing.assert_allclose(r.k.numpy(), (r.m + gamma * pt * r.l * r.q ** (gamma - 1)).numpy(), rtol=1e-12)
    # l at the confident pixels keeps its relative accuracy: -log p_t = q + q^2 / 2 + ... there
    for name in ("c20", "c40", "c120"):
        i = plants[name]
        np.testing.assert_allclose(r.l[i].numpy(), (r.q[i] + r.q[i] ** 2 / 2).numpy(), rtol=1e-12)
    lo = plants["low"]
    assert bool((r.l[lo] > 149).all()) and bool((r.q[lo] > 1 - 1e-12).all())


@pytest.mark.parametrize("P,C,gamma,reduction,accumulate,stray,weighted", [c for c in R.CASES if c[0] < 1000000])
def test_float32_restatement_stays_inside_the_bounds(P, C, gamma, reduction, accumulate, stray, weighted):
    """The map, the reduced value and the gradient of a float32 evaluation on the CPU, on the GPU test's inputs, against the float64
    reference: inside the bounds the kernels are held to."""
    w = R.weights(C, alt=reduction == R.SUM) if weighted else torch.ones(C)
    _, x, t, t_ref, sen, plants = R.inputs(P, C, w, stray, seed=P + 7 * C + reduction)
    r = R.Ref(x, t_ref, w, C, gamma)
    f, total, den, d = R.restate32(x, t_ref, w, gamma)
    loss, tol = r.value(reduction)
    bad = ~((f.double() - r.f).abs() <= r.ef)
    assert not bad.any(), (int(bad.sum()), int(torch.nonzero(bad)[0]))
    assert abs(den.item() - r.D) <= R.SUM_DEPTH * R.U * r.D
    got = total.item() / den.item() if reduction == R.MEAN else total.item()
    print(f"P={P} C={C} gamma={gamma} {R.RED[reduction]}: ref {loss.item()!r} tol {tol:.3e} fp32 err {abs(got - loss.item()):.3e}; "
          f"max map err / bound {((f.double() - r.f).abs() / r.ef.clamp(min=1e-300)).max().item():.3f}")
    assert abs(got - loss.item()) <= tol
    dref, bound = r.grad(r.fmap.sum(), 1.0)
    bad = ~((d.double() - dref).abs() <= bound)
    assert not bad.any(), (int(bad.sum()), int(torch.nonzero(bad.reshape(-1))[0]))
    # the sentinels are worth more than four times the bound, and the planted pixels are what their names say
    assert (r.wi[sen] > 0).all() and r.f[sen].min().item() / (r.D if reduction == R.MEAN else 1.0) > 4 * tol
    for name, lo, hi in (("c20", 1e-10, 1e-7), ("c40", 1e-19, 1e-15)):
        if len(plants[name]):
            q = r.q[plants[name]]
            assert bool(((q > lo) & (q < hi)).all()) and bool((r.wi[plants[name]] > 0).all())
    if len(plants["c120"]):
        i = plants["c120"]
        assert bool((r.q[i] < 2.0 ** -150).all())
        if gamma > 0:
            assert torch.equal(f[i], torch.zeros(len(i))) and torch.equal(d[i], torch.zeros(len(i), C))
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(d).all())
    assert math.isfinite(got)
