"""tests/criteria_ref.py against the references the kernel tests already hold the kernels to: the restated criteria give the same
float64 values and autograd gradients as ``F.cross_entropy``, ``focal_ref.Ref``, ``DiceRef`` and ``pseudo_label_ref.rule_autograd``, on
inputs with ignored and stray targets, a class of weight 0 and an image without a counted pixel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import criteria_ref as CR
import focal_ref as FR
import pseudo_label_ref as PL
from test_dice_loss_cpu import DiceRef, _case

W = [0.1, 1.0, 2.5, 0.0]


def _grad(loss, x):
    return torch.autograd.grad(loss, x)[0]


@pytest.mark.parametrize("weight", [None, W])
def test_cross_entropy_is_torchs(weight):
    x, t = _case(3)
    x = x.reshape(-1, 4).requires_grad_(True)
    tt = torch.where((t < 0) | (t >= 4), torch.full_like(t, CR.IGN), t).reshape(-1)
    want = F.cross_entropy(x, tt, weight=None if weight is None else torch.tensor(weight, dtype=torch.float32).double(), ignore_index=CR.IGN)
    got = CR.cross_entropy(x, t.reshape(-1), weight)
    assert abs(got.item() - want.item()) <= 1e-13
    ga, gb = _grad(got, x), _grad(want, x)
    assert (ga - gb).abs().max().item() <= 1e-14
    gone = tt == CR.IGN
    assert gone.any() and (ga[gone] == 0).all()
    if weight is not None:
        assert (ga[tt == 3] == 0).all()                     # a class of weight 0: counted, no gradient


@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
def test_focal_is_focal_refs(gamma):
    x, t = _case(4)
    x32 = x.reshape(-1, 4).float()
    tt = torch.where((t < 0) | (t >= 4), torch.full_like(t, CR.IGN), t).reshape(-1)
    r = FR.Ref(x32, tt, torch.tensor(W), 4, gamma)
    want, _ = r.value(FR.MEAN)
    xd = x32.double().requires_grad_(True)
    got = CR.focal(xd, t.reshape(-1), W, gamma)
    assert abs(got.item() - want.item()) <= 1e-13 * max(1.0, abs(want.item()))
    assert (_grad(got, xd) - _grad(want, r.xd)).abs().max().item() <= 1e-13


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes,coefs", [(None, (1.0, 1.0)), ([1, 2, 3], (0.0, 1.0)), ([1, 2, 3], (0.3, 2.5))])
def test_ce_dice_is_dicerefs(per_image, classes, coefs):
    x, t = _case(11, absent=3, empty_image=1)
    r = DiceRef(x, t, W, classes, 1e-5, per_image, *coefs)
    xd = x.clone().requires_grad_(True)
    got = CR.ce_dice(xd, t, W, classes, 1e-5, per_image, *coefs)
    assert abs(got.item() - r.total.item()) <= 1e-13
    assert (_grad(got, xd) - r.autograd()).abs().max().item() <= 1e-13


@pytest.mark.parametrize("teacher,S,tau", [(PL.CROSS, 2, 0.0), (PL.CROSS, 3, 0.4), (PL.ENSEMBLE, 2, 0.0), (PL.ENSEMBLE, 3, 0.35)])
def test_pseudo_label_is_the_rule(teacher, S, tau):
    g = torch.Generator().manual_seed(7 + S)
    P, C = 301, 4
    xs32 = [torch.randn(P, C, generator=g) for _ in range(S)]
    cons = CR.Consistency("cps" if teacher == PL.CROSS else "pseudo_label", tau)
    n, kept, near = cons.decide(xs32, 1e-6)
    assert (0.0 < kept < 1.0) if tau > 0 else kept == 1.0
    xs = [x.double().requires_grad_(True) for x in xs32]
    got = cons.value(xs, n)
    k, m, _ = PL.teachers_fp32([CR.softmax32(x) for x in xs32], teacher, tau)
    ys = [x.detach().clone().requires_grad_(True) for x in xs]
    want = PL.rule_autograd([torch.softmax(y, 1) for y in ys], k, m, teacher, cons.eps).mean()
    assert abs(got.item() - want.item()) <= 1e-13
    for a, b in zip(torch.autograd.grad(got, xs), torch.autograd.grad(want, ys)):
        assert (a - b).abs().max().item() <= 1e-15
    tol, gbs = cons.bounds(xs32, n)
    assert 0 < tol < 1e-5 and all(gb.shape == (P, C) and torch.isfinite(gb).all() for gb in gbs)


def test_jsd_and_kl_are_the_oracles():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(2, 5, 5, 3, generator=g).double(), torch.randn(2, 5, 5, 3, generator=g).double()
    pa, pb = torch.softmax(a, -1).permute(0, 3, 1, 2), torch.softmax(b, -1).permute(0, 3, 1, 2)
    np.testing.assert_allclose(CR.jsd([a, b]).item(), CR.OL.jsd_2d([pa, pb]).mean().item(), rtol=1e-13)
    np.testing.assert_allclose(CR.kl(a, b).item(), CR.OL.kl_divergence_2d(pa, pb, reduce=True).item(), rtol=1e-13)
    assert CR.kl(a, a).item() == 0.0 and CR.jsd([a, a]).abs().item() <= 1e-15


def test_supervised_bounds_are_the_kernel_tests():
    """``Supervised.bounds`` hands back finite bounds of the right shape, exactly 0 on ignored pixels, for every criterion."""
    x, t = _case(9, B=2, PPI=48)
    x32, t = x.float().reshape(2, 6, 8, 4), t.reshape(2, 6, 8)
    for sup in (CR.Supervised("cross_entropy"), CR.Supervised("cross_entropy", weight=W), CR.Supervised("focal", gamma=2.0, weight=W),
                CR.Supervised("ce_dice", weight=W, classes=[1, 2, 3]), CR.Supervised("dice", classes=[1, 2, 3], per_image=True)):
        tol, gb = sup.bounds(x32, t)
        assert 0 < tol < 1e-4 and gb.shape == x32.shape and torch.isfinite(gb).all()
        gone = ~CR._counted(t, 4, CR.IGN)
        assert gone.any() and (gb[gone] == 0).all() and (gb[~gone] > 0).all()
        v = sup.value(x32.double().requires_grad_(True), t)
        assert torch.isfinite(v) and v.requires_grad
