"""The softmax-MSE consistency criteria without a device: registry, constructor refusals, launch arguments, and the reference of
tests/mse_consistency_ref.py checked against itself (value and closed-form gradient vs a torch float64 autograd composition with the
teachers detached; the rule's closed forms and its bound 2 / C)."""
import numpy as np
import pytest
import torch

import mse_consistency_ref as R


def test_registry_names_and_types():
    from dct_amd.loss import (LOSS, CrossMSE_2D, EnsembleMSE_2D, MSEConsistency_2D, PseudoLabel_2D, SoftPseudoLabel_2D, get_loss_fn)
    assert LOSS['cross_mse'] is CrossMSE_2D and LOSS['mean_mse'] is EnsembleMSE_2D
    a = get_loss_fn('cross_mse', threshold=0.7)
    b = get_loss_fn('mean_mse')
    assert type(a) is CrossMSE_2D and isinstance(a, MSEConsistency_2D) and a.teacher == 'cross' and a.threshold == 0.7
    assert type(b) is EnsembleMSE_2D and isinstance(b, MSEConsistency_2D) and b.teacher == 'ensemble' and b.threshold == 0.0
    assert a.last_kept is None and b.last_kept is None and not hasattr(a, 'eps')
    # the trainer decides by exact type: the MSE criteria are no pseudo-label ones, and those are unchanged
    for x in (a, b):
        assert not isinstance(x, PseudoLabel_2D) and not isinstance(x, SoftPseudoLabel_2D)
    assert not issubclass(PseudoLabel_2D, MSEConsistency_2D) and not issubclass(SoftPseudoLabel_2D, MSEConsistency_2D)
    assert type(get_loss_fn('cps')).__name__ == 'CrossPseudoSupervision_2D' and type(get_loss_fn('jsd')).__name__ == 'JSD_2D'
    d = MSEConsistency_2D()
    assert (d.teacher, d.threshold) == ('cross', 0.0)


def test_mse_2d_still_raises():
    """The reference's cold MSE_2D has another call shape: its registry name stays refused, as get_loss_fn's docstring says."""
    from dct_amd.loss import LOSS, get_loss_fn
    assert 'mse_2d' not in LOSS
    with pytest.raises(ValueError, match="name error"):
        get_loss_fn('mse_2d')
    assert "'mse_2d'" in get_loss_fn.__doc__


@pytest.mark.parametrize("kw", [dict(teacher='mean'), dict(teacher=None), dict(threshold=-0.1), dict(threshold=float('nan')),
                                dict(threshold='high'), dict(threshold=None)])
def test_constructor_refusals(kw):
    from dct_amd.loss import MSEConsistency_2D, get_loss_fn
    with pytest.raises(ValueError, match="dct_amd MSEConsistency_2D"):
        MSEConsistency_2D(**kw)
    if 'teacher' not in kw:
        with pytest.raises(ValueError):
            get_loss_fn('cross_mse', **kw)
        with pytest.raises(ValueError):
            get_loss_fn('mean_mse', **kw)
    with pytest.raises(ValueError):
        get_loss_fn('cross_mse', eps=1e-10)              # there is no eps in this rule


def test_launch_args():
    from dct_amd import hip_ops as K
    from dct_amd.loss import CrossMSE_2D, EnsembleMSE_2D, MSEConsistency_2D
    assert MSEConsistency_2D().launch_args() == dict(teacher=K.PL_CROSS, tau=0.0)
    assert CrossMSE_2D(0.6).launch_args() == dict(teacher=0, tau=0.6)
    assert EnsembleMSE_2D(0.25).launch_args() == dict(teacher=1, tau=0.25)
    assert MSEConsistency_2D('ensemble', float('inf')).launch_args()['tau'] == float('inf')      # nothing kept is a legal threshold
    assert MSEConsistency_2D('cross').min_views() == 2 and MSEConsistency_2D('ensemble').min_views() == 1
    for f in (K.mse_map_fwd, K.mse_map_bwd, K.mse_logits_step):
        assert callable(f)


def test_cpu_tensors_and_too_few_views_are_refused():
    from dct_amd.loss import get_loss_fn
    p = torch.full((1, 2, 2, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss_fn('cross_mse')([p, p])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss_fn('mean_mse')([p])
    with pytest.raises(ValueError, match="at least 2 views"):
        get_loss_fn('cross_mse')([p])
    with pytest.raises(ValueError, match="up to 8"):
        get_loss_fn('mean_mse')([p] * 9)


def test_header_states_the_rule_beside_the_entry_points():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dct.h")).read()
    block = h[h.index("softmax-MSE consistency"):h.index("int dct_mse_logits_step")]
    for word in ("dct_mse_map_fwd", "dct_mse_map_bwd", "DCT_PL_CROSS", "DCT_PL_ENSEMBLE", "first maximum", "1.f / (float)S", "in ascending j",
                 "never as a total minus", "ROUNDED product", "in class order", "never over the kept ones", "[0, 2 / C]", "exactly 2 / C",
                 "exactly 0", "S = 1", "DCT_ERR_BAD_ARG", "DCT_ERR_UNSUPPORTED", "DCT_ERR_WORKSPACE"):
        assert word in block, word
    assert "#define DCT_VERSION 101" in h


def _p32(P, C, S, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.softmax(torch.randn(P, C, generator=g) * 3, 1).numpy() for _ in range(S)]


def _torch_composition(leaves, teacher, tau):
    """The loss as a user composes it from torch ops in float64: teachers detached, the mask from the detached confidences, the mean
    squared error over the classes, the mean over teacher terms and students."""
    S = len(leaves)
    if teacher == "cross":
        tot = 0.0
        for i in range(S):
            for j in range(S):
                if j != i:
                    t = leaves[j].detach()
                    keep = (t.max(1).values >= tau).double()
                    tot = tot + keep * torch.nn.functional.mse_loss(leaves[i], t, reduction='none').mean(1)
        return tot / (S * (S - 1))
    q = (sum(leaves) / S).detach()
    keep = (q.max(1).values >= tau).double()
    return sum(keep * torch.nn.functional.mse_loss(p, q, reduction='none').mean(1) for p in leaves) / S


@pytest.mark.parametrize("teacher", ["cross", "ensemble"])
@pytest.mark.parametrize("P", [1, 17])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("tau", [0.0, 0.6])
def test_reference_equals_a_torch_autograd_composition(teacher, P, S, C, tau):
    p32 = _p32(P, C, S, 100 * P + 10 * S + C)
    t, m = R.teachers(p32, teacher, tau)
    if tau and P > 1:
        assert 0 < m.mean() < 1
    v, vb, d, db = R.map_and_grad(p32, t, m, teacher)
    assert (vb >= 0).all() and (db >= 0).all() and (vb <= 1e-5).all() and (db <= 1e-5).all()
    leaves = [torch.from_numpy(p).double().requires_grad_(True) for p in p32]
    # the rule written out literally on the reference's own fp32 teacher vectors: 1e-12
    va = R.rule_autograd(leaves, t, m, teacher)
    torch.testing.assert_close(v, va.detach(), rtol=1e-12, atol=1e-300)
    g = torch.Generator().manual_seed(S)
    seed = torch.randn(P, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad((va * seed).sum(), leaves)
    for i in range(S):
        torch.testing.assert_close(seed[:, None] * d[i], grads[i], rtol=1e-12, atol=1e-300)
    # the composition a user writes, whose ensemble mean is float64 where the rule's q is fp32: 2 U relative to the probabilities
    vc = _torch_composition(leaves, teacher, tau)
    torch.testing.assert_close(v, vc.detach(), rtol=0, atol=8 * R.U)
    gc = torch.autograd.grad((vc * seed).sum(), leaves)
    for i in range(S):
        torch.testing.assert_close(seed[:, None] * d[i], gc[i], rtol=0, atol=8 * R.U * float(seed.abs().max()))


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 5), ("cross", 8), ("ensemble", 1), ("ensemble", 2)])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_identical_views_give_zero(teacher, S, C):
    """Views that agree bit for bit: exactly 0 under the cross teacher at any S, under the ensemble teacher at S = 1 and 2, where the
    sum and its scaling are exact (p + p = 2 p, 2 p * 0.5f = p); from three views on the fp32 mean of equal numbers may differ from them in
    the last bit, as the header says."""
    p = _p32(33, C, 1, 5 + C)[0]
    m, v, vb, d, db = R.rule([p.copy() for _ in range(S)], teacher, 0.0)
    assert m.all() and (v == 0).all() and (d == 0).all() and (vb <= S * S * C * R.TINY).all() and (db == 0).all()


@pytest.mark.parametrize("C", [2, 3, 4, 5, 8])
def test_opposite_one_hots_give_two_over_c(C):
    a, b = np.zeros((C, C), np.float32), np.zeros((C, C), np.float32)
    for r in range(C):
        a[r, r], b[r, (r + 1) % C] = 1.0, 1.0
    m, v, vb, d, db = R.rule([a, b], "cross", 0.0)
    assert m.all()
    np.testing.assert_allclose(v.numpy(), 2.0 / C, rtol=1e-15)
    # and in fp32, as the kernel forms it: 4 w with w = 1.f / (float)(2 C) is 2.f / C bit for bit (a power of two times w)
    assert np.float32(4.0) * (np.float32(1.0) / np.float32(2 * C)) == np.float32(2.0) / np.float32(C)
    # every student is pushed away from the other's class and towards its own by 2 w
    np.testing.assert_allclose(d[0].numpy(), 2.0 / (2 * C) * (a.astype(np.float64) - b), rtol=1e-15)


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 3), ("ensemble", 1), ("ensemble", 3)])
def test_everything_masked_gives_zero(teacher, S):
    p32 = _p32(17, 4, S, 9)
    m, v, vb, d, db = R.rule(p32, teacher, 2.0)
    assert not m.any() and (v == 0).all() and (d == 0).all() and (db == 0).all()


def test_single_view_ensemble_is_zero():
    p32 = _p32(65, 4, 1, 3)
    t, m = R.teachers(p32, "ensemble", 0.0)
    assert np.array_equal(t[0], p32[0])                  # q = p * 1.f
    v, vb, d, db = R.map_and_grad(p32, t, m, "ensemble")
    assert m.all() and (v == 0).all() and (d == 0).all()


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 3), ("cross", 8), ("ensemble", 2), ("ensemble", 5)])
@pytest.mark.parametrize("C", [2, 4, 8])
def test_map_is_bounded_by_two_over_c(teacher, S, C):
    """Random softmax outputs of logits x 3 and x 30 (nearly one-hot): 0 <= map <= 2 / C, with the rounding of the fp32 probabilities'
    sums (each within C U of 1) allowed for."""
    for scale, seed in ((3, 1), (30, 2)):
        g = torch.Generator().manual_seed(seed + S + C)
        p32 = [torch.softmax(torch.randn(257, C, generator=g) * scale, 1).numpy() for _ in range(S)]
        m, v, vb, d, db = R.rule(p32, teacher, 0.0)
        assert (v >= 0).all() and (v <= 2.0 / C * (1 + 4 * C * R.U)).all()
        if scale == 30 and teacher == "cross" and S == 2:
            assert v.max() > 1.5 / C                      # the bound is approached, not vacuous
