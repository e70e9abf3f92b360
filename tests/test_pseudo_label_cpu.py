"""The pseudo-label consistency criteria without a device: registry, constructor refusals, launch arguments, and the reference of
tests/pseudo_label_ref.py checked against itself (closed-form gradient vs autograd in float64; the fp32 teacher derivation on
hand-built pixels with exact ties)."""
import numpy as np
import pytest
import torch

import pseudo_label_ref as R


def test_registry_names_and_types():
    from dct_amd.loss import LOSS, CrossPseudoSupervision_2D, EnsemblePseudoLabel_2D, PseudoLabel_2D, get_loss_fn
    assert LOSS['cps'] is CrossPseudoSupervision_2D and LOSS['pseudo_label'] is EnsemblePseudoLabel_2D
    a, b = get_loss_fn('cps', threshold=0.7), get_loss_fn('pseudo_label', threshold=0.5, eps=1e-8)
    assert type(a) is CrossPseudoSupervision_2D and isinstance(a, PseudoLabel_2D) and a.teacher == 'cross' and a.threshold == 0.7
    assert type(b) is EnsemblePseudoLabel_2D and isinstance(b, PseudoLabel_2D) and b.teacher == 'ensemble' and b.eps == 1e-8
    assert a.last_kept is None and b.last_kept is None
    d = get_loss_fn('cps')
    assert d.threshold == 0.0 and d.eps == 1e-10
    assert type(get_loss_fn('jsd')).__name__ == 'JSD_2D'


@pytest.mark.parametrize("kw", [dict(teacher='mean'), dict(teacher=None), dict(threshold=-0.1), dict(threshold=float('nan')),
                                dict(threshold='high'), dict(eps=0.0), dict(eps=-1e-10), dict(eps=float('nan')), dict(eps=float('inf')),
                                dict(eps=1e-60)])
def test_constructor_refusals(kw):
    from dct_amd.loss import PseudoLabel_2D, get_loss_fn
    with pytest.raises(ValueError, match="dct_amd PseudoLabel_2D"):
        PseudoLabel_2D(**kw)
    if 'teacher' not in kw:
        with pytest.raises(ValueError):
            get_loss_fn('cps', **kw)
        with pytest.raises(ValueError):
            get_loss_fn('pseudo_label', **kw)


def test_launch_args():
    from dct_amd import hip_ops as K
    from dct_amd.loss import CrossPseudoSupervision_2D, EnsemblePseudoLabel_2D, PseudoLabel_2D
    assert (K.PL_CROSS, K.PL_ENSEMBLE) == (0, 1)
    assert PseudoLabel_2D().launch_args() == dict(teacher=0, tau=0.0, eps=1e-10)
    assert CrossPseudoSupervision_2D(0.6).launch_args() == dict(teacher=0, tau=0.6, eps=1e-10)
    assert EnsemblePseudoLabel_2D(0.25, 1e-6).launch_args() == dict(teacher=1, tau=0.25, eps=1e-6)
    assert PseudoLabel_2D('ensemble', float('inf')).launch_args()['tau'] == float('inf')      # nothing kept is a legal threshold
    assert PseudoLabel_2D('cross').min_views() == 2 and PseudoLabel_2D('ensemble').min_views() == 1


def test_cpu_tensors_and_too_few_views_are_refused():
    from dct_amd.loss import get_loss_fn
    p = torch.full((1, 2, 2, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss_fn('cps')([p, p])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss_fn('pseudo_label')([p])
    with pytest.raises(ValueError, match="at least 2 views"):
        get_loss_fn('cps')([p])
    with pytest.raises(ValueError, match="up to 8"):
        get_loss_fn('pseudo_label')([p] * 9)


def test_header_states_the_rule_beside_the_entry_points():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dct.h")).read()
    for word in ("DCT_PL_CROSS 0", "DCT_PL_ENSEMBLE 1", "dct_pl_map_fwd", "dct_pl_map_bwd", "dct_pl_logits_step", "first maximum",
                 "never over the kept ones"):
        assert word in h, word


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 3), ("cross", 5), ("ensemble", 1), ("ensemble", 3), ("ensemble", 8)])
@pytest.mark.parametrize("tau", [0.0, 0.45])
def test_reference_gradient_equals_autograd(teacher, S, tau):
    """The closed form d map / d p_i[c] = -w n_ic / (p_i[c] + eps) against torch autograd through the rule written out literally, both
    in float64 with the teachers held constant."""
    P, C, eps = 64, 4, 1e-10
    g = torch.Generator().manual_seed(7 * S + len(teacher))
    p32 = [torch.softmax(torch.randn(P, C, generator=g) * 3, 1).numpy() for _ in range(S)]
    k, m, _ = R.teachers_fp32(p32, teacher, tau)
    if tau:
        assert 0 < m.mean() < 1
    n = R.term_counts(k, m, teacher, S, C)
    v, _, d, _ = R.map_and_grad(p32, n, teacher, eps, fp32_sum=False)
    leaves = [torch.from_numpy(p).double().requires_grad_(True) for p in p32]
    va = R.rule_autograd(leaves, k, m, teacher, eps)
    torch.testing.assert_close(v, va.detach(), rtol=1e-13, atol=1e-15)
    seed = torch.randn(P, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad((va * seed).sum(), leaves, allow_unused=True)
    for i in range(S):
        ga = grads[i] if grads[i] is not None else torch.zeros(P, C, dtype=torch.float64)
        torch.testing.assert_close(seed[:, None] * d[i], ga, rtol=1e-13, atol=1e-300)
        assert (d[i][n[i] == 0] == 0).all()                  # no teacher term: exactly 0


def _collapsing_pair(S):
    """Two adjacent fp32 values a < b in [1, 2) whose products with fl(1 / S) round to the same fp32: a tie that only scaling creates."""
    inv = np.float32(1.0) / np.float32(S)
    a = np.float32(1.75)     # (for S = 3, 5, 7 the products here are spaced more narrowly than the fp32 grid they round to)
    for _ in range(64):
        b = np.nextafter(a, np.float32(2.0))
        if np.float32(a * inv) == np.float32(b * inv):
            return a, b
        a = b
    raise AssertionError("no collapsing pair found")


def test_reference_teachers_on_exact_ties():
    f = np.float32
    # cross: the first maximum wins; a later strictly larger value takes over; the confidence is compared with >=
    p0 = np.array([[0.25, 0.25, 0.25, 0.25], [0.1, 0.4, 0.4, 0.1], [0.2, 0.3, 0.1, 0.4], [0.5, 0.5, 0.0, 0.0]], dtype=f)
    p1 = np.array([[0.0, 0.5, 0.5, 0.0], [0.7, 0.1, 0.1, 0.1], [0.4, 0.4, 0.1, 0.1], [0.0, 0.0, 0.5, 0.5]], dtype=f)
    k, m, q = R.teachers_fp32([p0, p1], "cross", 0.4)
    assert k.tolist() == [[0, 1, 3, 0], [1, 0, 0, 2]]
    assert q.dtype == np.float32 and q.tolist() == [[f(0.25), f(0.4), f(0.4), f(0.5)], [f(0.5), f(0.7), f(0.4), f(0.5)]]
    assert m.tolist() == [[False, True, True, True], [True, True, True, True]]        # q == tau is kept
    assert R.kept_map(m, "cross", 2).tolist() == [0.5, 1.0, 1.0, 1.0]
    n = R.term_counts(k, m, "cross", 2, 4)
    assert n[0, 0].tolist() == [0, 1, 0, 0] and n[1, 0].tolist() == [0, 0, 0, 0]      # view 0 is masked as a teacher, still a student
    assert n[0, 2].tolist() == [1, 0, 0, 0] and n[1, 2].tolist() == [0, 0, 0, 1]

    # ensemble: sums that tie exactly -> the first class; the sums are added in view order, one rounding per add
    e0 = np.array([[0.5, 0.25, 0.25], [f(0.1), f(0.2), f(0.7)]], dtype=f)
    e1 = np.array([[0.25, 0.5, 0.25], [f(0.2), f(0.1), f(0.7)]], dtype=f)
    e2 = np.array([[0.25, 0.25, 0.5], [f(0.7), f(0.7), f(0.1)]], dtype=f)
    k, m, q = R.teachers_fp32([e0, e1, e2], "ensemble", 0.0)
    assert k.shape == (1, 2) and k[0, 0] == 0 and q[0, 0] == f(1.0) * (f(1.0) / f(3.0))
    s01 = (e0[1] + e1[1]).astype(f)
    s = (s01 + e2[1]).astype(f)
    assert q[0, 1] == f(s.max() * (f(1.0) / f(3.0))) and k[0, 1] == int(np.argmax(s))

    # a tie that only scaling creates: the argmax is taken on the unscaled sums, so the larger sum (class 1) wins
    for S in (3, 5, 7):
        a, b = _collapsing_pair(S)
        views = [np.array([[0.5, 0.5]], dtype=f), np.array([[0.5, 0.5]], dtype=f), np.array([[a - f(1.0), b - f(1.0)]], dtype=f)]
        views += [np.zeros((1, 2), dtype=f)] * (S - 3)
        assert f(f(1.0) + views[2][0, 0]) == a and f(f(1.0) + views[2][0, 1]) == b          # the sums are exactly a and b
        k, m, q = R.teachers_fp32(views, "ensemble", 0.0)
        inv = f(1.0) / f(S)
        assert f(a * inv) == f(b * inv) and k[0, 0] == 1 and q[0, 0] == f(b * inv)
        # the threshold is compared with the scaled sum
        assert R.teachers_fp32(views, "ensemble", float(q[0, 0]))[1][0, 0]
        assert not R.teachers_fp32(views, "ensemble", float(np.nextafter(q[0, 0], f(2.0))))[1][0, 0]
    assert R.kept_map(np.array([[True, False]]), "ensemble", 4).tolist() == [1.0, 0.0]
