"""The soft pseudo-label consistency criteria without a device: registry, constructor refusals, launch arguments, and the reference of
tests/soft_label_ref.py checked against itself (closed-form gradient vs autograd in float64; the two limits of the rule: T = 1 is the
pairwise cross entropy, T = 2^-10 on well-separated teachers is the hard pseudo-label)."""
import pytest
import torch

import pseudo_label_ref as PR
import soft_label_ref as R


def test_registry_names_and_types():
    from dct_amd.loss import (LOSS, PseudoLabel_2D, SoftCrossPseudoSupervision_2D, SoftEnsemblePseudoLabel_2D, SoftPseudoLabel_2D,
                              get_loss_fn)
    assert LOSS['soft_cps'] is SoftCrossPseudoSupervision_2D and LOSS['soft_pseudo_label'] is SoftEnsemblePseudoLabel_2D
    a = get_loss_fn('soft_cps', temperature=0.25, threshold=0.7)
    b = get_loss_fn('soft_pseudo_label', threshold=0.5, eps=1e-8)
    assert type(a) is SoftCrossPseudoSupervision_2D and isinstance(a, SoftPseudoLabel_2D) and a.teacher == 'cross'
    assert a.temperature == 0.25 and a.threshold == 0.7 and a.eps == 1e-10
    assert type(b) is SoftEnsemblePseudoLabel_2D and isinstance(b, SoftPseudoLabel_2D) and b.teacher == 'ensemble'
    assert b.temperature == 0.5 and b.threshold == 0.5 and b.eps == 1e-8
    assert a.last_kept is None and b.last_kept is None
    # the trainer decides by exact type: the soft criteria are no hard ones, and the hard ones are unchanged
    assert not isinstance(a, PseudoLabel_2D) and not isinstance(b, PseudoLabel_2D)
    assert not issubclass(PseudoLabel_2D, SoftPseudoLabel_2D)
    assert type(get_loss_fn('cps')).__name__ == 'CrossPseudoSupervision_2D' and type(get_loss_fn('jsd')).__name__ == 'JSD_2D'
    d = SoftPseudoLabel_2D()
    assert (d.teacher, d.temperature, d.threshold, d.eps) == ('cross', 0.5, 0.0, 1e-10)


@pytest.mark.parametrize("kw", [dict(teacher='mean'), dict(teacher=None), dict(threshold=-0.1), dict(threshold=float('nan')),
                                dict(threshold='high'), dict(eps=0.0), dict(eps=-1e-10), dict(eps=float('nan')), dict(eps=float('inf')),
                                dict(eps=1e-60), dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')),
                                dict(temperature=float('inf')), dict(temperature=1e-46), dict(temperature=1e-39),
                                dict(temperature=1e39), dict(temperature='cold'), dict(temperature=None)])
def test_constructor_refusals(kw):
    """(1e-46 is 0 in fp32; 1e-39 is a subnormal whose 1.f / T is infinite; 1e39 is infinite in fp32)"""
    from dct_amd.loss import SoftPseudoLabel_2D, get_loss_fn
    with pytest.raises(ValueError, match="dct_amd SoftPseudoLabel_2D"):
        SoftPseudoLabel_2D(**kw)
    if 'teacher' not in kw:
        with pytest.raises(ValueError):
            get_loss_fn('soft_cps', **kw)
        with pytest.raises(ValueError):
            get_loss_fn('soft_pseudo_label', **kw)


def test_launch_args():
    from dct_amd import hip_ops as K
    from dct_amd.loss import SoftCrossPseudoSupervision_2D, SoftEnsemblePseudoLabel_2D, SoftPseudoLabel_2D
    assert SoftPseudoLabel_2D().launch_args() == dict(teacher=K.PL_CROSS, tau=0.0, temperature=0.5, eps=1e-10)
    assert SoftCrossPseudoSupervision_2D(0.25, 0.6).launch_args() == dict(teacher=0, tau=0.6, temperature=0.25, eps=1e-10)
    assert SoftEnsemblePseudoLabel_2D(2.0, 0.25, 1e-6).launch_args() == dict(teacher=1, tau=0.25, temperature=2.0, eps=1e-6)
    assert SoftPseudoLabel_2D('ensemble', 1.0, float('inf')).launch_args()['tau'] == float('inf')      # nothing kept is a legal threshold
    assert SoftPseudoLabel_2D('cross').min_views() == 2 and SoftPseudoLabel_2D('ensemble').min_views() == 1
    assert SoftPseudoLabel_2D(temperature=2.0 ** -10).launch_args()['temperature'] == 2.0 ** -10        # the hard limit is a legal temperature
    for f in (K.spl_map_fwd, K.spl_map_bwd, K.spl_logits_step):
        assert callable(f)


def test_cpu_tensors_and_too_few_views_are_refused():
    from dct_amd.loss import get_loss_fn
    p = torch.full((1, 2, 2, 2), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss_fn('soft_cps')([p, p])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        get_loss_fn('soft_pseudo_label')([p])
    with pytest.raises(ValueError, match="at least 2 views"):
        get_loss_fn('soft_cps')([p])
    with pytest.raises(ValueError, match="up to 8"):
        get_loss_fn('soft_pseudo_label')([p] * 9)


def test_header_states_the_rule_beside_the_entry_points():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dct.h")).read()
    block = h[h.index("soft pseudo-label consistency"):h.index("int dct_spl_logits_step")]
    for word in ("dct_spl_map_fwd", "dct_spl_map_bwd", "DCT_PL_CROSS", "DCT_PL_ENSEMBLE", "r = 1.f / T", "first maximum", "before sharpening",
                 "exp2f(r * (log2f(q[c]) - log2f(q[k])))", "u[k] = 1 exactly", "in class order", "in ascending j", "never as a total minus",
                 "never over the kept ones", "2^-10", "exactly one-hot", "exactly 0", "DCT_ERR_BAD_ARG"):
        assert word in block, word
    assert "#define DCT_VERSION 101" in h


def _p32(P, C, S, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.softmax(torch.randn(P, C, generator=g) * 3, 1).numpy() for _ in range(S)]


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 3), ("cross", 5), ("ensemble", 1), ("ensemble", 3), ("ensemble", 8)])
@pytest.mark.parametrize("temperature", [0.25, 1.0, 2.0])
@pytest.mark.parametrize("tau", [0.0, 0.45])
def test_reference_gradient_equals_autograd(teacher, S, temperature, tau):
    """The closed form d map / d p_i[c] = -w n_ic / (p_i[c] + eps) against torch autograd through the rule written out literally (the
    sharpened target as a normalised power), both in float64 with the teachers held constant."""
    P, C, eps = 64, 4, 1e-10
    p32 = _p32(P, C, S, 7 * S + len(teacher))
    q, k, m = R.teachers(p32, teacher, tau)
    if tau:
        assert 0 < m.mean() < 1
    t, dt = R.sharpen(q, k, temperature)
    n, dn = R.terms(t, dt, m, teacher, S)
    assert (dn >= 0).all() and torch.isfinite(dn).all() and (dn <= 1e-4).all()
    torch.testing.assert_close(t.sum(-1), torch.ones(t.shape[:2], dtype=torch.float64), rtol=1e-14, atol=0)
    v, _, d, _ = R.map_and_grad(p32, n, dn, teacher, eps, fp32_sum=False)
    leaves = [torch.from_numpy(p).double().requires_grad_(True) for p in p32]
    va = R.rule_autograd(leaves, q, k, m, teacher, temperature, eps)
    torch.testing.assert_close(v, va.detach(), rtol=1e-12, atol=1e-15)
    g = torch.Generator().manual_seed(S)
    seed = torch.randn(P, generator=g, dtype=torch.float64)
    grads = torch.autograd.grad((va * seed).sum(), leaves, allow_unused=True)
    for i in range(S):
        ga = grads[i] if grads[i] is not None else torch.zeros(P, C, dtype=torch.float64)
        torch.testing.assert_close(seed[:, None] * d[i], ga, rtol=1e-12, atol=1e-300)
        assert (d[i][n[i] == 0] == 0).all()                  # no teacher term: exactly 0


@pytest.mark.parametrize("S", [2, 3, 5])
def test_reference_at_temperature_one_is_the_pairwise_cross_entropy(S):
    P, C, eps = 64, 4, 1e-10
    p32 = _p32(P, C, S, 90 + S)
    m, n, dn = R.soft_terms(p32, "cross", 0.0, 1.0)
    assert m.all()
    v, _, _, _ = R.map_and_grad(p32, n, dn, "cross", eps, fp32_sum=False)
    torch.testing.assert_close(v, R.pairwise_cross_entropy(p32, eps), rtol=1e-12, atol=0)
    # n_i is the sum of the other views' (normalised) probabilities
    ps = [torch.from_numpy(p).double() for p in p32]
    for i in range(S):
        want = sum(ps[j] / ps[j].sum(1, keepdim=True) for j in range(S) if j != i)
        torch.testing.assert_close(n[i], want, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 3), ("ensemble", 1), ("ensemble", 3)])
@pytest.mark.parametrize("tau", [0.0, 0.998])
def test_reference_at_the_hard_limit_is_the_hard_pseudo_label(teacher, S, tau):
    """T = 2^-10 (r = 1024) on teachers whose second-largest entry is at most half the largest (asserted): every u[c != k] is 2^z with
    z <= -1024 -- 0 in fp32, and at most 2^-1024 in the float64 of the reference -- so n is pseudo_label_ref.term_counts."""
    P, C = 257, 4
    g = torch.Generator().manual_seed(3 * S + len(teacher))
    xs = [torch.randn(P, C, generator=g) for _ in range(S)]
    for x in xs:
        x[torch.arange(P), torch.arange(P) % C] += 8.0
    p32 = [torch.softmax(x, 1).numpy() for x in xs]
    q, k, m = R.teachers(p32, teacher, tau)
    assert R.top_two_ratio_at_most_half(q)
    if tau:
        assert 0 < m.mean() < 1
    t, dt = R.sharpen(q, k, 2.0 ** -10)
    n, dn = R.terms(t, dt, m, teacher, S)
    counts = PR.term_counts(k, m, teacher, S, C)
    assert (n - counts).abs().max().item() <= S * C * 2.0 ** -1022
    assert ((n > 0.5) == (counts > 0.5)).all() and dn.max().item() <= S * (C + S + 2) * R.U
