"""Tversky and focal Tversky (``dct_ce_tversky_*``, include/dct.h; ``TverskyLoss`` / ``FocalTverskyLoss`` / ``CrossEntropyTverskyLoss2d``)
without a device: the header's closed-form gradient against ``torch.autograd.grad`` of the float64 reference (tests/tversky_ref.py), the
reference against Dice and Jaccard, the exact zeros of an empty denominator and of u == 0, the registry names and the constructors'
validation.  Header, exports and binding table of the four symbols are covered by tests/test_abi_cpu.py."""
import pytest
import torch

from test_dice_loss_cpu import DiceRef, _case
from tversky_ref import IGN, TverskyRef

PARAMS = [(0.3, 0.7, 1.0), (0.3, 0.7, 4.0 / 3.0), (1.0, 1.0, 2.0), (0.7, 0.3, 0.75), (0.5, 0.5, 1.0), (0.0, 1.0, 3.0)]
W = [0.1, 1.0, 0.0, 2.5]


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("abg", PARAMS)
@pytest.mark.parametrize("classes,smooth,coefs", [(None, 1e-5, (1.0, 1.0)), ([1, 2, 3], 0.0, (0.0, 1.0)), ([2], 1.0, (0.3, 2.5)),
                                                  (None, 0.0, (0.7, 0.0))])
def test_closed_form_gradient_is_autograds(per_image, abg, classes, smooth, coefs):
    """Six parameter sets, G = 1 and G = B, over inputs with stray targets, a class absent from gt (class 3) and an image with no counted
    pixel (image 1): under smooth = 0 that image's denominator is 0 when G = B (T = 1, no gradient)."""
    x, t = _case(11, absent=3, empty_image=1)
    r = TverskyRef(x, t, W, classes, smooth, *abg, per_image, *coefs)
    assert not r.keep[1].any() and not (t == 3).any()
    if per_image and smooth == 0.0:
        assert r.empty[1].all() and (r.T[1] == 1).all() and (r.term[1] == 0).all()
    got, want = r.closed_form(0.61), r.autograd(0.61)
    assert torch.isfinite(want).all()
    assert (got - want).abs().max().item() <= 1e-12, (got - want).abs().max().item()
    assert (got[~r.keep] == 0).all() and (want[~r.keep] == 0).all()
    assert got.abs().max().item() > 1e-4                                    # (the comparison is of something)


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", [None, [1, 2]])
@pytest.mark.parametrize("s", [0.0, 1e-5, 1.0])
def test_half_half_is_dice_with_twice_the_smooth(per_image, classes, s):
    x, t = _case(7, absent=3)
    r = TverskyRef(x, t, W, classes, s, 0.5, 0.5, 1.0, per_image, 0.5, 2.0)
    d = DiceRef(x, t, W, classes, 2 * s, per_image, 0.5, 2.0)
    assert r.c0 == 0.0 and not r.focal
    assert abs(r.tversky.item() - d.dice.item()) <= 1e-12 and abs(r.total.item() - d.total.item()) <= 1e-12
    assert (r.T - d.D).abs().max().item() <= 1e-12
    assert (r.closed_form(0.61) - d.closed_form(0.61)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("per_image", [False, True])
def test_one_one_is_jaccard(per_image):
    x, t = _case(9)
    r = TverskyRef(x, t, None, [1, 2, 3], 0.0, 1.0, 1.0, 1.0, per_image, 0.0, 1.0)
    k = r.keep[..., None].double()
    p, y = r.p.detach() * k, r.y
    dims = (1,) if per_image else (0, 1)
    inter, union = (p * y).sum(dims), (p + y - p * y).sum(dims)
    iou = (inter / union).reshape(r.G, 4)
    assert r.c0 == -1.0
    assert (r.T.detach() - iou).abs().max().item() <= 1e-12
    assert abs(r.tversky.item() - (1 - iou[:, 1:].mean().item())) <= 1e-12


@pytest.mark.parametrize("gamma", [1.0, 4.0 / 3.0, 0.75])
def test_empty_denominator_and_zero_u_are_exact_zeros(gamma):
    """(a) smooth = 0 under per_image with one image fully ignored: that image's Den is 0.  (b) alpha = 0, beta = 1, smooth = 0 and a class of
    the mask absent from the targets: its Den = beta Y = 0 although S > 0.  (c) alpha = 0, beta = 1 and a class whose target pixels are
    all predicted with probability exactly 1: Den = Y + smooth = N, so T = 1 and u = 0 with a non-zero denominator.  Each gives exactly 0
    to the value and exactly 0 gradient through that (g, c), by the closed form and by autograd."""
    # (a)
    x, t = _case(3, empty_image=1)
    r = TverskyRef(x, t, None, None, 0.0, 0.3, 0.7, gamma, True, 0.0, 1.0)
    assert r.empty[1].all() and not r.empty[0].any() and not r.empty[2].any()
    assert (r.T[1] == 1).all() and (r.term[1] == 0).all() and (r.u[1] == 0).all()
    f, qa, qb = r.coeffs()
    assert (f[1] == 0).all() and (qa[1] == 0).all() and (qb[1] == 0).all()
    for d in (r.closed_form(), r.autograd()):
        assert (d[1] == 0).all() and d[0].abs().max().item() > 1e-6
    assert abs(r.tversky.item() - (r.term[0].sum().item() + r.term[2].sum().item()) / 12) <= 1e-15        # (image 1 adds exactly 0)
    # (b)
    x, t = _case(4, absent=2)
    r = TverskyRef(x, t, None, [1, 2], 0.0, 0.0, 1.0, gamma, False, 0.0, 1.0)
    assert r.c0 == 0.0 and r.Y[0, 2].item() == 0 and r.S[0, 2].item() > 0 and r.empty[0, 2] and not r.empty[0, 1]
    assert r.T[0, 2].item() == 1.0 and r.term[0, 2].item() == 0.0
    f, qa, qb = r.coeffs()
    assert f[0, 2] == 0 and qa[0, 2] == 0 and qb[0, 2] == 0 and qa[0, 1] > 0
    assert r.tversky.item() == r.term[0, 1].item() / 2
    only1 = TverskyRef(x, t, None, [1], 0.0, 0.0, 1.0, gamma, False, 0.0, 1.0)
    for d, d1 in ((r.closed_form(), only1.closed_form()), (r.autograd(), only1.autograd())):
        assert torch.equal(d, d1 / 2) and d.abs().max().item() > 1e-6       # (class 2 adds nothing; K = 2 against K = 1)
    # (c)
    x, t = _case(5)
    x[t == 2] = torch.tensor([0.0, 0.0, 200.0, 0.0], dtype=x.dtype)
    r = TverskyRef(x, t, None, [1, 2], 1e-5, 0.0, 1.0, gamma, False, 0.0, 1.0)
    assert r.I[0, 2].item() == r.Y[0, 2].item() > 0 and not r.empty.any()
    assert r.T[0, 2].item() == 1.0 and r.u[0, 2].item() == 0.0 and r.term[0, 2].item() == 0.0 and not r.some[0, 2]
    f, qa, qb = r.coeffs()
    assert f[0, 2] == 0 and qa[0, 2] == 0 and qb[0, 2] == 0
    only1 = TverskyRef(x, t, None, [1], 1e-5, 0.0, 1.0, gamma, False, 0.0, 1.0)
    assert r.tversky.item() == only1.tversky.item() / 2
    for d, d1 in ((r.closed_form(), only1.closed_form()), (r.autograd(), only1.autograd())):
        assert torch.equal(d, d1 / 2) and d.abs().max().item() > 1e-6


# ------------------------------------------------------------------------------------------------------- registry and constructors
def test_registry_names():
    from dct_amd.loss import CrossEntropyTverskyLoss2d, FocalTverskyLoss, TverskyLoss, get_loss_fn
    a = get_loss_fn("tversky", classes=range(1, 4), per_image=True)
    assert type(a) is TverskyLoss and a.classes == [1, 2, 3] and a.per_image and a.ce_coef == 0.0 and a.tversky_coef == 1.0
    assert (a.alpha, a.beta, a.gamma, a.smooth, a.ignore_index) == (0.3, 0.7, 1.0, 1e-5, 255)
    b = get_loss_fn("focal_tversky", alpha=0.4, beta=0.6)
    assert type(b) is FocalTverskyLoss and (b.alpha, b.beta, b.gamma) == (0.4, 0.6, 4.0 / 3.0) and b.ce_coef == 0.0 and b.classes is None
    c = get_loss_fn("ce_tversky", weight=[0.1, 1, 2.5, 0], tversky_coef=0.5, gamma=2)
    assert type(c) is CrossEntropyTverskyLoss2d and c.ce_coef == 1.0 and c.tversky_coef == 0.5 and c.gamma == 2.0
    assert c.last_tversky is None and not c.per_image
    with pytest.raises(ValueError):
        get_loss_fn("no_such_loss")


def test_launch_arguments():
    from dct_amd.loss import CrossEntropyTverskyLoss2d, FocalTverskyLoss, TverskyLoss
    assert TverskyLoss(classes=range(1, 4)).launch_args(4) == dict(
        class_mask=0b1110, smooth=1e-5, alpha=0.3, beta=0.7, gamma=1.0, per_image=False, ce_coef=0.0, tversky_coef=1.0)
    assert FocalTverskyLoss(0.7, 0.3, 0.75, per_image=True).launch_args(2) == dict(
        class_mask=0b11, smooth=1e-5, alpha=0.7, beta=0.3, gamma=0.75, per_image=True, ce_coef=0.0, tversky_coef=1.0)
    assert CrossEntropyTverskyLoss2d(classes=[1, 1, 0], smooth=1, ce_coef=2).launch_args(2)["class_mask"] == 0b11
    assert CrossEntropyTverskyLoss2d().launch_args(8)["class_mask"] == 255


def test_constructor_validation():
    from dct_amd.loss import CrossEntropyTverskyLoss2d, FocalTverskyLoss, TverskyLoss
    nan, inf = float("nan"), float("inf")
    for cls in (TverskyLoss, FocalTverskyLoss, CrossEntropyTverskyLoss2d):
        who = f"dct_amd {cls.__name__}: "
        with pytest.raises(ValueError, match=who + "classes is empty"):
            cls(classes=[])
        with pytest.raises(ValueError, match=who + "class -1 is negative"):
            cls(classes=[-1, 2])
        for bad in (-1e-5, inf, nan):
            with pytest.raises(ValueError, match=who + "smooth"):
                cls(smooth=bad)
        with pytest.raises(ValueError, match=who + "smooth must be a number"):
            cls(smooth="x")
        with pytest.raises(ValueError, match=who + r"class 4 outside \[0, 4\)"):
            cls(classes=[1, 4]).launch_args(4)
        for name in ("alpha", "beta"):
            for bad in (-0.1, inf, nan, 1e39):
                with pytest.raises(ValueError, match=who + name if bad != 1e39 else who + "alpha \\+ beta"):
                    cls(**{name: bad})
            with pytest.raises(ValueError, match=who + name + " must be a number"):
                cls(**{name: None})
        with pytest.raises(ValueError, match=who + r"alpha \+ beta"):
            cls(alpha=0, beta=0.0)
        with pytest.raises(ValueError, match=who + r"alpha \+ beta"):
            cls(alpha=1e-60, beta=0.0)                                      # (0 as the kernels take it)
        cls(alpha=0, beta=1)
        cls(alpha=1, beta=0)
    for cls in (FocalTverskyLoss, CrossEntropyTverskyLoss2d):
        who = f"dct_amd {cls.__name__}: "
        for bad in (0, -1.0, inf, nan, 1e-60, 1e39):
            with pytest.raises(ValueError, match=who + "gamma must be finite and > 0"):
                cls(gamma=bad)
        with pytest.raises(ValueError, match=who + "gamma must be a number"):
            cls(gamma="two")
    with pytest.raises(TypeError):
        TverskyLoss(gamma=2.0)                                              # (gamma is fixed at 1 there)
    for name in ("ce_coef", "tversky_coef"):
        with pytest.raises(ValueError, match="dct_amd CrossEntropyTverskyLoss2d: " + name + " must be a number"):
            CrossEntropyTverskyLoss2d(**{name: "a"})
    with pytest.raises(ValueError, match="3 class weights for logits of 4 classes"):
        CrossEntropyTverskyLoss2d(weight=[1, 2, 3]).device_weight("cuda:0", 4)
    assert CrossEntropyTverskyLoss2d().device_weight("cuda:0") is None and TverskyLoss().device_weight("cuda:0", 4) is None


def test_the_cpu_is_refused():
    from dct_amd.loss import CrossEntropyTverskyLoss2d, FocalTverskyLoss, TverskyLoss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CrossEntropyTverskyLoss2d(weight=[0.1, 1, 2.5, 0]).device_weight("cpu")
    for crit in (TverskyLoss(), FocalTverskyLoss(), CrossEntropyTverskyLoss2d(weight=[0.1, 1, 2.5, 0]), CrossEntropyTverskyLoss2d(classes=[1])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crit(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))


def test_trainer_counts_the_family_as_fused_criteria():
    """The three classes are in the trainer's ``fused_sup`` set and ``_StepContext`` carries their launch arguments in a trailing keyword."""
    import inspect
    from dct_amd.trainer import cotraining_totalloss as ct
    params = list(inspect.signature(ct._StepContext.__init__).parameters)
    assert params[-1] == "overlap" and "overlap" in ct._StepContext.__slots__
    src = inspect.getsource(ct.CoTrainer._step_facts)
    for name in ("CrossEntropyTverskyLoss2d", "TverskyLoss", "FocalTverskyLoss"):
        assert name in src
