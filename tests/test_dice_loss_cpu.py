"""Soft Dice and CE + Dice (``dct_ce_dice_*``, include/dct.h; ``DiceLoss`` / ``CrossEntropyDiceLoss2d``) without a device: the float64
torch reference of the rule (``DiceRef``; tests/test_dice_loss_gpu.py holds the kernels to it), the header's closed-form gradient against
``torch.autograd.grad`` of that reference, the registry names and the constructors' validation.  Header, exports and binding table of the
four symbols are covered by tests/test_abi_cpu.py."""
import pytest
import torch
import torch.nn.functional as F

IGN = 255


class DiceRef:
    """The rule of include/dct.h in float64.  ``x``: logits [B, PPI, C] (any float dtype; taken to float64), ``t``: int64 [B, PPI],
    ``weight``: C values or None, ``classes``: the class indices of the Dice mean or None (all).  Fields: ``total``, ``ce``, ``sumw``,
    ``dice`` (0-d tensors; ``total`` carries the graph to ``xd``), ``D``, ``I``, ``S``, ``Y`` ([G, C]), ``keep`` [B, PPI], ``p``, ``y``."""

    def __init__(self, x, t, weight=None, classes=None, smooth=1e-5, per_image=False, ce_coef=1.0, dice_coef=1.0, ignore_index=IGN):
        B, PPI, C = x.shape
        self.B, self.PPI, self.C = B, PPI, C
        self.G = B if per_image else 1
        self.mask = torch.zeros(C, dtype=torch.bool)
        self.mask[list(range(C)) if classes is None else sorted(set(classes))] = True
        self.K = int(self.mask.sum())
        self.smooth, self.per_image, self.ce_coef, self.dice_coef = float(smooth), bool(per_image), float(ce_coef), float(dice_coef)
        self.xd = x.detach().double().requires_grad_(True)
        self.keep = (t != ignore_index) & (t >= 0) & (t < C)
        self.tc = torch.where(self.keep, t, torch.zeros_like(t))
        k = self.keep[..., None].double()
        self.wd = torch.ones(C, dtype=torch.float64) if weight is None else torch.as_tensor(weight).double()
        self.wi = self.wd[self.tc] * self.keep
        self.p = torch.softmax(self.xd, -1)
        self.y = F.one_hot(self.tc, C).double() * k
        dims = (1,) if per_image else (0, 1)
        shape = (self.G, C)
        self.I = (self.p * self.y).sum(dims).reshape(shape)
        self.S = (self.p * k).sum(dims).reshape(shape)
        self.Y = self.y.sum(dims).reshape(shape)
        self.num, self.den = 2 * self.I + self.smooth, self.S + self.Y + self.smooth
        self.empty = self.den == 0
        self.D = torch.where(self.empty, torch.ones_like(self.den), self.num / torch.where(self.empty, torch.ones_like(self.den), self.den))
        self.dice = 1 - self.D[:, self.mask].sum() / (self.G * self.K)
        self.l = (torch.logsumexp(self.xd, -1) - self.xd.gather(-1, self.tc[..., None])[..., 0]) * self.keep
        self.sumw = self.wi.sum()
        self.ce = (self.wi * self.l).sum() / self.sumw
        self.total = torch.zeros((), dtype=torch.float64)
        if self.ce_coef != 0:
            self.total = self.total + self.ce_coef * self.ce
        if self.dice_coef != 0:
            self.total = self.total + self.dice_coef * self.dice

    def autograd(self, g=1.0):
        """g * dtotal/dx by torch.autograd [B, PPI, C] (zeros when neither term depends on x)."""
        if not self.total.requires_grad:
            return torch.zeros_like(self.xd)
        return g * torch.autograd.grad(self.total, self.xd, retain_graph=True)[0]

    def q(self):
        """q_c per pixel [B, PPI, C] = -(m_c / (G K)) (alpha_gc y_c - beta_gc), and the per-group alpha, beta [G, C]."""
        with torch.no_grad():
            one = torch.ones_like(self.den)
            den = torch.where(self.empty, one, self.den)
            alpha = torch.where(self.empty, 0 * one, 2 / den)
            beta = torch.where(self.empty, 0 * one, self.num / den ** 2)
            m = self.mask.double() / (self.G * self.K)
            a, b = (alpha * m), (beta * m)                                  # [G, C]
            if not self.per_image:
                a, b = a.expand(self.B, self.C), b.expand(self.B, self.C)
            return -(a[:, None, :] * self.y - b[:, None, :]), alpha, beta

    def closed_form(self, g=1.0):
        """The header's gradient: g (ce_coef (w_i / sum w)(p - y) + dice_coef p (q - sum_k p_k q_k)); exactly 0 off the counted pixels."""
        with torch.no_grad():
            k = self.keep[..., None].double()
            d = torch.zeros_like(self.xd)
            if self.ce_coef != 0:
                d = d + self.ce_coef * (self.wi / self.sumw)[..., None] * (self.p - self.y)
            if self.dice_coef != 0:
                q, _, _ = self.q()
                d = d + self.dice_coef * self.p * (q - (self.p * q).sum(-1, keepdim=True))
            return g * d * k


def _case(seed, B=3, PPI=37, C=4, absent=None, empty_image=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, PPI, C, generator=g, dtype=torch.float64) * 2
    t = torch.randint(0, C, (B, PPI), generator=g)
    t[torch.rand(B, PPI, generator=g) < 0.25] = IGN
    t[0, 1], t[0, 2] = C, -1                                               # stray targets: uncounted like ignore_index
    if absent is not None:
        t[t == absent] = (absent + 1) % C
    if empty_image is not None:
        t[empty_image] = IGN
    return x, t


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", [None, [1, 2, 3], [2]])
@pytest.mark.parametrize("smooth", [0.0, 1e-5, 1.0])
@pytest.mark.parametrize("coefs", [(1.0, 1.0), (0.0, 1.0), (0.7, 0.0), (0.3, 2.5)])
def test_closed_form_gradient_is_autograds(per_image, classes, smooth, coefs):
    """G = 1 and G = B, masks with and without background (and K = 1), the three smooth values, each coefficient 0, over inputs with
    stray targets, a class absent from gt (class 3) and an image with no counted pixel (image 1): under smooth = 0 that image's
    denominator is 0 when G = B (D = 1, no gradient); under smooth > 0 it is smooth alone."""
    x, t = _case(11, absent=3, empty_image=1)
    w = [0.1, 1.0, 0.0, 2.5]
    r = DiceRef(x, t, w, classes, smooth, per_image, *coefs)
    assert not r.keep[1].any() and not (t == 3).any()
    if per_image and smooth == 0.0:
        assert r.empty[1].all() and (r.D[1] == 1).all()
    assert bool(r.empty.any()) == (per_image and smooth == 0.0)
    got, want = r.closed_form(0.61), r.autograd(0.61)
    assert torch.isfinite(want).all()
    assert (got - want).abs().max().item() <= 1e-12, (got - want).abs().max().item()
    assert (got[~r.keep] == 0).all() and (want[~r.keep] == 0).all()
    if coefs[0] != 0 or coefs[1] != 0:
        assert got.abs().max().item() > 1e-4                                # (the comparison is of something)


def test_reference_values():
    """The pieces of the reference against their definitions: ce is F.cross_entropy's weighted mean, D of a class absent from gt under
    smooth = 0 is 0, a zero coefficient removes its term (the NaN ce of all-zero weights with it), K counts the mask."""
    x, t = _case(5, absent=3)
    w = torch.tensor([0.1, 1.0, 0.0, 2.5], dtype=torch.float64)
    r = DiceRef(x, t, w, [1, 2, 3], 0.0, False, 0.5, 2.0)
    tt = torch.where((t < 0) | (t >= 4), torch.full_like(t, IGN), t)
    ce = F.cross_entropy(x.reshape(-1, 4), tt.reshape(-1), weight=w, ignore_index=IGN)
    assert abs(r.ce.item() - ce.item()) <= 1e-12 and r.K == 3 and r.G == 1
    assert r.D[0, 3].item() == 0.0 and r.Y[0, 3].item() == 0.0
    assert abs(r.total.item() - (0.5 * r.ce.item() + 2.0 * r.dice.item())) <= 1e-15
    z = DiceRef(x, t, [0.0] * 4, None, 1e-5, True, 0.0, 1.0)
    assert torch.isnan(z.ce) and z.total.item() == z.dice.item() and torch.isfinite(z.autograd()).all()
    assert DiceRef(x, t, None, None, 1e-5, False, 1.0, 0.0).total.item() == DiceRef(x, t).ce.item()


# ------------------------------------------------------------------------------------------------------- registry and constructors
def test_registry_names():
    from dct_amd.loss import CrossEntropyDiceLoss2d, DiceLoss, get_loss_fn
    d = get_loss_fn("dice", classes=range(1, 4), per_image=True)
    assert type(d) is DiceLoss and d.classes == [1, 2, 3] and d.per_image and d.ce_coef == 0.0 and d.dice_coef == 1.0 and d.smooth == 1e-5
    c = get_loss_fn("ce_dice", weight=[0.1, 1, 2.5, 0], dice_coef=0.5)
    assert type(c) is CrossEntropyDiceLoss2d and c.classes is None and c.ce_coef == 1.0 and c.dice_coef == 0.5 and c.ignore_index == 255
    assert c.last_dice is None and not c.per_image
    with pytest.raises(ValueError):
        get_loss_fn("no_such_loss")


def test_launch_arguments():
    from dct_amd.loss import CrossEntropyDiceLoss2d, DiceLoss
    assert DiceLoss(classes=range(1, 4)).launch_args(4) == dict(class_mask=0b1110, smooth=1e-5, per_image=False, ce_coef=0.0, dice_coef=1.0)
    assert CrossEntropyDiceLoss2d(classes=[1, 1, 0], smooth=1, per_image=True, ce_coef=2).launch_args(2) == dict(
        class_mask=0b11, smooth=1.0, per_image=True, ce_coef=2.0, dice_coef=1.0)
    assert CrossEntropyDiceLoss2d().launch_args(8)["class_mask"] == 255


def test_constructor_validation():
    from dct_amd.loss import CrossEntropyDiceLoss2d, DiceLoss
    for cls in (DiceLoss, CrossEntropyDiceLoss2d):
        with pytest.raises(ValueError, match="classes is empty"):
            cls(classes=[])
        with pytest.raises(ValueError, match="negative"):
            cls(classes=[-1, 2])
        with pytest.raises(ValueError, match="smooth"):
            cls(smooth=-1e-5)
        with pytest.raises(ValueError, match="smooth"):
            cls(smooth=float("inf"))
        with pytest.raises(ValueError, match=r"class 4 outside \[0, 4\)"):
            cls(classes=[1, 4]).launch_args(4)
    with pytest.raises(ValueError, match="3 class weights for logits of 4 classes"):
        CrossEntropyDiceLoss2d(weight=[1, 2, 3]).device_weight("cuda:0", 4)
    with pytest.raises(ValueError, match="class weights"):
        CrossEntropyDiceLoss2d(weight=[1, 1, 1]).device_weight("cuda:0", 4)
    assert CrossEntropyDiceLoss2d().device_weight("cuda:0") is None and DiceLoss().device_weight("cuda:0", 4) is None


def test_the_cpu_is_refused():
    from dct_amd.loss import CrossEntropyDiceLoss2d, DiceLoss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CrossEntropyDiceLoss2d(weight=[0.1, 1, 2.5, 0]).device_weight("cpu")
    for crit in (DiceLoss(), CrossEntropyDiceLoss2d(weight=[0.1, 1, 2.5, 0]), CrossEntropyDiceLoss2d(classes=[1])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crit(torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
