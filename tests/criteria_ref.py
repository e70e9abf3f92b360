"""The criteria of the co-training step restated in float64 plain torch, differentiable by autograd, for tests/test_step_seam_gpu.py
(and checked against the kernel tests' own references in tests/test_criteria_ref_cpu.py).

The rules are those of the docstrings in loss/loss.py and of include/dct.h, written down once more from the formulas -- nothing here
calls the package.  Every function takes float64 (or, for the fp32 restatement the tolerances are measured with, float32) logits with the
classes LAST ([..., C], the physical layout of the step's logits) and returns 0-d tensors that carry the graph to those logits:

  * ``cross_entropy``: class-weighted mean ``sum w_t l / sum w_t`` over the counted pixels (target != ignore_index and inside [0, C));
  * ``focal``: ``sum w_t (1 - p_t)^gamma l / sum w_t``, l = -log p_t;
  * ``ce_dice``: ``ce_coef`` * that cross entropy + ``dice_coef`` * (1 - mean over groups and masked classes of
    (2 I + smooth) / (S + Y + smooth)), I, S, Y over the counted pixels of the batch (one group) or of each image (``per_image``);
    an empty denominator gives D = 1; a coefficient of exactly 0 removes its term;
  * ``jsd`` / ``kl``: oracle.losses' formulas fed with the softmax of the logits (in the logits' dtype), mean over all pixels;
  * ``pseudo_label``: the hard pseudo-label consistency term.  The teachers (first-maximum argmax, confidence, threshold mask) are
    decided in fp32 from fp32 softmax maps by ``pseudo_label_ref.teachers_fp32``, exactly as the kernels' rule states them; given those
    decisions the loss is ``w sum_i sum_c n_ic -log(p_i[c] + eps)`` averaged over ALL pixels, in the logits' dtype.

``Supervised`` and ``Consistency`` carry one criterion's parameters and, beside the value, the bound on |fp32 kernel - float64| that the
criterion's own kernel test already derives (tests/focal_ref.py, tests/test_dice_loss_gpu.py, tests/pseudo_label_ref.py); the bounds of JSD
and KL are ``_jsd_ref`` and ``_kl_ref`` of tests/test_loss_kernels_scale_gpu.py, which the caller imports itself."""
import numpy as np
import torch
import torch.nn.functional as F

import oracle.losses as OL
import pseudo_label_ref as PL

IGN = 255
U = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------------------- the rules
def _counted(t, C, ignore_index):
    return (t != ignore_index) & (t >= 0) & (t < C)


def _class_weights(weight, C, dtype):
    """The class weights as the kernels read them: the fp32 copy of ``weight`` (None: all ones), taken to ``dtype``."""
    return torch.ones(C, dtype=dtype) if weight is None else torch.tensor([float(v) for v in weight], dtype=torch.float32).to(dtype)


def cross_entropy(x, t, weight=None, ignore_index=IGN):
    """x [..., C], t [...] int64 -> sum w_t l / sum w_t."""
    C = x.shape[-1]
    x, t = x.reshape(-1, C), t.reshape(-1)
    keep = _counted(t, C, ignore_index)
    tc = torch.where(keep, t, torch.zeros_like(t))
    w = _class_weights(weight, C, x.dtype)
    wi = w[tc] * keep.to(x.dtype)
    l = torch.logsumexp(x, 1) - x.gather(1, tc[:, None])[:, 0]
    return (wi * torch.where(keep, l, torch.zeros_like(l))).sum() / wi.sum()


def focal(x, t, weight=None, gamma=2.0, ignore_index=IGN):
    """x [..., C], t [...] -> sum w_t (1 - p_t)^gamma (-log p_t) / sum w_t."""
    C = x.shape[-1]
    x, t = x.reshape(-1, C), t.reshape(-1)
    keep = _counted(t, C, ignore_index)
    tc = torch.where(keep, t, torch.zeros_like(t))
    w = _class_weights(weight, C, x.dtype)
    wi = w[tc] * keep.to(x.dtype)
    logp = torch.log_softmax(x, 1)
    onehot = F.one_hot(tc, C).to(x.dtype)
    l = -(logp * onehot).sum(1)
    q = (torch.exp(logp) * (1 - onehot)).sum(1)                    # 1 - p_t without the cancellation
    f = wi * q.pow(gamma) * l if gamma != 0 else wi * l
    return torch.where(keep, f, torch.zeros_like(f)).sum() / wi.sum()


def soft_dice(x, t, classes=None, smooth=1e-5, per_image=False, ignore_index=IGN):
    """x [B, PPI, C], t [B, PPI] -> 1 - mean_{g, c in classes} (2 I + smooth) / (S + Y + smooth)."""
    B, PPI, C = x.shape
    keep = _counted(t, C, ignore_index)
    tc = torch.where(keep, t, torch.zeros_like(t))
    k = keep[..., None].to(x.dtype)
    p = torch.softmax(x, -1)
    y = F.one_hot(tc, C).to(x.dtype) * k
    dims = (1,) if per_image else (0, 1)
    G = B if per_image else 1
    I, S, Y = ((p * y).sum(dims).reshape(G, C), (p * k).sum(dims).reshape(G, C), y.sum(dims).reshape(G, C))
    num, den = 2 * I + smooth, S + Y + smooth
    empty = den == 0
    D = torch.where(empty, torch.ones_like(den), num / torch.where(empty, torch.ones_like(den), den))
    cls = list(range(C)) if classes is None else sorted(set(classes))
    return 1 - D[:, cls].sum() / (G * len(cls))


def ce_dice(x, t, weight=None, classes=None, smooth=1e-5, per_image=False, ce_coef=1.0, dice_coef=1.0, ignore_index=IGN):
    total = torch.zeros((), dtype=x.dtype)
    if ce_coef != 0:
        total = total + ce_coef * cross_entropy(x, t, weight, ignore_index)
    if dice_coef != 0:
        total = total + dice_coef * soft_dice(x, t, classes, smooth, per_image, ignore_index)
    return total


def _nchw(x):
    """[P, C] -> the [1, C, P, 1] probabilities-first layout of oracle.losses."""
    return x.t().reshape(1, x.shape[1], x.shape[0], 1)


def jsd(xs):
    """xs: S logits [..., C] -> mean over the pixels of H(mean_i p_i) - mean_i H(p_i)."""
    C = xs[0].shape[-1]
    return OL.jsd_2d([_nchw(torch.softmax(x.reshape(-1, C), 1)) for x in xs]).mean()


def kl(x_p, x_y, eps=1e-10):
    """mean over the pixels of sum_c y (log(y + eps) - log(p + eps)), p = softmax(x_p), y = softmax(x_y)."""
    C = x_p.shape[-1]
    return OL.kl_divergence_2d(_nchw(torch.softmax(x_p.reshape(-1, C), 1)), _nchw(torch.softmax(x_y.reshape(-1, C), 1)), reduce=True, eps=eps)


def first_max(x):
    """int64 [...]: the first maximum along the last axis (dct_argmax's rule)."""
    return torch.from_numpy(PL.first_max(x.detach().numpy())[0])


def softmax32(x):
    """The fp32 softmax map [P, C] of fp32 logits as a numpy array: what the teachers are decided from."""
    C = x.shape[-1]
    return torch.softmax(x.detach().float().reshape(-1, C), 1).numpy()


def near_ties(p32s, teacher, tau, near):
    """bool [P]: pixels where a hard decision sits on a rounding edge -- a teacher vector (each view for ``cross``, the mean for
    ``ensemble``) whose two best classes are within ``near``, or whose confidence is within ``near`` of ``tau``."""
    ps = [torch.from_numpy(np.asarray(p)).double() for p in p32s]
    vecs = ps if teacher == PL.CROSS else [sum(ps) / len(ps)]
    flag = torch.zeros(ps[0].shape[0], dtype=torch.bool)
    for v in vecs:
        top = v.topk(2, dim=1).values
        flag |= (top[:, 0] - top[:, 1]) < near
        if tau > 0:
            flag |= (top[:, 0] - tau).abs() < near
    return flag


def pseudo_label(xs, n, teacher, eps=1e-10):
    """xs: S logits [..., C]; n [S, P, C]: the kept teacher terms of class c that student i meets (``pseudo_label_ref.term_counts`` of the
    fp32 decisions) -> w sum_i sum_c n_ic -log(p_i[c] + eps), averaged over all P pixels."""
    S, C = len(xs), xs[0].shape[-1]
    w = PL.weight(teacher, S)
    total = 0.0
    for i, x in enumerate(xs):
        p = torch.softmax(x.reshape(-1, C), 1)
        ni = n[i].to(p.dtype)
        total = total + (ni * -torch.log(torch.where(ni > 0, p, torch.ones_like(p)) + eps)).sum()
    return w * total / xs[0].reshape(-1, C).shape[0]


# ------------------------------------------------------------------------------------------------- criteria with their bounds
def _softmax_bound(x64):
    """(p, e_p): the float64 softmax of [P, C] logits and the bound (C + 6 + |x_c - max|) U p_c on an fp32 softmax
    (tests/test_loss_kernels_scale_gpu.py::test_ce_at_scale; ``ep`` of tests/test_dice_loss_gpu.py)."""
    C = x64.shape[1]
    p = torch.softmax(x64, 1)
    spread = (x64 - x64.max(1, keepdim=True).values).abs()
    return p, (C + 6 + spread) * U * p


class Supervised:
    """One supervised criterion: ``name`` in cross_entropy | focal | ce_dice | dice with the keyword arguments of the registry."""

    def __init__(self, name, **kw):
        self.name, self.kw = name, dict(kw)
        self.ignore_index = kw.get("ignore_index", IGN)

    def module(self):
        from dct_amd.loss import get_loss_fn
        return get_loss_fn(self.name, **self.kw)

    def weight(self, C):
        w = self.kw.get("weight")
        return None if w is None else torch.tensor([float(v) for v in w], dtype=torch.float32)

    def value(self, x, t):
        """x [B, H, W, C] in float64 (or float32), t [B, H, W] -> the criterion's value with a graph to x."""
        B, C = x.shape[0], x.shape[-1]
        k = self.kw
        if self.name == "cross_entropy":
            return cross_entropy(x, t, k.get("weight"), self.ignore_index)
        if self.name == "focal":
            return focal(x, t, k.get("weight"), float(k.get("gamma", 2.0)), self.ignore_index)
        cc, dc = (0.0, 1.0) if self.name == "dice" else (float(k.get("ce_coef", 1.0)), float(k.get("dice_coef", 1.0)))
        return ce_dice(x.reshape(B, -1, C), t.reshape(B, -1), k.get("weight") if self.name != "dice" else None, k.get("classes"),
                       float(k.get("smooth", 1e-5)), bool(k.get("per_image", False)), cc, dc, self.ignore_index)

    def bounds(self, x32, t):
        """(value bound, gradient bound [B, H, W, C]) on |fp32 kernel - float64| for the criterion on fp32 logits ``x32`` with gradient
        factor 1, from the criterion's kernel test: tests/focal_ref.py (``ce_bounds`` as tests/test_weighted_ce_gpu.py applies it to the
        mean: k = 6; ``Ref.value`` / ``Ref.grad`` for focal) and ``_Bounds`` of tests/test_dice_loss_gpu.py."""
        import focal_ref as FR
        B, C = x32.shape[0], x32.shape[-1]
        k = self.kw
        t_ref = torch.where(_counted(t, C, self.ignore_index), t, torch.full_like(t, FR.IGN)).reshape(-1)
        w = self.weight(C)
        if self.name in ("cross_entropy", "focal"):
            gamma = float(k.get("gamma", 2.0)) if self.name == "focal" else 0.0
            r = FR.Ref(x32.reshape(-1, C), t_ref, torch.ones(C) if w is None else w, C, gamma)
            loss, tol = r.value(FR.MEAN)
            if self.name == "focal":
                _, gb = r.grad(loss, 1.0 / r.D, mean=True)
            else:
                num_tol, _, grad_bound = FR.ce_bounds(r)
                tol = num_tol / r.D + (FR.SUM_DEPTH + 2) * U * abs(loss.item())
                gb = grad_bound(1.0 / r.D, 6)
            return tol, gb.reshape(x32.shape)
        from test_dice_loss_cpu import DiceRef
        from test_dice_loss_gpu import _Bounds
        cc, dc = (0.0, 1.0) if self.name == "dice" else (float(k.get("ce_coef", 1.0)), float(k.get("dice_coef", 1.0)))
        xb = x32.reshape(B, -1, C)
        r = DiceRef(xb, t_ref.reshape(B, -1), None if self.name == "dice" else w, k.get("classes"), float(k.get("smooth", 1e-5)),
                    bool(k.get("per_image", False)), cc, dc)
        bd = _Bounds(r, xb)
        _, gb = bd.grad(1.0)
        return bd.e_total, gb.reshape(x32.shape)


class Consistency:
    """One consistency criterion: ``name`` in jsd | cps | pseudo_label with its threshold."""

    def __init__(self, name, tau=0.0, eps=1e-10):
        self.name, self.tau, self.eps = name, float(tau), float(eps)
        self.teacher = {"jsd": None, "cps": PL.CROSS, "pseudo_label": PL.ENSEMBLE}[name]

    def module(self):
        from dct_amd.loss import get_loss_fn
        return get_loss_fn("jsd") if self.name == "jsd" else get_loss_fn(self.name, threshold=self.tau, eps=self.eps)

    def decide(self, x32s, near):
        """The fp32 teachers of S fp32 logits [..., C]: (n [S, P, C], kept fraction, near-tie pixels bool [P])."""
        S, C = len(x32s), x32s[0].shape[-1]
        p32 = [softmax32(x) for x in x32s]
        k, m, _ = PL.teachers_fp32(p32, self.teacher, self.tau)
        return PL.term_counts(k, m, self.teacher, S, C), float(m.mean()), near_ties(p32, self.teacher, self.tau, near)

    def value(self, xs, n=None):
        return jsd(xs) if self.name == "jsd" else pseudo_label(xs, n, self.teacher, self.eps)

    def near_value_slack(self, x32s, flag):
        """The most a near-tie pixel can move the mean: its teacher terms swapped for the dearest ones, i.e. at most
        max_i,c -log(p_i[c] + eps) per pixel (the map is a weighted mean of such terms with weights summing to at most 1)."""
        if not bool(flag.any()):
            return 0.0
        P = flag.numel()
        worst = torch.stack([-torch.log(torch.from_numpy(softmax32(x)).double()[flag] + self.eps).max(1).values for x in x32s]).max(0).values
        return worst.sum().item() / P

    def bounds(self, x32s, n, g=1.0):
        """(value bound, [gradient bound [P, C]] per view) of the pseudo-label term from tests/pseudo_label_ref.py (``map_and_grad``,
        ``logit_grad`` and the step's value tolerance of tests/test_pseudo_label_gpu.py), evaluated on the float64 softmax.  Those bounds
        start from the fp32 probabilities a kernel holds; the reference here starts from the logits, so the fp32 softmax's own bound e_p
        (``_softmax_bound``) is carried through both formulas to first order:
          value:     |d -log(p + eps)| <= e_p / (p + eps) per kept term;
          gradient:  o_c = g w (-n_c r_c + p_c sum_k n_k r_k) with r = p / (p + eps), |dr| <= e_p eps / (p + eps)^2:
                     |do_c| <= |g| w (n_c dr_c + e_p_c sum_k n_k r_k + p_c sum_k n_k dr_k).
        None for JSD, whose bound is tests/test_loss_kernels_scale_gpu.py's ``_jsd_ref``."""
        if self.name == "jsd":
            return None
        S, C = len(x32s), x32s[0].shape[-1]
        w = PL.weight(self.teacher, S)
        pe = [_softmax_bound(x.detach().double().reshape(-1, C)) for x in x32s]
        p64 = [p for p, _ in pe]
        P = p64[0].shape[0]
        v, vb, d, _ = PL.map_and_grad([p.numpy() for p in p64], n, self.teacher, self.eps, fp32_sum=False)
        soft_v = sum((w * n[i] * e / (p + self.eps)).sum() for i, (p, e) in enumerate(pe)).item()
        tol = (vb.sum().item() + soft_v + PL.SUM_DEPTH * U * v.abs().sum().item()) / P + 2 * U * abs(v.mean().item()) + PL.TINY
        gbs = []
        for i, (p, e) in enumerate(pe):
            _, gb = PL.logit_grad(p.numpy(), d[i], g / P, C)
            r = p / (p + self.eps)
            dr = e * self.eps / (p + self.eps) ** 2
            ni = n[i]
            soft = abs(g / P) * w * (ni * dr + e * (ni * r).sum(1, keepdim=True) + p * (ni * dr).sum(1, keepdim=True))
            # (p + eps is formed in fp32 by the kernels, exactly here: one more rounding of d)
            gbs.append(gb + soft + U * abs(g / P) * p * (d[i].abs() + (d[i] * p).abs().sum(1, keepdim=True)))
        return tol, gbs
