"""Loss modules of the hot path with the reference's signatures
(/root/reference/generalframework/loss/loss.py) on top of the fused HIP kernels (K10).

``CrossEntropyLoss2d`` (:12-25), ``Entropy_2D`` (:70-84), ``KL_Divergence_2D`` (:110-134),
``JSD_2D`` (:183-196).  Inputs/outputs are logical NCHW torch tensors exactly as in the
reference; internally every module works on the physical NHWC fp32 image of its input (free
for tensors produced by dct_amd networks, which are channels_last already).

The reference asserts ``simplex(p)`` (a host-synchronising ``allclose``) on every call; here
that check runs only when ``dct_amd.loss.DEBUG_ASSERTS`` is True, so the stream is never
drained in production.  HIP only -- CPU tensors are rejected.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from .. import hip_ops as K

DEBUG_ASSERTS = False


def _pc(t: torch.Tensor) -> torch.Tensor:
    """logical [B,C,H,W] -> physical NHWC fp32 dense (no copy when already so)."""
    if not t.is_cuda:
        raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
    p = t.permute(0, 2, 3, 1)
    if p.dtype != torch.float32 or not p.is_contiguous():
        p = p.to(torch.float32).contiguous()
    return p


def _nchw(p: torch.Tensor) -> torch.Tensor:
    return p.permute(0, 3, 1, 2)


def _simplex(t: torch.Tensor, axis=1) -> bool:
    s = t.sum(axis).type(torch.float32)
    return torch.allclose(s, torch.ones_like(s))


def _targets(targets):
    t = targets.reshape(-1)
    if t.dtype != torch.int64 or not t.is_contiguous():
        t = t.to(torch.int64).contiguous()
    return t


class _ReducedFn(torch.autograd.Function):
    """The mean or sum of one criterion on a hip_ops family: ``family`` is 'ce', 'ce_weighted' or 'focal' (its ``_fwd`` and ``_bwd``
    wrappers are called), ``kw`` their keyword arguments (``ignore_index`` and, beyond the plain family, ``weight`` -- the fp32 device
    buffer or None for all ones --, ``reduction`` and ``gamma``)."""

    @staticmethod
    def forward(ctx, logits, targets, family, kw):
        lp = _pc(logits)
        t = _targets(targets)
        out = getattr(K, family + "_fwd")(lp, t, lp.shape[3], **kw)
        ctx.save_for_backward(lp, t, out)
        ctx.family, ctx.kw = family, kw
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lp, t, out = ctx.saved_tensors
        dl = torch.empty_like(lp)
        g = g.to(torch.float32).contiguous()
        getattr(K, ctx.family + "_bwd")(lp, t, lp.shape[3], out[1:2], dl, gscale=g, **ctx.kw)
        return _nchw(dl), None, None, None


class _MapFn(torch.autograd.Function):
    """The [B, H, W] map of ``reduce=False`` on a hip_ops family: 'ce_map' (w_t * (logsumexp(x) - x_t)) or 'focal_map'
    (w_t (1 - p_t)^gamma (-log p_t)); ``kw``: ``weight``, ``ignore_index`` and focal's ``gamma``."""

    @staticmethod
    def forward(ctx, logits, targets, family, kw):
        lp = _pc(logits)
        t = _targets(targets)
        ctx.save_for_backward(lp, t)
        ctx.family, ctx.kw = family, kw
        return getattr(K, family + "_fwd")(lp, t, lp.shape[3], **kw).view(lp.shape[:3])

    @staticmethod
    def backward(ctx, g):
        lp, t = ctx.saved_tensors
        dl = torch.empty_like(lp)
        getattr(K, ctx.family + "_bwd")(lp, t, lp.shape[3], g.to(torch.float32).contiguous().view(-1), dl, **ctx.kw)
        return _nchw(dl), None, None, None


def _ce_reduced(outputs, targets, w, reduction, ignore_index):
    """The class-weighted cross entropy under ``reduction``; None (all-ones) weights under the mean run the plain family."""
    if w is None and reduction == K.CE_MEAN:
        return _ReducedFn.apply(outputs, targets, 'ce', dict(ignore_index=ignore_index))
    return _ReducedFn.apply(outputs, targets, 'ce_weighted', dict(weight=w, reduction=reduction, ignore_index=ignore_index))


class _ClassWeighted(nn.Module):
    """The class weights of a criterion: kept on the module as passed, read by the kernels from an fp32 copy on the device that is made
    once per device on first use (``device_weight``) and never refreshed from ``weight``."""

    def _set_weight(self, weight):
        self.weight = weight
        self._host_weight = None if weight is None else [float(w) for w in weight]
        self._unit = self._host_weight is None or all(w == 1.0 for w in self._host_weight)
        self._device_weights = {}

    def device_weight(self, device, C=None):
        """The fp32 [C] buffer of the class weights on ``device`` that the kernels read (None when the weights are None or all ones:
        the kernels then take every weight as 1)."""
        name = type(self).__name__
        if self._unit:
            if C is not None and self._host_weight is not None and len(self._host_weight) != C:
                raise ValueError(f"dct_amd {name}: {len(self._host_weight)} class weights for logits of {C} classes")
            return None
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if C is not None and len(self._host_weight) != C:
            raise ValueError(f"dct_amd {name}: {len(self._host_weight)} class weights for logits of {C} classes")
        buf = self._device_weights.get(device)
        if buf is None:
            buf = self._device_weights[device] = torch.tensor(self._host_weight, dtype=torch.float32, device=device)
        return buf


class CrossEntropyLoss2d(_ClassWeighted):
    """``nn.NLLLoss(weight, reduce=, size_average=, ignore_index=)`` of the log-softmax, as the reference builds it: the class-weighted
    mean ``sum w_t l / sum w_t`` (default), the sum (``reduce=True, size_average=False``) or the [B, H, W] map ``w_t l``
    (``reduce=False``, whatever ``size_average`` is) -- torch's ``F.cross_entropy(weight=, ignore_index=, reduction=)``.

    ``weight`` (None, or C values) stays on the module as passed.  The kernels read an fp32 copy on the device, made once per device
    on first use (``device_weight``) and never refreshed from ``weight``: nothing is copied from the host per call, and an in-place
    update of that buffer (``crit.device_weight(dev).copy_(...)``) is what the next call -- and every replay of a captured step --
    sees.  None or all-ones weights with the mean reduction run the unweighted kernels."""

    def __init__(self, weight=None, reduce=True, size_average=True, ignore_index=255):
        super().__init__()
        self._set_weight(weight)
        self.reduce, self.size_average = reduce, size_average
        self.reduction = 'none' if not reduce else ('mean' if size_average else 'sum')
        self.ignore_index = ignore_index

    def forward(self, outputs, targets):
        assert outputs.dim() == 4 and targets.dim() == 3, (outputs.shape, targets.shape)
        if not outputs.is_cuda:
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        w = self.device_weight(outputs.device, outputs.shape[1])
        if self.reduction == 'none':
            return _MapFn.apply(outputs, targets, 'ce_map', dict(weight=w, ignore_index=self.ignore_index))
        return _ce_reduced(outputs, targets, w, K.CE_MEAN if self.reduction == 'mean' else K.CE_SUM, self.ignore_index)


class FocalLoss2d(_ClassWeighted):
    """Focal loss of Lin et al. (ICCV 2017) in its softmax form: ``w_t (1 - p_t)^gamma (-log p_t)`` per pixel (the rule: include/dct.h,
    dct_focal_*), which turns the easy pixels down instead of whole classes.  ``gamma``: finite and >= 0; 0 is the class-weighted cross
    entropy (computed by the focal kernels all the same).  ``weight`` (the per-class alpha), ``reduce``, ``size_average`` and
    ``ignore_index`` as on ``CrossEntropyLoss2d``: the mean is ``sum f / sum w_t`` over the counted pixels -- with ``weight=None`` the
    mean over the counted pixels of most published focal-loss code --, the sum ``sum f``, the map ``f``; the weights are read from
    ``device_weight``'s buffer on the device."""

    def __init__(self, gamma=2.0, weight=None, reduce=True, size_average=True, ignore_index=255):
        super().__init__()
        try:
            self.gamma = float(gamma)
        except (TypeError, ValueError):
            raise ValueError(f"dct_amd {type(self).__name__}: gamma must be a number, got {gamma!r}")
        if not (0.0 <= self.gamma < float('inf')):
            raise ValueError(f"dct_amd {type(self).__name__}: gamma must be finite and >= 0, got {gamma!r}")
        self._set_weight(weight)
        self.reduce, self.size_average = reduce, size_average
        self.reduction = 'none' if not reduce else ('mean' if size_average else 'sum')
        self.ignore_index = ignore_index

    def launch_args(self, C):
        """The keyword arguments of hip_ops.focal_* beyond the weights (the same for every ``C``)."""
        return dict(gamma=self.gamma)

    def forward(self, outputs, targets):
        assert outputs.dim() == 4 and targets.dim() == 3, (outputs.shape, targets.shape)
        if not outputs.is_cuda:
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        w = self.device_weight(outputs.device, outputs.shape[1])
        kw = dict(weight=w, gamma=self.gamma, ignore_index=self.ignore_index)
        if self.reduction == 'none':
            return _MapFn.apply(outputs, targets, 'focal_map', kw)
        return _ReducedFn.apply(outputs, targets, 'focal', dict(kw, reduction=K.CE_MEAN if self.reduction == 'mean' else K.CE_SUM))


class _TopKFn(torch.autograd.Function):
    """The top-k cross entropy on dct_topk_ce_*.  Returns the value and, without a gradient, ``out2`` = (value, tau) and ``counts4`` =
    (K, N, n_gt, n_eq); the backward launch compares the map the forward launch stored."""

    @staticmethod
    def forward(ctx, logits, targets, weight, k_percent, ignore_index):
        lp = _pc(logits)
        t = _targets(targets)
        out2, counts4, vmap = K.topk_ce_fwd(lp, t, lp.shape[3], weight, k_percent, ignore_index)
        ctx.save_for_backward(lp, t, vmap, out2, counts4)
        ctx.weight, ctx.ignore_index = weight, ignore_index
        info = out2.clone()
        ctx.mark_non_differentiable(info, counts4)
        return out2[0], info, counts4

    @staticmethod
    def backward(ctx, g, *_):
        lp, t, vmap, out2, counts4 = ctx.saved_tensors
        dl = torch.empty_like(lp)
        g = g.to(torch.float32).contiguous()
        K.topk_ce_bwd(lp, t, lp.shape[3], vmap, out2, counts4, dl, weight=ctx.weight, gscale=g, ignore_index=ctx.ignore_index)
        return _nchw(dl), None, None, None, None


class TopKCrossEntropyLoss2d(_ClassWeighted):
    """Top-k cross entropy (nnU-Net's ``TopKLoss``, online hard-example mining): the mean of the per-pixel class-weighted cross entropy
    ``w_t l`` over the hardest ``k`` % of the counted pixels only (the rule: include/dct.h, dct_topk_ce_*), so that the mass of easy
    background stops diluting the mean.  ``k``: a number, finite, 0 < k <= 100; 100 is ``sum w_t l / N`` (with ``weight=None`` the plain
    mean cross entropy).  ``weight`` and ``ignore_index`` as on ``CrossEntropyLoss2d``.  Returns a scalar only.  After a call
    ``last_topk`` = (``out2``, ``counts4``): the device tensors (value, tau) and int64 (K, N, n_gt, n_eq) for logging (nothing
    synchronises)."""

    def __init__(self, k=10.0, weight=None, ignore_index=255):
        super().__init__()
        try:
            self.k = float(k)
        except (TypeError, ValueError):
            raise ValueError(f"dct_amd {type(self).__name__}: k must be a number, got {k!r}")
        if not (0.0 < self.k <= 100.0):
            raise ValueError(f"dct_amd {type(self).__name__}: k must be finite with 0 < k <= 100, got {k!r}")
        self._set_weight(weight)
        self.reduction = 'mean'
        self.ignore_index = ignore_index
        self.last_topk = None

    def launch_args(self, C):
        """The keyword arguments of hip_ops.topk_ce_* beyond the weights (the same for every ``C``)."""
        return dict(k_percent=self.k)

    def forward(self, outputs, targets):
        assert outputs.dim() == 4 and targets.dim() == 3, (outputs.shape, targets.shape)
        if not outputs.is_cuda:
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        w = self.device_weight(outputs.device, outputs.shape[1])
        value, out2, counts4 = _TopKFn.apply(outputs, targets, w, self.k, self.ignore_index)
        self.last_topk = (out2, counts4)
        return value


class _OverlapFn(torch.autograd.Function):
    """``ce_coef`` ce + coefficient * overlap term on one hip_ops family of the overlap kernels: ``family`` is 'ce_dice' or 'ce_tversky' (its
    ``_fwd`` and ``_bwd`` wrappers are called), ``rule`` the criterion's ``launch_args``.  Returns the total and, without a gradient, the [G, C] table
    of the index (D_gc, T_gc)."""

    @staticmethod
    def forward(ctx, logits, targets, weight, family, rule, ignore_index):
        lp = _pc(logits)
        t = _targets(targets)
        out4, index_gc, sums = getattr(K, family + "_fwd")(lp, t, lp.shape[3], weight, ignore_index=ignore_index, **rule)
        ctx.save_for_backward(lp, t, out4, sums)
        ctx.weight, ctx.family, ctx.rule, ctx.ignore_index = weight, family, rule, ignore_index
        ctx.mark_non_differentiable(index_gc)
        return out4[0], index_gc

    @staticmethod
    def backward(ctx, g, _):
        lp, t, out4, sums = ctx.saved_tensors
        dl = torch.empty_like(lp)
        g = g.to(torch.float32).contiguous()
        getattr(K, ctx.family + "_bwd")(lp, t, lp.shape[3], out4, sums, dl, weight=ctx.weight, gscale=g, ignore_index=ctx.ignore_index, **ctx.rule)
        return _nchw(dl), None, None, None, None, None


class _OverlapLoss2d(_ClassWeighted):
    """What the overlap criteria share: the class weights, ``classes``, ``smooth``, ``per_image``, ``ignore_index`` and the call.  A
    family names its hip_ops functions' prefix (``family``), its coefficient (``_coef``) and the attribute that publishes the index table
    (``_last``), and adds its own parameters to the launch arguments (``_rule_args``)."""
    family = _coef = _last = None

    def __init__(self, weight, ce_coef, coef, classes, smooth, per_image, ignore_index):
        super().__init__()
        who = type(self).__name__
        self._set_weight(weight)
        self.ce_coef = _number(ce_coef, "ce_coef", who)
        setattr(self, self._coef, _number(coef, self._coef, who))
        self.classes = _class_list(classes, who)
        self.smooth = _number(smooth, "smooth", who)
        if not (0.0 <= self.smooth < float('inf')):
            raise ValueError(f"dct_amd {who}: smooth must be finite and >= 0, got {smooth!r}")
        self.per_image = bool(per_image)
        self.ignore_index = ignore_index
        setattr(self, self._last, None)

    def _rule_args(self):
        return {}

    def launch_args(self, C):
        """The keyword arguments of the family's hip_ops functions for logits of ``C`` classes (checks ``classes`` against C)."""
        return dict(class_mask=_class_mask(self.classes, C, type(self).__name__), smooth=self.smooth, **self._rule_args(),
                    per_image=self.per_image, ce_coef=self.ce_coef, **{self._coef: getattr(self, self._coef)})

    def forward(self, outputs, targets):
        assert outputs.dim() == 4 and targets.dim() == 3, (outputs.shape, targets.shape)
        if not outputs.is_cuda:
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        rule = self.launch_args(outputs.shape[1])
        w = self.device_weight(outputs.device, outputs.shape[1])
        total, index_gc = _OverlapFn.apply(outputs, targets, w, self.family, rule, self.ignore_index)
        setattr(self, self._last, index_gc)
        return total


class CrossEntropyDiceLoss2d(_OverlapLoss2d):
    """``ce_coef`` * class-weighted mean cross entropy + ``dice_coef`` * soft Dice loss of the softmax (the rule: include/dct.h,
    dct_ce_dice_*), in one forward and one backward launch pair.  ``classes``: the class indices of the Dice mean (None: all;
    ``range(1, C)``: foreground only); ``per_image``: one Dice per image and class instead of one per class over the batch; ``weight``
    and ``ignore_index`` as on ``CrossEntropyLoss2d``.  After a call ``last_dice`` is the [G, C] device tensor of D_gc of every class
    (nothing synchronises).  A coefficient of exactly 0 removes its term."""
    family, _coef, _last = "ce_dice", "dice_coef", "last_dice"

    def __init__(self, weight=None, ce_coef=1.0, dice_coef=1.0, classes=None, smooth=1e-5, per_image=False, ignore_index=255):
        super().__init__(weight, ce_coef, dice_coef, classes, smooth, per_image, ignore_index)


class DiceLoss(CrossEntropyDiceLoss2d):
    """Soft Dice loss alone: ``1 - mean_{g, c in classes} (2 I + smooth) / (S + Y + smooth)`` of the softmax (``CrossEntropyDiceLoss2d``
    with the cross-entropy term removed)."""

    def __init__(self, classes=None, smooth=1e-5, per_image=False, ignore_index=255):
        super().__init__(None, 0.0, 1.0, classes, smooth, per_image, ignore_index)


def _number(value, what, who):
    try:
        return float(value)
    except (TypeError, ValueError):
        raise ValueError(f"dct_amd {who}: {what} must be a number, got {value!r}")


class CrossEntropyTverskyLoss2d(_OverlapLoss2d):
    """``ce_coef`` * class-weighted mean cross entropy + ``tversky_coef`` * focal Tversky loss of the softmax (Salehi et al. 2017; Abraham &
    Khan 2019; the rule: include/dct.h, dct_ce_tversky_*), in one forward and one backward launch pair.  Per group and class the index is
    ``T = (I + smooth) / (I + alpha FP + beta FN + smooth)`` and the loss the mean of ``(1 - T)^(1 / gamma)``: ``alpha`` weighs the false
    positives, ``beta`` the false negatives (both finite and >= 0, not both 0; 0.5 / 0.5 is Dice, 1 / 1 Jaccard), ``gamma`` (finite, > 0;
    1: plain Tversky) is the focal parameter.  ``classes``, ``smooth``, ``per_image``, ``weight`` and ``ignore_index`` as on
    ``CrossEntropyDiceLoss2d``.  After a call ``last_tversky`` is the [G, C] device tensor of T_gc of every class (nothing synchronises).
    A coefficient of exactly 0 removes its term."""
    family, _coef, _last = "ce_tversky", "tversky_coef", "last_tversky"

    def __init__(self, weight=None, ce_coef=1.0, tversky_coef=1.0, alpha=0.3, beta=0.7, gamma=1.0, classes=None, smooth=1e-5,
                 per_image=False, ignore_index=255):
        super().__init__(weight, ce_coef, tversky_coef, classes, smooth, per_image, ignore_index)
        who = type(self).__name__
        self.alpha, self.beta, self.gamma = _number(alpha, "alpha", who), _number(beta, "beta", who), _number(gamma, "gamma", who)
        for name, v, given in (("alpha", self.alpha, alpha), ("beta", self.beta, beta)):
            if not (0.0 <= v < float('inf')):
                raise ValueError(f"dct_amd {who}: {name} must be finite and >= 0, got {given!r}")
        # (the kernels take the three as fp32: what is 0 or infinite there is refused here)
        a32, b32, g32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (self.alpha, self.beta, self.gamma))
        if a32 + b32 == 0.0 or a32 == float('inf') or b32 == float('inf'):
            raise ValueError(f"dct_amd {who}: alpha + beta must be > 0 and finite in fp32, got {alpha!r}, {beta!r}")
        if not (0.0 < self.gamma < float('inf')) or not (0.0 < g32 < float('inf')):
            raise ValueError(f"dct_amd {who}: gamma must be finite and > 0, got {gamma!r}")

    def _rule_args(self):
        return dict(alpha=self.alpha, beta=self.beta, gamma=self.gamma)


class FocalTverskyLoss(CrossEntropyTverskyLoss2d):
    """Focal Tversky loss alone: ``mean_{g, c in classes} (1 - T_gc)^(1 / gamma)`` (``CrossEntropyTverskyLoss2d`` with the cross-entropy
    term removed; the defaults are the paper's)."""

    def __init__(self, alpha=0.3, beta=0.7, gamma=4.0 / 3.0, classes=None, smooth=1e-5, per_image=False, ignore_index=255):
        super().__init__(None, 0.0, 1.0, alpha, beta, gamma, classes, smooth, per_image, ignore_index)


class TverskyLoss(CrossEntropyTverskyLoss2d):
    """Tversky loss alone: ``1 - mean_{g, c in classes} T_gc`` (``CrossEntropyTverskyLoss2d`` with the cross-entropy term removed and
    ``gamma`` = 1)."""

    def __init__(self, alpha=0.3, beta=0.7, classes=None, smooth=1e-5, per_image=False, ignore_index=255):
        super().__init__(None, 0.0, 1.0, alpha, beta, 1.0, classes, smooth, per_image, ignore_index)


def _spacing2(spacing, who):
    try:
        sy, sx = (float(s) for s in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"dct_amd {who}: spacing must be two numbers (sy, sx), got {spacing!r}")
    if not (0.0 < sy < float('inf') and 0.0 < sx < float('inf')):
        raise ValueError(f"dct_amd {who}: spacing must be positive and finite, got {spacing!r}")
    return sy, sx


def _class_list(classes, who):
    """``classes`` as a sorted list of distinct ints, None for all; empty and negative are refused here, ``>= C`` by ``_class_mask``."""
    if classes is None:
        return None
    classes = sorted({int(c) for c in classes})
    if not classes:
        raise ValueError(f"dct_amd {who}: classes is empty")
    if classes[0] < 0:
        raise ValueError(f"dct_amd {who}: class {classes[0]} is negative")
    return classes


def _class_mask(classes, C, who):
    if classes is not None and classes[-1] >= C:
        raise ValueError(f"dct_amd {who}: class {classes[-1]} outside [0, {C})")
    return (1 << C) - 1 if classes is None else sum(1 << c for c in classes)


def signed_distance_map(gt, C, classes=None, spacing=(1., 1.)):
    """The signed Euclidean distance maps of the boundary loss (Kervadec's ``one_hot2dist``) on the device: ``gt`` [B, H, W] or
    [B, 1, H, W] class indices -> fp32 [B, C, H, W] (the logical view of the NHWC buffer the kernels write), per image and class the
    distance to the class's contour in units of ``spacing`` = (sy, sx), negative inside (the rule: include/dct.h).  A class that is
    absent from an image, fills it, or is not in ``classes`` (None: all) has an all-zero map.  Not differentiable."""
    who = "signed_distance_map"
    mask_classes = _class_list(classes, who)
    _class_mask(mask_classes, C, who)
    if not gt.is_cuda:
        raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
    if gt.dim() == 4 and gt.shape[1] == 1:
        gt = gt[:, 0]
    assert gt.dim() == 3, gt.shape
    with torch.no_grad():
        return _nchw(K.signed_distance(gt, C, mask_classes, _spacing2(spacing, who)))


class _BoundaryFn(torch.autograd.Function):
    """The boundary term on dct_boundary_*; ``phi``: the fp32 NHWC map [B, H, W, C]."""

    @staticmethod
    def forward(ctx, logits, targets, phi, mask, ignore_index):
        lp = _pc(logits)
        if lp.data_ptr() % 16:              # (a dense view that starts inside its storage: the kernels read 16 bytes at a time)
            lp = lp.clone()
        t = _targets(targets)
        out = K.boundary_fwd(lp, t, phi, lp.shape[3], mask, ignore_index)
        ctx.save_for_backward(lp, t, phi, out)
        ctx.mask, ctx.ignore_index = mask, ignore_index
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lp, t, phi, out = ctx.saved_tensors
        dl = torch.empty_like(lp)
        g = g.to(torch.float32).contiguous()
        K.boundary_bwd(lp, t, phi, lp.shape[3], out[1:2], dl, class_mask=ctx.mask, gscale=g, ignore_index=ctx.ignore_index)
        return _nchw(dl), None, None, None, None


class BoundaryLoss(nn.Module):
    """Boundary loss of Kervadec et al.: the mean over counted pixels and ``classes`` of softmax x signed distance to the ground-truth
    contour (the rule: include/dct.h, dct_boundary_*).  ``classes``: the class indices of the mean (None: all; the paper leaves the
    background out: pass ``range(1, C)``); ``spacing`` = (sy, sx): the pixel size the distances are measured in.

    ``forward(outputs, targets, dist_map=None)``: a caller that holds the map of this batch (``signed_distance_map`` under the same
    ``classes`` and ``spacing``) passes it and the distance chain is skipped; otherwise the map is computed from ``targets`` on the
    spot, on the device.  The loss can be negative; it is meant to be added to a regional loss (``CrossEntropyBoundaryLoss2d``)."""

    def __init__(self, classes=None, spacing=(1., 1.), ignore_index=255):
        super().__init__()
        self.classes = _class_list(classes, type(self).__name__)
        self.spacing = _spacing2(spacing, type(self).__name__)
        self.ignore_index = ignore_index

    def _phi(self, outputs, targets, dist_map):
        """The fp32 NHWC map [B, H, W, C] of this batch: ``dist_map`` (logical [B, C, H, W]) if given, else computed from ``targets``."""
        B, C, H, W = outputs.shape
        if dist_map is None:
            with torch.no_grad():
                return K.signed_distance(targets, C, self.classes, self.spacing)
        assert tuple(dist_map.shape) == (B, C, H, W), (dist_map.shape, outputs.shape)
        phi = _pc(dist_map.detach())
        return phi.clone() if phi.data_ptr() % 16 else phi

    def forward(self, outputs, targets, dist_map=None):
        assert outputs.dim() == 4 and targets.dim() == 3, (outputs.shape, targets.shape)
        mask = _class_mask(self.classes, outputs.shape[1], type(self).__name__)
        if not outputs.is_cuda:
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        return _BoundaryFn.apply(outputs, targets, self._phi(outputs, targets, dist_map), mask, self.ignore_index)


class CrossEntropyBoundaryLoss2d(_ClassWeighted):
    """``ce_coef`` * class-weighted mean cross entropy (``CrossEntropyLoss2d(weight)``) + ``boundary_coef`` * ``BoundaryLoss(classes,
    spacing)``, composed of the two criteria's own kernels.  A coefficient of exactly 0 removes its term (a NaN cross entropy then does
    not reach the total).  ``boundary_coef`` is a plain attribute read at every call: the paper's rebalancing schedule is the user
    raising it per epoch.  After a call ``last_terms`` holds the two device scalars (ce, boundary), None for a removed term; nothing
    synchronises."""

    def __init__(self, weight=None, ce_coef=1.0, boundary_coef=0.01, classes=None, spacing=(1., 1.), ignore_index=255):
        super().__init__()
        self._set_weight(weight)
        self.ce_coef, self.boundary_coef = float(ce_coef), float(boundary_coef)
        self.boundary = BoundaryLoss(classes, spacing, ignore_index)
        self.ignore_index = ignore_index
        self.last_terms = None

    classes = property(lambda self: self.boundary.classes)
    spacing = property(lambda self: self.boundary.spacing)

    def forward(self, outputs, targets, dist_map=None):
        assert outputs.dim() == 4 and targets.dim() == 3, (outputs.shape, targets.shape)
        _class_mask(self.boundary.classes, outputs.shape[1], type(self).__name__)
        if self.ce_coef == 0.0 and self.boundary_coef == 0.0:
            raise ValueError(f"dct_amd {type(self).__name__}: ce_coef and boundary_coef are both 0")
        if not outputs.is_cuda:
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        w = self.device_weight(outputs.device, outputs.shape[1])
        ce = bd = None
        if self.ce_coef != 0.0:
            ce = _ce_reduced(outputs, targets, w, K.CE_MEAN, self.ignore_index)
        if self.boundary_coef != 0.0:
            bd = self.boundary(outputs, targets, dist_map)
        self.last_terms = (None if ce is None else ce.detach(), None if bd is None else bd.detach())
        if bd is None:
            return ce if self.ce_coef == 1.0 else self.ce_coef * ce
        if ce is None:
            return self.boundary_coef * bd
        return self.ce_coef * ce + self.boundary_coef * bd


class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        lp = _pc(logits)
        probs = K.softmax_fwd(lp, lp.shape[3])
        ctx.save_for_backward(probs)
        return _nchw(probs)

    @staticmethod
    def backward(ctx, g):
        (probs,) = ctx.saved_tensors
        return _nchw(K.softmax_bwd(probs, _pc(g), probs.shape[3]))


def softmax_channels(logits: torch.Tensor) -> torch.Tensor:
    """F.softmax(logits, 1) of models/segmentators.py:50 on the HIP kernel."""
    return _SoftmaxFn.apply(logits)


class _EntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, probs):
        pp = _pc(probs)
        ctx.save_for_backward(pp)
        return K.entropy_fwd(pp, pp.shape[3]).view(pp.shape[:3])

    @staticmethod
    def backward(ctx, g):
        (pp,) = ctx.saved_tensors
        return _nchw(K.entropy_bwd(pp, g.to(torch.float32).contiguous().view(-1), pp.shape[3]))


class Entropy_2D(nn.Module):
    def forward(self, input: torch.Tensor):
        assert input.shape.__len__() == 4
        if DEBUG_ASSERTS:
            assert _simplex(input)
        return _EntropyFn.apply(input)


class _KLMapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, y, eps):
        pp, yp = _pc(p), _pc(y)
        ctx.save_for_backward(pp, yp)
        ctx.eps = eps
        return K.kl_map_fwd(pp, yp, pp.shape[3], eps).view(pp.shape[:3])

    @staticmethod
    def backward(ctx, g):
        pp, yp = ctx.saved_tensors
        dp = K.kl_map_bwd(pp, yp, g.to(torch.float32).contiguous().view(-1), pp.shape[3], ctx.eps)
        return _nchw(dp), None, None


class KL_Divergence_2D(nn.Module):
    """sum_c y*(log(y+eps) - log(p+eps)); the target ``y_prob`` is a constant on the co-training
    path (cotraining_totalloss.py:392 passes ``real_preds.detach()``), so only ``p_prob`` gets a gradient."""

    def __init__(self, reduce=False, eps=1e-10):
        super().__init__()
        self.reduce = reduce
        self.eps = eps

    def forward(self, p_prob: torch.Tensor, y_prob: torch.Tensor):
        if y_prob.requires_grad:
            raise NotImplementedError("dct_amd KL_Divergence_2D: pass y_prob.detach() (as the co-training step does)")
        if DEBUG_ASSERTS:
            assert _simplex(p_prob, 1) and _simplex(y_prob, 1)
        kl = _KLMapFn.apply(p_prob, y_prob, self.eps)
        return kl.mean() if self.reduce else kl


class _JSDMapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *probs):
        pps = [_pc(p) for p in probs]
        ctx.save_for_backward(*pps)
        return K.jsd_map_fwd(pps, pps[0].shape[3]).view(pps[0].shape[:3])

    @staticmethod
    def backward(ctx, g):
        pps = list(ctx.saved_tensors)
        dps = K.jsd_map_bwd(pps, g.to(torch.float32).contiguous().view(-1), pps[0].shape[3])
        return tuple(_nchw(d) for d in dps)


MAX_VIEWS = 8     # csrc/loss.hip MAXS


class JSD_2D(nn.Module):
    """H(mean_i p_i) - mean_i H(p_i) -> [B,H,W]; up to 8 views per call (the reference's sweeps run 2, 4 and 6:
    script/GM/run_multiview.sh:2-6, script/ACDC/5_run_multiple_view.sh:27-33)."""

    def __init__(self):
        super().__init__()
        self.entropy = Entropy_2D()

    def forward(self, input: List[torch.Tensor]):
        assert 1 <= len(input) <= MAX_VIEWS, f"dct_amd JSD_2D handles up to {MAX_VIEWS} models per call"
        if DEBUG_ASSERTS:
            for inprob in input:
                assert _simplex(inprob, 1)
        return _JSDMapFn.apply(*input)


class _ConsMapFn(torch.autograd.Function):
    """A view-consistency map on dct_{pl,spl,mse}_map_*; ``family``: the criterion's ``family``, ``rule``: its ``launch_args()``.  Returns
    the [B,H,W] map and, without a gradient, the per-pixel kept map.  Nothing but the inputs is saved: the backward recomputes the teachers."""

    @staticmethod
    def forward(ctx, family, rule, *probs):
        pps = [_pc(p) for p in probs]
        ctx.save_for_backward(*pps)
        ctx.family, ctx.rule = family, rule
        out, kept = getattr(K, family + "_map_fwd")(pps, pps[0].shape[3], **rule)
        kept = kept.view(pps[0].shape[:3])
        ctx.mark_non_differentiable(kept)
        return out.view(pps[0].shape[:3]), kept

    @staticmethod
    def backward(ctx, g, _):
        pps = list(ctx.saved_tensors)
        dps = getattr(K, ctx.family + "_map_bwd")(pps, g.to(torch.float32).contiguous().view(-1), pps[0].shape[3], **ctx.rule)
        return (None, None) + tuple(_nchw(d) for d in dps)


class _ViewConsistency_2D(nn.Module):
    """What the view-consistency criteria share: a list of [B,C,H,W] probabilities in, a [B,H,W] map out, whose mean over ALL pixels is the
    loss; a teacher mode, a confidence threshold and (the logarithmic ones) eps; ``last_kept``.  A criterion names its ``family`` (the
    prefix of its hip_ops functions) and its ``launch_args()``.  The public criteria are unrelated to each other beyond this base: the
    trainer tells them apart by exact type."""
    family = None

    def __init__(self, teacher):
        super().__init__()
        if teacher not in K.PL_TEACHERS:
            raise ValueError(f"dct_amd {type(self).__name__}: teacher must be 'cross' or 'ensemble', got {teacher!r}")
        self.teacher = teacher
        self.last_kept = None

    def _check_threshold(self, threshold):
        if not (0.0 <= self.threshold <= float('inf')):
            raise ValueError(f"dct_amd {type(self).__name__}: threshold must be >= 0, got {threshold}")

    def _check_eps(self, eps):
        # (eps is handed to the kernels as fp32: one that rounds to 0 there would put log(0) back)
        if not (0.0 < self.eps < float('inf')) or float(torch.tensor(self.eps, dtype=torch.float32)) == 0.0:
            raise ValueError(f"dct_amd {type(self).__name__}: eps must be finite and > 0 in fp32, got {eps}")

    def min_views(self):
        return 2 if self.teacher == 'cross' else 1

    def forward(self, input: List[torch.Tensor]):
        input = list(input)
        name = type(self).__name__
        if len(input) < self.min_views():
            raise ValueError(f"dct_amd {name}: teacher='{self.teacher}' needs at least {self.min_views()} views, got {len(input)}")
        if len(input) > MAX_VIEWS:
            raise ValueError(f"dct_amd {name} handles up to {MAX_VIEWS} views per call, got {len(input)}")
        if not all(p.is_cuda for p in input):
            raise RuntimeError("dct_amd losses run on the HIP device only (no CPU fallback)")
        if DEBUG_ASSERTS:
            for inprob in input:
                assert _simplex(inprob, 1)
        out, kept = _ConsMapFn.apply(self.family, self.launch_args(), *input)
        self.last_kept = kept.mean()
        return out


class PseudoLabel_2D(_ViewConsistency_2D):
    """Hard pseudo-label consistency of S views (the rule: include/dct.h, dct_pl_*), with ``JSD_2D``'s call shape: a list of [B,C,H,W]
    probabilities in, a [B,H,W] map out, whose mean over ALL pixels is the loss.  ``teacher='cross'``: cross pseudo supervision, every
    view learns the argmax of every other view (2 or more views); ``teacher='ensemble'``: every view learns the argmax of the summed
    probabilities.  ``threshold``: a teacher whose confidence (its maximum probability; for the ensemble the mean of the views') is below
    it is masked out; 0 keeps every teacher.  Teachers are constants: no gradient flows through argmax, confidence or mask.  After a
    call ``last_kept`` is a device scalar, the kept fraction of the teacher terms (nothing synchronises)."""
    family = 'pl'

    def __init__(self, teacher='cross', threshold=0.0, eps=1e-10):
        super().__init__(teacher)
        try:
            self.threshold, self.eps = float(threshold), float(eps)
        except (TypeError, ValueError):
            raise ValueError(f"dct_amd {type(self).__name__}: threshold and eps must be numbers, got {threshold!r}, {eps!r}")
        self._check_threshold(threshold)
        self._check_eps(eps)

    def launch_args(self):
        """The keyword arguments of hip_ops.pl_* (and what a captured step is valid for)."""
        return dict(teacher=K.PL_TEACHERS[self.teacher], tau=self.threshold, eps=self.eps)


class CrossPseudoSupervision_2D(PseudoLabel_2D):
    """Cross pseudo supervision (Chen et al., CVPR 2021): ``PseudoLabel_2D(teacher='cross')``."""

    def __init__(self, threshold=0.0, eps=1e-10):
        super().__init__('cross', threshold, eps)


class EnsemblePseudoLabel_2D(PseudoLabel_2D):
    """The voted pseudo-label with a confidence threshold: ``PseudoLabel_2D(teacher='ensemble')``."""

    def __init__(self, threshold=0.0, eps=1e-10):
        super().__init__('ensemble', threshold, eps)


class SoftPseudoLabel_2D(_ViewConsistency_2D):
    """Soft pseudo-label consistency of S views (the rule: include/dct.h, dct_spl_*), with ``PseudoLabel_2D``'s call shape: a list of
    [B,C,H,W] probabilities in, a [B,H,W] map out, whose mean over ALL pixels is the loss.  The teacher is the other views' prediction
    (``teacher='cross'``, 2 or more views) or the summed prediction (``teacher='ensemble'``), sharpened with ``temperature`` T as
    MixMatch's Sharpen(q, T) = q^(1/T) / sum q^(1/T): T = 1 is plain cross entropy against the teacher's probabilities, T -> 0 the hard
    pseudo-label.  ``threshold`` masks a teacher by its raw confidence, before sharpening.  Teachers are constants.  After a call
    ``last_kept`` is a device scalar, the kept fraction of the teacher terms (nothing synchronises).
    Not a ``PseudoLabel_2D``: the trainer tells the criteria apart by exact type."""
    family = 'spl'

    def __init__(self, teacher='cross', temperature=0.5, threshold=0.0, eps=1e-10):
        super().__init__(teacher)
        name = type(self).__name__
        try:
            self.temperature, self.threshold, self.eps = float(temperature), float(threshold), float(eps)
        except (TypeError, ValueError):
            raise ValueError(f"dct_amd {name}: temperature, threshold and eps must be numbers, got {temperature!r}, {threshold!r}, {eps!r}")
        # (the kernels receive T as fp32 and form r = 1.f / T there: both must be finite and > 0)
        t32 = torch.tensor(self.temperature, dtype=torch.float32)
        r32 = 1.0 / t32
        if not (0.0 < float(t32) < float('inf')) or not (0.0 < float(r32) < float('inf')):
            raise ValueError(f"dct_amd {name}: temperature and 1 / temperature must be finite and > 0 in fp32, got {temperature}")
        self._check_threshold(threshold)
        self._check_eps(eps)

    def launch_args(self):
        """The keyword arguments of hip_ops.spl_* (and what a captured step is valid for)."""
        return dict(teacher=K.PL_TEACHERS[self.teacher], tau=self.threshold, temperature=self.temperature, eps=self.eps)


class SoftCrossPseudoSupervision_2D(SoftPseudoLabel_2D):
    """Soft cross pseudo supervision: ``SoftPseudoLabel_2D(teacher='cross')``."""

    def __init__(self, temperature=0.5, threshold=0.0, eps=1e-10):
        super().__init__('cross', temperature, threshold, eps)


class SoftEnsemblePseudoLabel_2D(SoftPseudoLabel_2D):
    """The sharpened mean prediction as everyone's target (one network: self-training on its own sharpened prediction):
    ``SoftPseudoLabel_2D(teacher='ensemble')``."""

    def __init__(self, temperature=0.5, threshold=0.0, eps=1e-10):
        super().__init__('ensemble', temperature, threshold, eps)


class MSEConsistency_2D(_ViewConsistency_2D):
    """Softmax-MSE consistency of S views (the rule: include/dct.h, dct_mse_*), with ``PseudoLabel_2D``'s call shape: a list of [B,C,H,W]
    probabilities in, a [B,H,W] map out, whose mean over ALL pixels is the loss.  Every view is pulled towards every other view's
    prediction (``teacher='cross'``, 2 or more views) or towards the mean prediction (``teacher='ensemble'``) by the squared distance,
    averaged over the classes: bounded by 2 / C per pixel, no eps, no logarithm.  ``threshold`` masks a teacher by its confidence, as for
    the pseudo-label criteria; 0 keeps every teacher.  Teachers are constants.  After a call ``last_kept`` is a device scalar, the kept
    fraction of the teacher terms (nothing synchronises).
    Not a ``PseudoLabel_2D``: the trainer tells the criteria apart by exact type."""
    family = 'mse'

    def __init__(self, teacher='cross', threshold=0.0):
        super().__init__(teacher)
        try:
            self.threshold = float(threshold)
        except (TypeError, ValueError):
            raise ValueError(f"dct_amd {type(self).__name__}: threshold must be a number, got {threshold!r}")
        self._check_threshold(threshold)

    def launch_args(self):
        """The keyword arguments of hip_ops.mse_* (and what a captured step is valid for)."""
        return dict(teacher=K.PL_TEACHERS[self.teacher], tau=self.threshold)


class CrossMSE_2D(MSEConsistency_2D):
    """The squared distance to every other view's prediction: ``MSEConsistency_2D(teacher='cross')``."""

    def __init__(self, threshold=0.0):
        super().__init__('cross', threshold)


class EnsembleMSE_2D(MSEConsistency_2D):
    """The squared distance to the mean prediction (temporal-ensembling style, the mean held constant):
    ``MSEConsistency_2D(teacher='ensemble')``."""

    def __init__(self, threshold=0.0):
        super().__init__('ensemble', threshold)
