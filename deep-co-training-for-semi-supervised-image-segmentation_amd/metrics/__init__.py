"""Meters used inside the step (reference: generalframework/metrics/dice_meter.py:12-83,
averagemeter.py:3-48), kept on the device: ``add`` launches one counting kernel and never
synchronises; ``value`` is where the (tiny) results are read.  ``HausdorffMeter`` is the second column of the reference's
result tables (Summary.py:70-252), which takes it from an external package: here ``dct_hausdorff`` (include/dct.h).
``AgreementMeter`` is the third: Cohen's kappa between every pair of raters (the models, an ensemble, gt), and the IoU of the
reference's ``IoU`` / ``ConfusionMatrix`` meters, from the pairwise confusion matrices of ``dct_confusion_counts``.
``keep_largest_component`` is the cleaning ACDC-style pipelines apply in front of all of them (``dct_largest_component``), and
``ComponentMeter`` reports what it removed.  ``CalibrationMeter`` is the first that uses the values of the probabilities and not only
their argmax: ECE, MCE, Brier score, NLL, the reliability diagram and the coverage-accuracy curve of every view and of their mean,
from the integer tables of ``dct_calibration_counts``.  ``TemperatureScaler`` is the remedy: one temperature per view and one for their
mean, fitted by ``solve_temperature`` on the integer sums of ``dct_temperature_sums``, applied by ``dct_temperature_apply``."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import hip_ops as K

__all__ = ["DiceMeter", "HausdorffMeter", "AgreementMeter", "ComponentMeter", "AverageValueMeter", "keep_largest_component", "pair_index",
           "kappa_of", "iou_of", "CalibrationMeter", "ece_of", "mce_of", "TemperatureScaler", "solve_temperature"]


class DiceMeter(object):
    def __init__(self, method='2d', report_axises='all', C=4) -> None:
        assert method in ('2d', '3d')
        assert report_axises == 'all' or isinstance(report_axises, list)
        self.method = method
        self.report_axis = report_axises
        self.diceLog = []
        self.C = C
        self._acc = None        # float64 [2, C + 1] on the device: running sum / sum of squares per class and of the report mean
        self._n = 0
        self._cache = None

    def reset(self):
        self.diceLog = []
        self._acc = None
        self._n = 0
        self._cache = None

    def add(self, pred_logit: torch.Tensor, gt: torch.Tensor, smooth: float = 1e-8):
        """pred_logit [B,C,H,W] (logits or probabilities: only the argmax matters, dice_meter.py:28-32),
        gt [B,1,H,W] int64."""
        if not pred_logit.is_cuda:
            raise RuntimeError("dct_amd DiceMeter counts on the HIP device only (no CPU fallback)")
        B, C = pred_logit.shape[0], pred_logit.shape[1]
        lp = pred_logit.detach().permute(0, 2, 3, 1)
        if lp.dtype != torch.float32 or not lp.is_contiguous():
            lp = lp.to(torch.float32).contiguous()
        g = gt.reshape(B, -1)
        if g.dtype != torch.int64 or not g.is_contiguous():
            g = g.to(torch.int64).contiguous()
        inter, ps, gs = K.dice_counts(lp, g, B, C)
        # the Dice rows and the running moments behind value() in one more launch: three launches per add, nothing that scales
        # with the history (the reference re-concatenates the whole log 4 S times per reported step, :251-264)
        if self._acc is None or self._acc.device != inter.device:
            self._acc = torch.zeros(2, C + 1, dtype=torch.float64, device=inter.device)
        axes = range(C) if self.report_axis == 'all' else self.report_axis
        mask = sum(1 << int(a) for a in axes)
        if B <= 64:
            dice = K.dice_update(inter, ps, gs, self.method == '3d', mask, smooth, self._acc)
        else:       # patient batches of more than 64 slices: the same arithmetic in torch ops
            if self.method == '3d':
                inter, ps, gs = inter.sum(0, keepdim=True), ps.sum(0, keepdim=True), gs.sum(0, keepdim=True)
            dice = (2 * inter.float() + smooth) / ((ps + gs).float() + smooth)
            rep = dice[:, list(axes)].mean(1, keepdim=True)
            row = torch.cat((dice, rep), dim=1).double()
            self._acc += torch.stack((row.sum(0), (row * row).sum(0)))
        self.diceLog.append(dice)
        self._n += dice.shape[0]

    @property
    def log(self):
        if self.diceLog:
            log = torch.cat(self.diceLog)
        else:
            log = torch.zeros(1, self.C)
        return log

    def value(self, **kwargs):
        if self._acc is None:               # nothing added yet: the reference reports over one row of zeros
            log = self.log
            report_means = log.mean(1) if self.report_axis == 'all' else log[:, self.report_axis].mean(1)
            return (report_means.mean(), report_means.std()), (log.mean(0), log.std(0))
        # ONE device->host copy of the 2 x (C + 1) running sums per reading (cached until the next add): the per-class floats
        # the progress bar then takes (4 S readings of C values each, cotraining_totalloss.py:251-264) cost no further
        # synchronisation -- a blocking read of a device scalar is ~ms on this stack, the arithmetic below is nothing
        if self._cache is None or self._cache[0] != self._n:
            acc = self._acc.cpu()
            n = self._n
            mean = acc[0] / n
            var = (acc[1] - n * mean * mean).clamp_min(0.0) / (n - 1) if n > 1 else torch.full_like(mean, float('nan'))
            mean, std = mean.float(), var.sqrt().float()
            self._cache = (n, ((mean[-1], std[-1]), (mean[:-1], std[:-1])))
        return self._cache[1]

    def detailed_summary(self) -> dict:
        _, (means, _) = self.value()
        return {f'DSC{i}': means[i].item() for i in range(len(means))}

    def summary(self) -> dict:
        (means, var), (_, _) = self.value()
        return {'mDSC': means.item(), 'mVars': var.item()}


class HausdorffMeter(object):
    """Hausdorff distance per class between the argmax of the prediction and gt (``dct_hausdorff``: medpy's ``hd`` rule),
    '2d' = one row per slice, '3d' = one row for the batch taken as a volume; ``spacing`` = (sz, sy, sx).  A class that is
    absent from the prediction or from gt has no distance: its entry is NaN in ``log``, is left out of every statistic and is
    not counted in ``defined``.  Same layout as ``DiceMeter``."""

    def __init__(self, method='2d', report_axises='all', C=4, spacing=(1., 1., 1.)) -> None:
        assert method in ('2d', '3d')
        assert report_axises == 'all' or isinstance(report_axises, list)
        assert len(spacing) == 3 and all(float(s) > 0 for s in spacing), spacing
        self.method = method
        self.report_axis = report_axises
        self.C = C
        self.spacing = tuple(float(s) for s in spacing)
        self.reset()

    def reset(self):
        self.hdLog = []
        self._cache = None

    def add(self, pred_logit: torch.Tensor, gt: torch.Tensor):
        """pred_logit [B,C,H,W] (logits or probabilities: only the argmax matters), gt [B,1,H,W] integer."""
        if not pred_logit.is_cuda or not gt.is_cuda:
            raise RuntimeError("dct_amd HausdorffMeter measures on the HIP device only (no CPU fallback)")
        B, H, W = pred_logit.shape[0], pred_logit.shape[2], pred_logit.shape[3]
        lp = pred_logit.detach().permute(0, 2, 3, 1)
        if lp.dtype != torch.float32 or not lp.is_contiguous():
            lp = lp.to(torch.float32).contiguous()
        g = gt.reshape(B, H, W)
        if g.dtype != torch.int64 or not g.is_contiguous():
            g = g.to(torch.int64).contiguous()
        hd2 = K.hausdorff(lp, g, self.method == '3d', self.spacing)
        self.hdLog.append(hd2.sqrt())           # NaN stays NaN; nothing here waits for the device
        self._cache = None

    @property
    def log(self):
        if self.hdLog:
            return torch.cat(self.hdLog)
        return torch.full((1, self.C), float('nan'))

    def _stats(self):
        # ONE device->host copy of the log per reading (cached until the next add); the NaN-aware moments are host arithmetic on
        # rows x C numbers
        if self._cache is None:
            log = self.log.cpu().double()
            axes = list(range(log.shape[1])) if self.report_axis == 'all' else list(self.report_axis)

            def moments(v):         # over the defined entries of each column of v [n, k]
                ok = ~torch.isnan(v)
                n = ok.sum(0)
                z = torch.where(ok, v, torch.zeros_like(v))
                nan = torch.full((v.shape[1],), float('nan'), dtype=v.dtype)
                mean = torch.where(n > 0, z.sum(0) / n.clamp_min(1), nan)
                dev = torch.where(ok, v - mean, torch.zeros_like(v))
                std = torch.where(n > 1, ((dev * dev).sum(0) / (n - 1).clamp_min(1)).sqrt(), nan)
                return mean.float(), std.float(), n

            mean, std, n = moments(log)
            rep, _, _ = moments(log[:, axes].t().contiguous())      # a row's report value: the mean over its defined report axes
            rmean, rstd, _ = moments(rep.double().unsqueeze(1))
            self._cache = ((rmean[0], rstd[0]), (mean, std), n)
        return self._cache

    @property
    def defined(self):
        """Number of defined (non-NaN) entries per class."""
        return self._stats()[2]

    def value(self, **kwargs):
        s = self._stats()
        return s[0], s[1]

    def detailed_summary(self) -> dict:
        _, (means, _) = self.value()
        return {f'HD{i}': means[i].item() for i in range(len(means))}

    def summary(self) -> dict:
        (means, var), (_, _) = self.value()
        return {'mHD': means.item(), 'mVars': var.item()}


def pair_index(i: int, j: int, R: int) -> int:
    """Index of the pair (i, j), i < j, of R raters in lexicographic order (include/dct.h, ``dct_confusion_counts``)."""
    assert 0 <= i < j < R, (i, j, R)
    return i * (2 * R - i - 1) // 2 + (j - i - 1)


def kappa_of(M, cols=None):
    """Cohen's kappa (unweighted) of confusion matrices M [..., C, C] in float64: (po - pe) / (1 - pe), po = tr M / n,
    pe = sum_k row_k col_k / n^2; NaN where n = 0 or pe = 1.  ``cols``: keep only these columns (the pixels whose second
    rater lies in this class set -- the reference's ``considered_classes`` on the target)."""
    M = np.asarray(M, dtype=np.float64)
    if cols is not None:
        keep = np.zeros(M.shape[-1])
        keep[list(cols)] = 1.0
        M = M * keep
    n = M.sum((-2, -1))
    with np.errstate(divide='ignore', invalid='ignore'):
        po = np.trace(M, axis1=-2, axis2=-1) / n
        pe = (M.sum(-1) * M.sum(-2)).sum(-1) / (n * n)
        k = (po - pe) / (1.0 - pe)
    return np.where((n == 0) | (pe == 1.0), np.nan, k)


def iou_of(M):
    """IoU per class of confusion matrices M [..., C, C] in float64: M[c][c] / (row_c + col_c - M[c][c]), NaN where that is 0."""
    M = np.asarray(M, dtype=np.float64)
    d = np.diagonal(M, axis1=-2, axis2=-1)
    den = M.sum(-1) + M.sum(-2) - d
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den == 0, np.nan, d / den)


def _nan_moments(v):
    """mean, sample std and count over the defined (non-NaN) entries along axis 0 of v [n, ...]; NaN where there are too few."""
    ok = ~np.isnan(v)
    n = ok.sum(0)
    z = np.where(ok, v, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where(n > 0, z.sum(0) / np.maximum(n, 1), np.nan)
        dev = np.where(ok, v - mean, 0.0)
        std = np.where(n > 1, np.sqrt((dev * dev).sum(0) / np.maximum(n - 1, 1)), np.nan)
    return mean, std, n


class AgreementMeter(object):
    """Agreement between ``n_models`` predictions (and gt, the last rater, ``with_gt``) from the confusion matrix of every pair
    of raters (``dct_confusion_counts``, one launch per ``add``): '2d' = one row per slice, '3d' = one row for the batch.
    ``kappa`` is Cohen's kappa per pair, restricted to the pixels whose second rater lies in ``considered_classes`` when that is
    set; ``iou`` the IoU per model and class against gt.  A kappa or IoU that is undefined on a row (include/dct.h) is NaN, is
    left out of every statistic and is not counted in ``defined``.  ``rater_names`` renames the predictions (default ``S{i}``)."""

    def __init__(self, method='2d', C=4, n_models=2, with_gt=True, considered_classes=None, rater_names=None) -> None:
        assert method in ('2d', '3d')
        assert 1 <= n_models <= 8 and n_models + bool(with_gt) >= 2, (n_models, with_gt)
        assert 1 <= C <= 8, C
        assert considered_classes is None or all(0 <= int(c) < C for c in considered_classes), considered_classes
        self.method = method
        self.C = C
        self.n_models = n_models
        self.with_gt = bool(with_gt)
        self.considered_classes = None if considered_classes is None else [int(c) for c in considered_classes]
        names = list(rater_names) if rater_names is not None else [f"S{i}" for i in range(n_models)]
        assert len(names) == n_models, names
        self.raters = names + (["gt"] if self.with_gt else [])
        R = len(self.raters)
        self.pairs = [f"{self.raters[i]}_{self.raters[j]}" for i in range(R) for j in range(i + 1, R)]
        self._gt_pairs = [pair_index(i, R - 1, R) for i in range(n_models)] if self.with_gt else []
        self.reset()

    def reset(self):
        self.countLog = []
        self._cache = None

    def add(self, preds, gt=None):
        """preds: ``n_models`` tensors [B,C,H,W] (logits or probabilities: only the argmax matters), gt [B,1,H,W] integer (None
        without ``with_gt``)."""
        if not isinstance(preds, (list, tuple)) or len(preds) != self.n_models:
            raise RuntimeError(f"dct_amd AgreementMeter was built for a list of {self.n_models} predictions")
        if self.with_gt != (gt is not None):
            raise RuntimeError("dct_amd AgreementMeter: gt is " + ("required" if self.with_gt else "not expected (with_gt=False)"))
        if any(not p.is_cuda for p in preds) or (gt is not None and not gt.is_cuda):
            raise RuntimeError("dct_amd AgreementMeter counts on the HIP device only (no CPU fallback)")
        B = preds[0].shape[0]
        ls = [p.detach().permute(0, 2, 3, 1) for p in preds]
        g = gt.reshape(B, -1) if gt is not None else None
        cnt = K.confusion_counts(ls, g).to(torch.int64)      # (confusion_counts makes the dense fp32 / int64 copies it needs)
        if self.method == '3d':
            cnt = cnt.sum(0, keepdim=True)
        self.countLog.append(cnt)                               # nothing here waits for the device
        self._cache = None

    def _rows(self):
        # ONE device->host copy of the log per reading (cached until the next add); everything derived is float64 host
        # arithmetic on rows x P x C x C integers
        if self._cache is None:
            if self.countLog:
                rows = torch.cat(self.countLog).cpu().numpy()
            else:
                rows = np.zeros((0, len(self.pairs), self.C, self.C), dtype=np.int64)
            self._cache = {'rows': rows}
        return self._cache['rows']

    def confusion(self):
        """int64 [P, C, C]: the confusion matrix of every pair over everything added."""
        return torch.from_numpy(self._rows().sum(0))

    def _kappa_stats(self):
        rows = self._rows()
        if 'kappa' not in self._cache:
            k = kappa_of(rows, self.considered_classes)              # [rows, P]
            mean, std, n = _nan_moments(k)
            report = self._gt_pairs or list(range(len(self.pairs)))
            with np.errstate(invalid='ignore'):
                rep = _nan_moments(k[:, report].T)[0]                # a row's report value: the mean over its defined report pairs
            rmean, rstd, _ = _nan_moments(rep[:, None])
            self._cache['kappa'] = (mean, std, n, float(rmean[0]), float(rstd[0]))
        return self._cache['kappa']

    def kappa(self):
        """(mean [P], std [P], defined [P]) of the per-row kappa of every pair, in the order of ``pairs``."""
        mean, std, n, _, _ = self._kappa_stats()
        return torch.from_numpy(mean), torch.from_numpy(std), torch.from_numpy(n)

    def iou(self):
        """(mean [n_models, C], std [n_models, C]) of the per-row IoU of every model against gt."""
        if not self.with_gt:
            raise RuntimeError("dct_amd AgreementMeter.iou needs with_gt=True")
        rows = self._rows()
        if 'iou' not in self._cache:
            mean, std, _ = _nan_moments(iou_of(rows[:, self._gt_pairs]))
            self._cache['iou'] = (mean, std)
        mean, std = self._cache['iou']
        return torch.from_numpy(mean), torch.from_numpy(std)

    def value(self, **kwargs):
        mean, std, _, rmean, rstd = self._kappa_stats()
        return (rmean, rstd), (torch.from_numpy(mean), torch.from_numpy(std))

    def detailed_summary(self) -> dict:
        mean = self._kappa_stats()[0]
        return {name: float(mean[p]) for p, name in enumerate(self.pairs)}

    def summary(self) -> dict:
        """Mean (and std) over the rows of a row's mean kappa over the pairs that contain gt (all pairs without gt)."""
        (mean, std), _ = self.value()
        return {'mKappa': mean, 'mVars': std}


CONF_UNIT = float(1 << 24)      # the fixed-point unit of the confidence, Brier and NLL sums of dct_calibration_counts


def _gaps_of(bins):
    """bins [..., n_bins, 3] -> (n [..., n_bins], N [...], |acc_k - conf_k| [..., n_bins] with 0 in the empty bins) in float64."""
    b = np.asarray(bins, dtype=np.float64)
    assert b.ndim >= 2 and b.shape[-1] == 3, b.shape
    n = b[..., 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        gap = np.where(n > 0, np.abs(b[..., 1] / n - b[..., 2] / (CONF_UNIT * n)), 0.0)
    return n, n.sum(-1), gap


def ece_of(bins):
    """Expected calibration error of reliability tables bins [..., n_bins, 3] = {pixels, correct pixels, sum of conf * 2^24} per bin
    (``dct_calibration_counts``, include/dct.h) in float64: sum_k (n_k / N) |acc_k - conf_k|; NaN where N = 0."""
    n, N, gap = _gaps_of(bins)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(N > 0, (n * gap).sum(-1) / N, np.nan)


def mce_of(bins):
    """Maximum calibration error of reliability tables bins [..., n_bins, 3]: the largest |acc_k - conf_k| over the non-empty bins;
    NaN where there is none."""
    n, N, gap = _gaps_of(bins)
    return np.where(N > 0, gap.max(-1), np.nan)


class CalibrationMeter(object):
    """Calibration of ``n_models`` views and, ``with_ensemble``, of the mean of their probabilities (always the soft vote: a hard
    vote has no confidence), from the reliability tables of ``dct_calibration_counts`` (one launch per ``add``): '2d' = one row per
    slice, '3d' = one row for the batch.  Only the pixels whose gt lies in ``considered_classes`` count when that is set (on a
    segmentation slice ~90 % of the pixels are background that is confidently right, and every aggregate over them looks
    perfect).  ``from_logits``: ``add`` is given logits and the kernel takes their softmax.  A row without a counted pixel has
    no ECE, MCE, Brier score or NLL: NaN, left out of every statistic and not counted in ``defined``.  ``rater_names`` renames the
    views (default ``S{i}``); the mean of the views is ``ensemble``."""

    def __init__(self, method='2d', C=4, n_models=2, with_ensemble=True, n_bins=15, considered_classes=None, from_logits=False,
                 rater_names=None) -> None:
        assert method in ('2d', '3d')
        assert 1 <= n_models <= 8, n_models
        assert 1 <= C <= 8, C
        assert 1 <= int(n_bins) <= 32, n_bins
        assert considered_classes is None or all(0 <= int(c) < C for c in considered_classes), considered_classes
        self.method = method
        self.C = C
        self.n_models = n_models
        self.with_ensemble = bool(with_ensemble)
        self.n_bins = int(n_bins)
        self.considered_classes = None if considered_classes is None else [int(c) for c in considered_classes]
        self.from_logits = bool(from_logits)
        names = list(rater_names) if rater_names is not None else [f"S{i}" for i in range(n_models)]
        assert len(names) == n_models, names
        self.raters = names + (["ensemble"] if self.with_ensemble else [])
        self.reset()

    def reset(self):
        self.countLog = []
        self._cache = None

    def add(self, preds, gt):
        """preds: ``n_models`` tensors [B,C,H,W], probabilities (logits with ``from_logits``); gt [B,1,H,W] integer."""
        if not isinstance(preds, (list, tuple)) or len(preds) != self.n_models:
            raise RuntimeError(f"dct_amd CalibrationMeter was built for a list of {self.n_models} predictions")
        if gt is None:
            raise RuntimeError("dct_amd CalibrationMeter: gt is required")
        if any(not p.is_cuda for p in preds) or not gt.is_cuda:
            raise RuntimeError("dct_amd CalibrationMeter counts on the HIP device only (no CPU fallback)")
        B = preds[0].shape[0]
        ps = [p.detach().permute(0, 2, 3, 1) for p in preds]
        bins, scores = K.calibration_counts(ps, gt.reshape(B, -1), n_bins=self.n_bins, classes=self.considered_classes,
                                            with_ensemble=self.with_ensemble, from_logits=self.from_logits)
        row = torch.cat((bins.flatten(2), scores), dim=2)       # [B, R, n_bins * 3 + 2]: one log, one host copy per reading
        if self.method == '3d':
            row = row.sum(0, keepdim=True)
        self.countLog.append(row)                               # nothing here waits for the device
        self._cache = None

    def _rows(self):
        # ONE device->host copy of the log per reading (cached until the next add); everything derived is float64 host arithmetic
        # on rows x R x (n_bins x 3 + 2) integers
        if self._cache is None:
            R, nb = len(self.raters), self.n_bins
            if self.countLog:
                rows = torch.cat(self.countLog).cpu().numpy()
            else:
                rows = np.zeros((0, R, nb * 3 + 2), dtype=np.int64)
            self._cache = {'bins': rows[:, :, :nb * 3].reshape(-1, R, nb, 3), 'scores': rows[:, :, nb * 3:]}
        return self._cache['bins'], self._cache['scores']

    def _stats(self):
        bins, scores = self._rows()
        if 'stats' not in self._cache:
            N = bins[..., 0].sum(-1).astype(np.float64)                              # [rows, R]
            with np.errstate(divide='ignore', invalid='ignore'):
                per_row = {'ECE': ece_of(bins), 'MCE': mce_of(bins),
                           'Brier': np.where(N > 0, scores[..., 0] / (CONF_UNIT * N), np.nan),
                           'NLL': np.where(N > 0, scores[..., 1] / (CONF_UNIT * N), np.nan)}
                stats = {k: _nan_moments(v) for k, v in per_row.items()}
                rep = _nan_moments(per_row['ECE'].T)[0]          # a row's report value: the mean ECE over its raters
            rmean, rstd, _ = _nan_moments(rep[:, None])
            stats['report'] = (float(rmean[0]), float(rstd[0]))
            self._cache['stats'] = stats
        return self._cache['stats']

    def _triple(self, key):
        mean, std, n = self._stats()[key]
        return torch.from_numpy(mean), torch.from_numpy(std), torch.from_numpy(n)

    def ece(self):
        """(mean [R], std [R], defined [R]) of the per-row expected calibration error of every rater, in the order of ``raters``."""
        return self._triple('ECE')

    def mce(self):
        """(mean [R], std [R], defined [R]) of the per-row maximum calibration error."""
        return self._triple('MCE')

    def brier(self):
        """(mean [R], std [R], defined [R]) of the per-row Brier score (mean over the counted pixels of sum_c (p_c - [c == gt])^2)."""
        return self._triple('Brier')

    def nll(self):
        """(mean [R], std [R], defined [R]) of the per-row negative log-likelihood (mean of -log(p_gt + 1e-10))."""
        return self._triple('NLL')

    def tables(self):
        """int64 [R, n_bins, 3]: the reliability table of every rater over everything added."""
        return torch.from_numpy(self._rows()[0].sum(0))

    def reliability(self):
        """(count int64 [R, n_bins], accuracy [R, n_bins], confidence [R, n_bins]) over everything added; NaN in an empty bin."""
        t = self._rows()[0].sum(0)
        n = t[..., 0].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            acc = np.where(n > 0, t[..., 1] / n, np.nan)
            conf = np.where(n > 0, t[..., 2] / (CONF_UNIT * n), np.nan)
        return torch.from_numpy(t[..., 0].copy()), torch.from_numpy(acc), torch.from_numpy(conf)

    def coverage_accuracy(self):
        """(coverage [R, n_bins], kept_accuracy [R, n_bins]) over everything added: at a bin's lower edge k / n_bins, the share of
        the counted pixels whose confidence lies in the bins >= k and the accuracy of those pixels -- what a pseudo-label
        ``threshold=k / n_bins`` would keep, and how right it would be.  NaN where nothing is counted / kept."""
        t = self._rows()[0].sum(0).astype(np.float64)
        kept = t[..., 0][:, ::-1].cumsum(-1)[:, ::-1]
        right = t[..., 1][:, ::-1].cumsum(-1)[:, ::-1]
        N = t[..., 0].sum(-1, keepdims=True)
        with np.errstate(divide='ignore', invalid='ignore'):
            cov = np.where(N > 0, kept / N, np.nan)
            acc = np.where(kept > 0, right / kept, np.nan)
        return torch.from_numpy(cov), torch.from_numpy(acc)

    def value(self, **kwargs):
        s = self._stats()
        return s['report'], (torch.from_numpy(s['ECE'][0]), torch.from_numpy(s['ECE'][1]))

    def detailed_summary(self) -> dict:
        s = self._stats()
        return {name: {k: float(s[k][0][r]) for k in ('ECE', 'MCE', 'Brier', 'NLL')} for r, name in enumerate(self.raters)}

    def summary(self) -> dict:
        """Mean (and std) over the rows of a row's mean ECE over its raters."""
        (mean, std), _ = self.value()
        return {'mECE': mean, 'mVars': std}


TEMP_UNIT = float(1 << 20)     # the fixed-point unit of the NLL and gradient sums of dct_temperature_sums


def solve_temperature(sum_fn, R, n_candidates=16, rounds=4, log2_range=(-4., 4.)):
    """The inverse temperature beta = 1 / T of each of R raters that minimises the negative log-likelihood, from pooled sums alone:
    host float64, no torch device.  ``sum_fn(betas [R, K] float64)`` -> ``(sums [R, K, 2], N)``: per rater and candidate the integer
    sums {nll * 2^20, d nll / d beta * 2^20} of ``dct_temperature_sums`` (include/dct.h) pooled over the data, and the number of
    counted pixels.  The gradient sum g is non-decreasing in beta (the NLL is convex in it), so the fit is a root search, and it
    is fixed so that the result is deterministic: each round places ``n_candidates`` candidates evenly in log2 beta across each rater's
    bracket, endpoints included (first: ``log2_range``), and keeps the adjacent pair with g_k <= 0 < g_k+1; after ``rounds`` rounds g
    is interpolated linearly inside the bracket (with exact sums the bracket is then 8 / 15^4 = 1.6e-4 wide in log2 beta at the
    defaults).  g > 0 at the low end of the first bracket: ``at_bound`` 'low', beta = that end (T = 16); g <= 0 at its high end:
    'high', beta = that end (T = 1 / 16).  A last call with the candidates {1, beta} gives the mean NLL before and after.  N = 0: NaN
    everywhere, after one call.  ``sum_fn`` is called ``rounds + 1`` times.
    -> dict: beta, temperature, nll_before, nll_after [R] float64; at_bound: list of None / 'low' / 'high'; N; curve_temperature,
    curve_nll [R, K]: the first round's grid, the NLL(T) curve over the whole range."""
    K_ = int(n_candidates)
    assert R >= 1 and 2 <= K_ <= 16 and rounds >= 1 and log2_range[0] < log2_range[1], (R, n_candidates, rounds, log2_range)
    lo, hi = np.full(R, float(log2_range[0])), np.full(R, float(log2_range[1]))
    bound = [None] * R
    steps = np.arange(K_, dtype=np.float64) / (K_ - 1)
    nan = np.full(R, np.nan)
    fit = None
    for rnd in range(rounds):
        grid = lo[:, None] + (hi - lo)[:, None] * steps[None]
        grid[:, 0], grid[:, -1] = lo, hi                        # the ends are the bracket's own numbers: their sums repeat exactly
        sums, N = sum_fn(np.exp2(grid))
        sums, N = np.asarray(sums), int(N)
        assert sums.shape == (R, K_, 2), sums.shape
        if rnd == 0:
            with np.errstate(divide='ignore', invalid='ignore'):
                curve = (np.exp2(-grid), sums[..., 0].astype(np.float64) / (TEMP_UNIT * N) if N > 0 else np.full((R, K_), np.nan))
            if N == 0:
                return dict(beta=nan, temperature=nan.copy(), nll_before=nan.copy(), nll_after=nan.copy(), at_bound=bound, N=0,
                            curve_temperature=curve[0], curve_nll=curve[1])
        g = sums[..., 1].astype(np.float64)
        fit = np.empty(R)
        for r in range(R):
            if rnd == 0 and g[r, 0] > 0:
                bound[r] = 'low'
            elif rnd == 0 and g[r, -1] <= 0:
                bound[r] = 'high'
            if bound[r] is not None:
                fit[r] = lo[r] if bound[r] == 'low' else hi[r]
                continue
            k = next(k for k in range(K_ - 1) if g[r, k] <= 0 < g[r, k + 1])
            fit[r] = grid[r, k] + (grid[r, k + 1] - grid[r, k]) * (-g[r, k]) / (g[r, k + 1] - g[r, k])
            lo[r], hi[r] = grid[r, k], grid[r, k + 1]
    beta = np.exp2(fit)
    sums, N = sum_fn(np.stack([np.ones(R), beta], 1))
    nll = np.asarray(sums)[..., 0].astype(np.float64) / (TEMP_UNIT * int(N))
    return dict(beta=beta, temperature=1.0 / beta, nll_before=nll[:, 0], nll_after=nll[:, 1], at_bound=bound, N=int(N),
                curve_temperature=curve[0], curve_nll=curve[1])


class TemperatureScaler(object):
    """Temperature scaling of ``n_models`` views and, ``with_ensemble``, of the mean of their probabilities (scaled as
    log(p_ens + 1e-10): the ensemble is formed first, as ``CalibrationMeter``'s ensemble rater): one temperature per rater, fitted by
    ``solve_temperature`` on the integer sums of ``dct_temperature_sums`` over the pixels whose gt lies in ``considered_classes``
    (None: all).  Scaling never changes a hard prediction.  ``fit`` walks its batches ``rounds + 1`` times, one launch per batch and
    one device->host copy per walk; ``apply`` is one launch (``dct_temperature_apply``)."""

    def __init__(self, C=4, n_models=2, with_ensemble=True, considered_classes=None, rater_names=None, n_candidates=16, rounds=4) -> None:
        assert 1 <= n_models <= 8, n_models
        assert 1 <= C <= 8, C
        assert 2 <= int(n_candidates) <= 16 and int(rounds) >= 1, (n_candidates, rounds)
        assert considered_classes is None or all(0 <= int(c) < C for c in considered_classes), considered_classes
        self.C = C
        self.n_models = n_models
        self.with_ensemble = bool(with_ensemble)
        self.considered_classes = None if considered_classes is None else [int(c) for c in considered_classes]
        self.n_candidates, self.rounds = int(n_candidates), int(rounds)
        names = list(rater_names) if rater_names is not None else [f"S{i}" for i in range(n_models)]
        assert len(names) == n_models, names
        self.raters = names + (["ensemble"] if self.with_ensemble else [])
        self._fit = None

    def _check(self, logits):
        if not isinstance(logits, (list, tuple)) or len(logits) != self.n_models:
            raise RuntimeError(f"dct_amd TemperatureScaler was built for a list of {self.n_models} predictions")
        if any(not z.is_cuda for z in logits):
            raise RuntimeError("dct_amd TemperatureScaler counts on the HIP device only (no CPU fallback)")

    def _device_sums(self, batches, betas):
        R, K_ = betas.shape
        out, bt = None, None
        for logits, gt in batches:
            self._check(logits)
            if gt is None:
                raise RuntimeError("dct_amd TemperatureScaler: gt is required")
            if not gt.is_cuda:
                raise RuntimeError("dct_amd TemperatureScaler counts on the HIP device only (no CPU fallback)")
            if bt is None:
                bt = torch.from_numpy(betas.astype(np.float32)).to(logits[0].device)
            B = logits[0].shape[0]
            out = K.temperature_sums([z.detach().permute(0, 2, 3, 1) for z in logits], gt.reshape(B, -1), bt,
                                     classes=self.considered_classes, with_ensemble=self.with_ensemble, out=out)
        if out is None:
            return np.zeros((R, K_, 2), dtype=np.int64), 0
        row = torch.cat((out[0].flatten(), out[1].flatten())).cpu().numpy()      # ONE device->host copy per walk
        return row[:-1].reshape(R, K_, 2), int(row[-1])

    def fit(self, batches):
        """batches: a re-iterable of ``(list of n_models logits [B,C,H,W], gt [B,1,H,W])``, iterated ``rounds + 1`` times."""
        return self.fit_sums(lambda betas: self._device_sums(batches, betas))

    def fit_sums(self, sum_fn):
        """The fit from any ``sum_fn`` of ``solve_temperature`` (``fit`` hands it the device sums)."""
        self._fit = solve_temperature(sum_fn, len(self.raters), n_candidates=self.n_candidates, rounds=self.rounds)
        return self

    def set_temperature(self, temperatures):
        """Given temperatures, one per rater, instead of a fit (no NLL, no curve)."""
        t = np.asarray([float(x) for x in temperatures], dtype=np.float64)
        R = len(self.raters)
        if t.shape != (R,) or not (t > 0).all():
            raise ValueError(f"dct_amd TemperatureScaler: {R} positive temperatures expected, got {temperatures}")
        nan = np.full(R, np.nan)
        self._fit = dict(beta=1.0 / t, temperature=t, nll_before=nan, nll_after=nan.copy(), at_bound=[None] * R, N=0,
                         curve_temperature=np.zeros((R, 0)), curve_nll=np.zeros((R, 0)))
        return self

    def _get(self, key):
        if self._fit is None:
            raise RuntimeError("dct_amd TemperatureScaler: fit() or set_temperature() first")
        return self._fit[key]

    temperature = property(lambda self: torch.from_numpy(self._get('temperature').copy()))
    beta = property(lambda self: torch.from_numpy(self._get('beta').copy()))
    nll_before = property(lambda self: torch.from_numpy(self._get('nll_before').copy()))
    nll_after = property(lambda self: torch.from_numpy(self._get('nll_after').copy()))
    at_bound = property(lambda self: list(self._get('at_bound')))

    def curve(self):
        """(temperature [R, K], mean NLL [R, K]): the first round's grid, from T = 16 down to T = 1 / 16."""
        return torch.from_numpy(self._get('curve_temperature').copy()), torch.from_numpy(self._get('curve_nll').copy())

    def apply(self, logits):
        """logits: ``n_models`` tensors [B,C,H,W] -> one [B,C,H,W] probability tensor per rater (logical views of NHWC buffers)."""
        self._check(logits)
        outs = K.temperature_apply([z.detach().permute(0, 2, 3, 1) for z in logits], self._get('beta'), with_ensemble=self.with_ensemble)
        return [o.permute(0, 3, 1, 2) for o in outs]

    def detailed_summary(self) -> dict:
        t, before, after, bound = (self._get(k) for k in ('temperature', 'nll_before', 'nll_after', 'at_bound'))
        return {name: {'T': float(t[r]), 'NLL_before': float(before[r]), 'NLL_after': float(after[r]), 'at_bound': bound[r]}
                for r, name in enumerate(self.raters)}

    summary = detailed_summary


def keep_largest_component(pred: torch.Tensor, method='2d', classes=None, background=0, full_connectivity=False, return_stats=False):
    """pred [B,C,H,W] (logits or probabilities, any float dtype, any layout) -> the one-hot float32 map of its argmax with only the
    largest connected component of every class in ``classes`` kept (None: all but ``background``) and the rest of those classes moved
    to ``background`` (``dct_largest_component``, include/dct.h): per slice ('2d') or with the batch as a volume ('3d'); 4- / 6-
    connectivity, 8- / 26- with ``full_connectivity``.  The result is a logical [B,C,H,W] view of an NHWC buffer, so the meters'
    ``permute`` costs nothing.  ``return_stats``: also the int32 [rows, C, 3] tensor ``ComponentMeter.add`` takes."""
    assert method in ('2d', '3d')
    if not pred.is_cuda:
        raise RuntimeError("dct_amd keep_largest_component labels on the HIP device only (no CPU fallback)")
    lp = pred.detach().permute(0, 2, 3, 1)
    if lp.dtype != torch.float32 or not lp.is_contiguous():
        lp = lp.to(torch.float32).contiguous()
    onehot, _, stats = K.largest_component(lp, method == '3d', full_connectivity, classes, background)
    out = onehot.permute(0, 3, 1, 2)
    return (out, stats) if return_stats else out


class ComponentMeter(object):
    """What ``keep_largest_component`` found, from the stats rows of ``dct_largest_component`` ([rows, C, 3] = components, size of the
    largest, pixels per class before cleaning; '2d': a row per slice, '3d': a row per batch): per class the mean and std over the rows
    where the class is present of the number of components and of the removed share (pixels - largest) / pixels.  A class that is never
    present gives NaN.  ``add`` keeps the device tensor and waits for nothing; ``value`` makes one host copy."""

    def __init__(self, method='2d', C=4) -> None:
        assert method in ('2d', '3d')
        self.method = method
        self.C = C
        self.reset()

    def reset(self):
        self.statLog = []
        self._cache = None

    def add(self, stats: torch.Tensor):
        if stats.dim() != 3 or tuple(stats.shape[1:]) != (self.C, 3) or stats.is_floating_point():
            raise RuntimeError(f"dct_amd ComponentMeter takes integer stats [rows, {self.C}, 3], got {tuple(stats.shape)} {stats.dtype}")
        self.statLog.append(stats.detach())
        self._cache = None

    def value(self, **kwargs):
        """((mean components [C], std), (mean removed share [C], std)) as float64 tensors."""
        if self._cache is None:
            if self.statLog:
                rows = torch.cat(self.statLog).cpu().numpy().astype(np.float64)
            else:
                rows = np.zeros((0, self.C, 3))
            present = rows[:, :, 2] > 0
            with np.errstate(divide='ignore', invalid='ignore'):
                comps = np.where(present, rows[:, :, 0], np.nan)
                removed = np.where(present, (rows[:, :, 2] - rows[:, :, 1]) / rows[:, :, 2], np.nan)
            cm, cs, n = _nan_moments(comps)
            rm, rs, _ = _nan_moments(removed)
            self._cache = ((torch.from_numpy(cm), torch.from_numpy(cs)), (torch.from_numpy(rm), torch.from_numpy(rs)), torch.from_numpy(n))
        return self._cache[0], self._cache[1]

    @property
    def defined(self):
        """Number of rows in which each class is present."""
        self.value()
        return self._cache[2]

    def detailed_summary(self) -> dict:
        (cm, _), (rm, _) = self.value()
        d = {f'CC{j}': float(cm[j]) for j in range(self.C)}
        d.update({f'removed{j}': float(rm[j]) for j in range(self.C)})
        return d

    summary = detailed_summary


class AverageValueMeter(object):
    """Running mean/std of scalars.  Device scalars are kept as tensors and only read in value()."""

    def __init__(self, name='Average Meter'):
        self.name = name
        self.reset()

    def reset(self):
        self._vals = []

    def add(self, value, n=1):
        self._vals.append(value)

    def _floats(self):
        if self._vals and any(isinstance(v, torch.Tensor) for v in self._vals):
            ts = [v.detach().float().reshape(()) if isinstance(v, torch.Tensor) else torch.tensor(float(v)) for v in self._vals]
            dev = next(t.device for t in ts if t.is_cuda) if any(t.is_cuda for t in ts) else ts[0].device
            self._vals = torch.stack([t.to(dev) for t in ts]).cpu().tolist()
        return self._vals

    def value(self):
        v = self._floats()
        n = len(v)
        if n == 0:
            return math.nan, math.nan
        mean = sum(v) / n
        if n == 1:
            return mean, math.inf
        var = sum((x - mean) ** 2 for x in v) / (n - 1.0)
        return mean, math.sqrt(var)

    def summary(self) -> dict:
        return {'mean': self.value()[0], 'val': self.value()[1]}

    detailed_summary = summary
