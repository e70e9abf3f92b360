"""Checkpoint ensemble summary (reference: /root/reference/Summary.py:70-252, the SURVEY.md 8f "next" row 3).

``load_model`` / ``load_models`` rebuild ``Segmentator``s from ``best_{i}.pth`` checkpoints exactly as Summary.py:70-79 does;
``Ensembleway`` is the soft / hard voting of :92-126; ``summarize`` is the evaluation loop of :148-172 + the result tables of
:176-252: Dice and, on request, Hausdorff distance (2-D per slice and 3-D per patient batch, per model and for the ensemble),
Cohen's kappa between every pair of raters (the models, the ensemble vote, gt) and IoU.
The reference takes the Hausdorff distance from the external ``deepclustering`` package, absent from its tree; here it is
medpy's ``metric.binary.hd`` rule as include/dct.h states it (``dct_hausdorff``).  It takes kappa from scikit-learn's
``cohen_kappa_score``; here it is that rule as include/dct.h states it, float64 host arithmetic on the pairwise confusion
matrices that ``dct_confusion_counts`` leaves.

Predictions come from the HIP networks; voting, the Dice counting (``dct_dice_counts``), the distance transform behind the
Hausdorff distance (``dct_hausdorff``), the confusion matrices behind kappa and IoU (``dct_confusion_counts``) and, on request,
the largest-connected-component cleaning of every prediction in front of a second set of tables (``dct_largest_component``) and
the fit of a temperature per model and for their mean (``dct_temperature_sums``) run on the device."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
from torch import Tensor

from .metrics import AgreementMeter, CalibrationMeter, ComponentMeter, DiceMeter, HausdorffMeter, TemperatureScaler, keep_largest_component
from .models import Segmentator


def load_model(checkpoint, map_location="cpu") -> Segmentator:
    """Summary.py:70-74 (+ :140-146: the weights are loaded too)."""
    state = torch.load(checkpoint, map_location=torch.device(map_location), weights_only=False)
    sd = state['segmentator']
    model = Segmentator(arch_dict=sd['arch_dict'], optim_dict=sd['optim_dict'], scheduler_dict=sd['scheduler_dict'])
    model.load_state_dict(sd)
    return model


def load_models(checkpoints) -> List[Segmentator]:
    return [load_model(c) for c in checkpoints]


class Ensembleway(object):
    def __init__(self, ensembleway: str, num_classes: Optional[int] = None) -> None:
        assert ensembleway in ('soft', 'hard'), ensembleway
        self.ensembleway = ensembleway
        self.num_classes = num_classes

    def __call__(self, predicts: List[Tensor]) -> Tensor:
        return self._softVoting(predicts) if self.ensembleway == 'soft' else self._hardVoting(predicts, self.num_classes)

    @staticmethod
    def _softVoting(predicts: List[Tensor]) -> Tensor:
        assert isinstance(predicts, list), type(predicts)
        out = torch.stack(predicts, dim=0).mean(0)
        assert out.shape == predicts[0].shape
        return out

    @staticmethod
    def _hardVoting(predicts: List[Tensor], num_classes: Optional[int] = None) -> Tensor:
        """Majority of the argmax maps, ties to the smallest class (np.bincount(...).argmax(), Summary.py:120), as a one-hot
        float map.  Like the reference it votes over the concatenated batch axis, i.e. it expects single-slice batches."""
        assert isinstance(predicts, list), type(predicts)
        C = num_classes or predicts[0].shape[1]
        votes = torch.cat([p.max(1)[1] for p in predicts], 0)
        counts = torch.stack([(votes == c).sum(0) for c in range(C)])
        winner = counts.max(0)[1]
        return torch.nn.functional.one_hot(winner, C).permute(2, 0, 1).unsqueeze(0).float()


@torch.no_grad()
def summarize(models: List[Segmentator], val_dataloader, device, ensemble_method: str = 'soft',
              report_axises: Optional[List[int]] = None, hausdorff: bool = False, spacing=None,
              kappa: bool = False, iou: bool = False, kappa_classes: Optional[List[int]] = None,
              largest_component: Optional[str] = None, lcc_classes: Optional[List[int]] = None, lcc_full: bool = False,
              temperature=None, temperature_loader=None,
              calibration: bool = False, calibration_bins: int = 15, calibration_classes: Optional[List[int]] = None) -> Dict[str, dict]:
    """Per-model and ensemble 2-D / 3-D Dice over a validation loader (batches ``[(img, gt), meta, names]``): tables ``'2d'`` and
    ``'3d'`` with keys ``DSC{j}``.  ``hausdorff=True`` adds the tables ``'hd_2d'`` and ``'hd_3d'`` with keys ``HD{j}``: mean (and
    for the ensemble the std) of the Hausdorff distance over the slices / patient batches where class j is in both the
    prediction and gt, NaN where it never is; ``spacing`` = (sz, sy, sx) of a voxel, default 1, 1, 1.

    ``kappa=True`` adds ``'kappa_2d'`` and ``'kappa_3d'``, each ``{'mean': {pair: float}, 'std': {...}, 'defined': {pair: int}}``:
    Cohen's kappa between every pair of the raters model 0 .. (``S{i}``), the ensemble vote (``ensemble``) and ``gt`` -- pairs such
    as ``S0_S1``, ``S0_ensemble``, ``ensemble_gt`` -- over the slices / patient batches where it is defined; at most 7 models.
    ``kappa_classes`` restricts it to the pixels whose second rater lies in that class set.  ``iou=True`` adds ``'iou_2d'`` and
    ``'iou_3d'`` in the layout of the Dice tables with keys ``IoU{j}``.

    ``largest_component='2d'`` / ``'3d'`` also scores every prediction and the ensemble vote with only the largest connected component
    of each class in ``lcc_classes`` kept (default: every class but 0; the rest goes to class 0), found per slice / per loader batch as
    a volume, with 4- / 6-connectivity (8- / 26- with ``lcc_full``): every table that is switched on gets a twin named ``..._lcc``
    (``'2d_lcc'``, ``'hd_3d_lcc'``, ``'kappa_2d_lcc'``, ...), and ``'components'`` = ``{model_i | ensemble: {'CC{j}': mean number of
    components of class j, 'removed{j}': mean share of its pixels that the cleaning removed}}`` over the slices / batches that hold the
    class.  The tables without the suffix are what they are without the argument.

    ``calibration=True`` adds ``'calibration_2d'`` and ``'calibration_3d'`` = ``{model_i | ensemble: {'ECE', 'MCE', 'Brier', 'NLL'}}``
    plus ``ensemble_std``: expected and maximum calibration error over ``calibration_bins`` equal confidence bins, Brier score and
    negative log-likelihood (include/dct.h, ``dct_calibration_counts``), mean over the slices / patient batches that hold a counted
    pixel; ``calibration_classes`` counts only the pixels whose gt lies in that class set.  It also adds ``'reliability'`` =
    ``{model_i | ensemble: {'count': [...], 'accuracy': [...], 'confidence': [...], 'coverage': [...], 'kept_accuracy': [...]}}``, one
    entry per bin, pooled over the loader: the reliability diagram, and at each bin's lower edge the share of the counted pixels at
    or above it and their accuracy (the curve a pseudo-label ``threshold=`` is read from).  The ensemble rater of these tables is
    always the MEAN of the models' probabilities, whatever ``ensemble_method`` is: a hard vote has no confidence.  They get no
    ``_lcc`` twin: the cleaned maps are one-hot.

    ``temperature='fit'`` fits one temperature per model and one for the mean of their probabilities (``metrics.TemperatureScaler``,
    include/dct.h ``dct_temperature_sums``; over the pixels of ``calibration_classes``) on ``temperature_loader`` if one is given, else
    on ``val_dataloader`` itself; a list of R = models + 1 numbers gives the temperatures instead.  A fit on the set that is reported
    is optimistic: the reported NLL is then the minimum over T on that very set; fit on held-out data (``temperature_loader``) for
    figures that carry over.  The fit re-runs the models' eval forward in each of its five walks and caches no logits.  It adds
    ``'temperature'`` = ``{model_i | ensemble: {'T', 'NLL_before', 'NLL_after', 'at_bound'}, 'fitted_on': 'temperature_loader' |
    'val_dataloader' | 'given', 'curve': {model_i | ensemble: {'T': [...], 'NLL': [...]}}}`` (NLL pooled over the fitting set's
    counted pixels; the curve is the fit's first grid, T from 16 down to 1/16; empty for given temperatures), and with
    ``calibration=True`` the twins ``'calibration_2d_ts'``, ``'calibration_3d_ts'`` and ``'reliability_ts'`` of the scaled
    probabilities (one more eval forward per batch for the logits).  Every other table is what it is without the argument: scaling never changes a hard prediction."""
    assert largest_component in (None, '2d', '3d'), largest_component
    device = torch.device(device)
    C = models[0].arch_params['num_classes']
    axes = report_axises if report_axises is not None else list(range(C))
    ens = Ensembleway(ensemble_method, C)
    for m in models:
        m.to(device)
        m.eval()
    names = [f"S{i}" for i in range(len(models))] + ["ensemble"]
    if calibration:
        assert len(models) <= 8, "calibration tables: at most 8 models (dct_calibration_counts takes 8 views)"
    if kappa or iou:
        assert len(models) <= 7, "kappa / iou tables: at most 7 models beside the ensemble (dct_confusion_counts takes 8 predictions)"
    sp = tuple(spacing) if spacing is not None else (1., 1., 1.)

    def meter_set():
        groups = [([DiceMeter(method=method, report_axises=axes, C=C) for _ in models], DiceMeter(method=method, report_axises=axes, C=C))
                  for method in ('2d', '3d')]
        if hausdorff:
            for method in ('2d', '3d'):
                groups.append(([HausdorffMeter(method=method, report_axises=axes, C=C, spacing=sp) for _ in models],
                               HausdorffMeter(method=method, report_axises=axes, C=C, spacing=sp)))
        agree = []
        if kappa or iou:
            agree = [AgreementMeter(method=method, C=C, n_models=len(names), with_gt=True, considered_classes=kappa_classes,
                                    rater_names=names) for method in ('2d', '3d')]
        return groups, agree

    def feed(meters, preds, v, gt):
        groups, agree = meters
        for a in agree:
            a.add(preds + [v], gt)
        for per_model, ensemble in groups:
            for j, p in enumerate(preds):
                per_model[j].add(p, gt)
            ensemble.add(v, gt)

    raw = meter_set()
    calib = [CalibrationMeter(method=method, C=C, n_models=len(models), with_ensemble=True, n_bins=calibration_bins,
                              considered_classes=calibration_classes, from_logits=False, rater_names=names[:-1])
             for method in ('2d', '3d')] if calibration else []
    scaler, fitted_on = None, None
    if temperature is not None:
        assert len(models) <= 8, "temperature scaling: at most 8 models (dct_temperature_sums takes 8 views)"
        scaler = TemperatureScaler(C=C, n_models=len(models), with_ensemble=True, considered_classes=calibration_classes,
                                   rater_names=names[:-1])
        if isinstance(temperature, str):
            assert temperature == 'fit', temperature
            fit_loader = temperature_loader if temperature_loader is not None else val_dataloader
            fitted_on = 'temperature_loader' if temperature_loader is not None else 'val_dataloader'

            class _Logits(object):          # re-iterable: every walk of the fit runs the eval forward again
                def __iter__(self):
                    for (img, gt), _, _ in fit_loader:
                        img = img.to(device)
                        yield [m.predict(img, logit=True) for m in models], gt.to(device)

            scaler.fit(_Logits())
        else:
            scaler.set_temperature(temperature)
            fitted_on = 'given'
    calib_ts = [CalibrationMeter(method=method, C=C, n_models=len(names), with_ensemble=False, n_bins=calibration_bins,
                                 considered_classes=calibration_classes, from_logits=False, rater_names=names)
                for method in ('2d', '3d')] if calibration and scaler is not None else []
    cleaned = meter_set() if largest_component else None
    comp = [ComponentMeter(method=largest_component, C=C) for _ in names] if largest_component else []
    for (img, gt), _, _ in val_dataloader:
        img, gt = img.to(device), gt.to(device)
        preds = [m.predict(img, logit=False) for m in models]
        v = ens(preds)
        feed(raw, preds, v, gt)
        for c in calib:
            c.add(preds, gt)
        if calib_ts:
            scaled = scaler.apply([m.predict(img, logit=True) for m in models])
            for c in calib_ts:
                c.add(scaled, gt)
        if cleaned is not None:
            kept = []
            for meter, p in zip(comp, preds + [v]):
                onehot, stats = keep_largest_component(p, method=largest_component, classes=lcc_classes, background=0,
                                                       full_connectivity=lcc_full, return_stats=True)
                meter.add(stats)
                kept.append(onehot)
            feed(cleaned, kept[:-1], kept[-1], gt)

    def table(meter, key):
        (_, _), (means, stds) = meter.value()
        return {f'{key}{j}': float(means[j]) for j in range(C)}, {f'{key}{j}': float(stds[j]) for j in range(C)}

    out: Dict[str, dict] = {}

    def tables(meters, suffix):
        groups, agree = meters
        for name, key, pair in zip(("2d", "3d", "hd_2d", "hd_3d"), ("DSC", "DSC", "HD", "HD"), groups):
            res = {f'model_{i}': table(m, key)[0] for i, m in enumerate(pair[0])}
            res['ensemble'] = table(pair[1], key)[0]
            res['ensemble_std'] = table(pair[1], key)[1]
            out[name + suffix] = res
        for a in agree:
            if kappa:
                mean, std, n = a.kappa()
                out[f'kappa_{a.method}{suffix}'] = {'mean': {k: float(mean[p]) for p, k in enumerate(a.pairs)},
                                                    'std': {k: float(std[p]) for p, k in enumerate(a.pairs)},
                                                    'defined': {k: int(n[p]) for p, k in enumerate(a.pairs)}}
            if iou:
                mean, std = a.iou()
                res = {f'model_{i}': {f'IoU{j}': float(mean[i][j]) for j in range(C)} for i in range(len(models))}
                res['ensemble'] = {f'IoU{j}': float(mean[-1][j]) for j in range(C)}
                res['ensemble_std'] = {f'IoU{j}': float(std[-1][j]) for j in range(C)}
                out[f'iou_{a.method}{suffix}'] = res

    tables(raw, "")
    keys = [f'model_{i}' for i in range(len(models))] + ['ensemble']
    for meters, suffix in ((calib, ""), (calib_ts, "_ts")):
        for c in meters:
            stats = {k: fn() for k, fn in (('ECE', c.ece), ('MCE', c.mce), ('Brier', c.brier), ('NLL', c.nll))}
            res = {key: {k: float(stats[k][0][r]) for k in stats} for r, key in enumerate(keys)}
            res['ensemble_std'] = {k: float(stats[k][1][-1]) for k in stats}
            out[f'calibration_{c.method}{suffix}'] = res
        if meters:
            count, acc, conf = meters[0].reliability()
            cov, kept = meters[0].coverage_accuracy()
            out['reliability' + suffix] = {key: {'count': count[r].tolist(), 'accuracy': acc[r].tolist(), 'confidence': conf[r].tolist(),
                                                 'coverage': cov[r].tolist(), 'kept_accuracy': kept[r].tolist()}
                                           for r, key in enumerate(keys)}
    if scaler is not None:
        res = dict(zip(keys, scaler.detailed_summary().values()))
        res['fitted_on'] = fitted_on
        ct, cn = scaler.curve()
        res['curve'] = {key: {'T': ct[r].tolist(), 'NLL': cn[r].tolist()} for r, key in enumerate(keys)}
        out['temperature'] = res
    if cleaned is not None:
        tables(cleaned, "_lcc")
        out['components'] = {(f'model_{i}' if i < len(models) else 'ensemble'): m.detailed_summary() for i, m in enumerate(comp)}
    return out
