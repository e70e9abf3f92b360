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
Hausdorff distance (``dct_hausdorff``) and the confusion matrices behind kappa and IoU (``dct_confusion_counts``) run on the
device."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
from torch import Tensor

from .metrics import AgreementMeter, DiceMeter, HausdorffMeter
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
              kappa: bool = False, iou: bool = False, kappa_classes: Optional[List[int]] = None) -> Dict[str, dict]:
    """Per-model and ensemble 2-D / 3-D Dice over a validation loader (batches ``[(img, gt), meta, names]``): tables ``'2d'`` and
    ``'3d'`` with keys ``DSC{j}``.  ``hausdorff=True`` adds the tables ``'hd_2d'`` and ``'hd_3d'`` with keys ``HD{j}``: mean (and
    for the ensemble the std) of the Hausdorff distance over the slices / patient batches where class j is in both the
    prediction and gt, NaN where it never is; ``spacing`` = (sz, sy, sx) of a voxel, default 1, 1, 1.

    ``kappa=True`` adds ``'kappa_2d'`` and ``'kappa_3d'``, each ``{'mean': {pair: float}, 'std': {...}, 'defined': {pair: int}}``:
    Cohen's kappa between every pair of the raters model 0 .. (``S{i}``), the ensemble vote (``ensemble``) and ``gt`` -- pairs such
    as ``S0_S1``, ``S0_ensemble``, ``ensemble_gt`` -- over the slices / patient batches where it is defined; at most 7 models.
    ``kappa_classes`` restricts it to the pixels whose second rater lies in that class set.  ``iou=True`` adds ``'iou_2d'`` and
    ``'iou_3d'`` in the layout of the Dice tables with keys ``IoU{j}``."""
    device = torch.device(device)
    C = models[0].arch_params['num_classes']
    axes = report_axises if report_axises is not None else list(range(C))
    ens = Ensembleway(ensemble_method, C)
    for m in models:
        m.to(device)
        m.eval()
    d2 = [DiceMeter(method='2d', report_axises=axes, C=C) for _ in models]
    d3 = [DiceMeter(method='3d', report_axises=axes, C=C) for _ in models]
    e2, e3 = DiceMeter(method='2d', report_axises=axes, C=C), DiceMeter(method='3d', report_axises=axes, C=C)
    groups = [(d2, e2), (d3, e3)]
    if hausdorff:
        sp = tuple(spacing) if spacing is not None else (1., 1., 1.)
        for method in ('2d', '3d'):
            groups.append(([HausdorffMeter(method=method, report_axises=axes, C=C, spacing=sp) for _ in models],
                           HausdorffMeter(method=method, report_axises=axes, C=C, spacing=sp)))
    agree = []
    if kappa or iou:
        assert len(models) <= 7, "kappa / iou tables: at most 7 models beside the ensemble (dct_confusion_counts takes 8 predictions)"
        names = [f"S{i}" for i in range(len(models))] + ["ensemble"]
        agree = [AgreementMeter(method=method, C=C, n_models=len(names), with_gt=True, considered_classes=kappa_classes,
                                rater_names=names) for method in ('2d', '3d')]
    for (img, gt), _, _ in val_dataloader:
        img, gt = img.to(device), gt.to(device)
        preds = [m.predict(img, logit=False) for m in models]
        v = ens(preds)
        for a in agree:
            a.add(preds + [v], gt)
        for per_model, ensemble in groups:
            for j, p in enumerate(preds):
                per_model[j].add(p, gt)
            ensemble.add(v, gt)

    def table(meter, key):
        (_, _), (means, stds) = meter.value()
        return {f'{key}{j}': float(means[j]) for j in range(C)}, {f'{key}{j}': float(stds[j]) for j in range(C)}

    out: Dict[str, dict] = {}
    for name, key, meters in zip(("2d", "3d", "hd_2d", "hd_3d"), ("DSC", "DSC", "HD", "HD"), groups):
        res = {f'model_{i}': table(m, key)[0] for i, m in enumerate(meters[0])}
        res['ensemble'] = table(meters[1], key)[0]
        res['ensemble_std'] = table(meters[1], key)[1]
        out[name] = res
    for a in agree:
        if kappa:
            mean, std, n = a.kappa()
            out[f'kappa_{a.method}'] = {'mean': {k: float(mean[p]) for p, k in enumerate(a.pairs)},
                                        'std': {k: float(std[p]) for p, k in enumerate(a.pairs)},
                                        'defined': {k: int(n[p]) for p, k in enumerate(a.pairs)}}
        if iou:
            mean, std = a.iou()
            res = {f'model_{i}': {f'IoU{j}': float(mean[i][j]) for j in range(C)} for i in range(len(models))}
            res['ensemble'] = {f'IoU{j}': float(mean[-1][j]) for j in range(C)}
            res['ensemble_std'] = {f'IoU{j}': float(std[-1][j]) for j in range(C)}
            out[f'iou_{a.method}'] = res
    return out
