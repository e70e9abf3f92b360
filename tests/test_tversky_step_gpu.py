"""``TverskyLoss`` / ``FocalTverskyLoss`` / ``CrossEntropyTverskyLoss2d`` as the supervised criterion of the co-training step: the fused
launch sequence (``dct_ce_tversky_step`` for the supervised term and for the FGSM generator's criterion) against the generic step
through the public modules, the captured step against eager launches (with the class weights changed in place on the way), and the
captured-step signature.  Method, shapes and tolerances are tests/test_dice_step_gpu.py's, on golden set-up ``g5_step_unet_adv``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_dice_step_gpu import DICE, _sup, _trainer  # noqa: E402
from test_weighted_step_gpu import DEV, WEIGHT, _moments_agree, _one_step  # noqa: E402

CE_TVERSKY = dict(weight=WEIGHT, ce_coef=1.0, tversky_coef=1.0, alpha=0.3, beta=0.7, gamma=4.0 / 3.0, classes=[1, 2, 3], smooth=1e-5)
FOCAL_TVERSKY = dict(classes=[1, 2, 3], per_image=True)


@pytest.fixture(scope="module")
def fused_steps(golden, tmp_path_factory):
    """One fused step per criterion: name -> (step output, weight digests)."""
    g = golden("g5_step_unet_adv")
    assert str(g["arch"]) == "unet" and int(g["C"]) == len(WEIGHT)
    res = {}
    for name, kw in (("ce_tversky", CE_TVERSKY), ("focal_tversky", FOCAL_TVERSKY)):
        tr, lab, unl = _trainer(tmp_path_factory.mktemp(name), g, 1, _sup(name, kw))
        assert tr._fused_ok()                    # the Tversky family stays on the fused step
        res[name] = _one_step(tr, lab, unl)
        assert tr.last_route.joint_pass or tr.last_route.model_streams        # (a fused route, not the generic one)
        last = tr.criterions["sup"].last_tversky
        assert last is not None and last.is_cuda and last.shape[1] == int(g["C"]) and bool(torch.isfinite(last).all())
    return res


@pytest.mark.parametrize("name,kw", [("ce_tversky", CE_TVERSKY), ("focal_tversky", FOCAL_TVERSKY)])
def test_tversky_fused_and_generic_paths_agree(golden, tmp_path, fused_steps, name, kw):
    """test_dice_fused_and_generic_paths_agree with a CE + focal Tversky (G = 1, foreground, class weights) and a focal-Tversky-only
    (G = B, foreground, the paper's defaults) criterion, at that test's tolerances.  The adversarial value and model a's weights depend on
    the FGSM generator's criterion being the same one, pseudo-labelled tail included."""
    a, wa = fused_steps[name]
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, _sup(name, kw), fused=False)
    b, wb = _one_step(tr, lab, unl)
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    _moments_agree(wa, wb)


def test_tversky_reaches_the_fused_step(golden, tmp_path, tmp_path_factory, fused_steps):
    """No silent fall-through to the cross-entropy or the Dice kernels: the supervised values are neither a plain-CE trainer's, nor a
    Dice trainer's, nor each other's."""
    from dct_amd.loss import get_loss_fn
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, get_loss_fn("cross_entropy"))
    ce, _ = _one_step(tr, lab, unl)
    tr, lab, unl = _trainer(tmp_path_factory.mktemp("dice"), g, 1, _sup("dice", DICE))
    dice, _ = _one_step(tr, lab, unl)
    for name in ("ce_tversky", "focal_tversky"):
        for other in (ce, dice):
            for x, y in zip(fused_steps[name][0]["sup"], other["sup"]):
                assert abs(x.item() - y.item()) > 1e-3 * abs(y.item()), (name, x.item(), y.item())
    for x, y in zip(fused_steps["ce_tversky"][0]["sup"], fused_steps["focal_tversky"][0]["sup"]):
        assert abs(x.item() - y.item()) > 1e-3 * abs(y.item()), (x.item(), y.item())


@pytest.mark.parametrize("arch,adv,name", [("unet", True, "ce_tversky"), ("enet", False, "ce_tversky")])
def test_tversky_graph_replay_equals_eager_step_sequence(tmp_path, arch, adv, name):
    """test_dice_graph_replay_equals_eager_step_sequence with a CE + focal Tversky criterion: its device weight buffer changes in place at
    step 4 -- no new capture, and exactly the eager steps' results."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B, H, n = 3, 2, (176 if arch == "unet" else 64), 7
    kw = dict(weight=WEIGHT[:C], tversky_coef=0.5, alpha=0.3, beta=0.7, gamma=4.0 / 3.0, classes=[1, 2], per_image=True)
    res = []
    for use_graph in (False, True):
        segs = []
        for seed in (11, 12):
            torch.manual_seed(seed)
            segs.append(Segmentator({"name": arch, "num_classes": C, "compute_dtype": torch.bfloat16},
                                    {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
        lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(2)]
        unl = FakeLoader(batches(91, n, B, H, C), B)
        crit = {"sup": get_loss_fn(name, **kw), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        tr.use_hip_graph = use_graph
        assert tr._fused_ok()
        for s in segs:
            s.train()
        sups = []
        for k in range(n):
            if k == 4:                          # between replays: lr, lambda_cot and the class weights change
                for s in segs:
                    s.optimizer.param_groups[0]["lr"] = 3e-4
                tr.cot_scheduler.max_value = 0.25
                crit["sup"].device_weight(DEV, C).copy_(torch.tensor([2.0, 0.3, 0.75], device=DEV))
            lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
            out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, adv, (0, 1) if adv else None)
            sups.append([float(v) for v in out["sup"]])
        torch.cuda.synchronize()
        if use_graph:
            assert tr._step_graphs is not None and tr._step_graphs.captures >= 1 and tr._step_graphs.replays >= 4
        res.append(dict(
            w=[torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in segs],
            m=[s.optimizer._m.cpu() for s in segs], steps=[s.optimizer._steps for s in segs],
            dev_steps=[float(s.optimizer._dev_state[0]) for s in segs], sups=sups))
    a, b = res
    assert a["steps"] == b["steps"] == [n, n] and a["dev_steps"] == b["dev_steps"] == [float(n)] * 2
    assert a["sups"] == b["sups"] and all(np.isfinite(v) for s in a["sups"] for v in s)
    for x, y in zip(a["w"] + a["m"], b["w"] + b["m"]):
        assert torch.equal(x, y)


def test_another_tversky_criterion_is_another_capture(tmp_path, golden):
    """StepGraphCache._signature carries the criterion's module type and launch arguments: another alpha, beta or gamma (or coefficient,
    mask, smooth, per_image) is another capture, an in-place weight change is not."""
    from dct_amd.trainer.step_graph import StepGraphCache
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, _sup("ce_tversky", CE_TVERSKY))
    _one_step(tr, lab, unl)                      # (flat parameters and gradients exist)
    cache = StepGraphCache(tr)
    lb = [(lab[i][0][0][0].to(DEV), lab[i][0][0][1].to(DEV)) for i in range(2)]

    def sig():
        return cache._signature(lb, None, False, False, None, (0.0, 0.0), "one_graph", tr.last_route)
    s0 = sig()
    tr.criterions["sup"].device_weight(DEV).mul_(0.5)
    assert sig() == s0
    sigs = [s0]
    noweight = {k: v for k, v in CE_TVERSKY.items() if k != "weight"}
    for name, kw in (("ce_tversky", noweight), ("ce_tversky", dict(noweight, alpha=0.4)), ("ce_tversky", dict(noweight, beta=0.6)),
                     ("ce_tversky", dict(noweight, gamma=1.0)), ("ce_tversky", dict(noweight, gamma=2.0)), ("ce_tversky", dict(noweight, classes=[1, 2])),
                     ("ce_tversky", dict(noweight, per_image=True)), ("ce_tversky", dict(noweight, smooth=1.0)), ("ce_tversky", dict(noweight, ce_coef=0.5)),
                     ("ce_tversky", dict(noweight, tversky_coef=0.5)), ("ce_tversky", dict(noweight, ce_coef=0.0)),
                     ("focal_tversky", dict(classes=[1, 2, 3])), ("tversky", dict(classes=[1, 2, 3])), ("dice", dict(classes=[1, 2, 3])),
                     ("cross_entropy", dict())):
        tr.criterions["sup"] = _sup(name, kw)
        sigs.append(sig())
    # ("ce_tversky" with ce_coef = 0 and "focal_tversky" launch the same kernels with the same arguments; the module type still tells them apart)
    assert len(set(sigs)) == len(sigs)
