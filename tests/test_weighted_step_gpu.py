"""A class-weighted ``CrossEntropyLoss2d`` in the co-training step: the fused launch sequence (``dct_ce_weighted_step`` for the
supervised term and for the FGSM generator's cross entropy) against the generic step through the public modules, the captured step
against eager launches (with the weights changed in place on the way), and the routes of the sum / map reductions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches, digest  # noqa: E402
from test_step_gpu import _seeded_state  # noqa: E402

DEV = "cuda:0"
WEIGHT = [0.1, 1, 2.5, 0]


def _trainer(tmp_path, g, n_steps, fused=True, **ce):
    """test_step_gpu's trainer of a golden set-up (fp32), with ``CrossEntropyLoss2d(**ce)`` as the supervised criterion."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, H, B = int(g["C"]), int(g["H"]), int(g["B"])
    arch = str(g["arch"])
    segs = []
    for s in g["net_seeds"]:
        seg = Segmentator({"name": arch, "num_classes": C, "compute_dtype": torch.float32, "dropout_p": 0.0},
                          {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1})
        seg.torchnet.load_state_dict(_seeded_state(arch, C, int(s)))
        segs.append(seg)
    lab = [FakeLoader(batches(int(s), n_steps, B, H, C), B) for s in g["lab_seeds"]]
    unl = FakeLoader(batches(int(g["unl_seed"]), n_steps, B, H, C), B)
    crit = {"sup": get_loss_fn("cross_entropy", **ce), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segmentators=segs, labeled_dataloaders=lab, unlabeled_dataloader=unl, val_dataloader=unl,
                   criterions=crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=list(range(1, C)),
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": float(g["lam_cot"])},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": float(g["lam_adv"])},
                   adv_training_dict={"eplision": float(g["eps"])}, use_tqdm=False, steps_per_epoch=n_steps)
    if not fused:
        tr._fused_ok = lambda: False
    return tr, lab, unl


class _Digests(list):
    """The weight digests of ``_one_step`` with, as ``moments``, the l2 norm of Adam's first moment per model and parameter tensor."""
    moments = None


def _first_moments(tr):
    """Per model: the l2 norm of ``exp_avg`` of every parameter tensor.  After the first step that is 0.1 x the step's total gradient:
    unlike the weights (which Adam's first update moves by lr * sign(g)) it shows a wrong scale of any gradient term."""
    return [np.array([digest(s.optimizer.state[p]["exp_avg"])[2] for p in s.torchnet.parameters()]) for s in tr.segmentators]


def _moments_agree(wa, wb):
    """tests/test_step_gpu.py::test_train_loop_fp32_matches_reference_golden's UNet band for the first moments, per parameter tensor."""
    assert len(wa.moments) == len(wb.moments) == 2
    for x, y in zip(wa.moments, wb.moments):
        assert x.shape == y.shape and len(x) > 10 and np.all(np.isfinite(x)) and x.max() > 1e-6
        print(f"first moments of {len(x)} parameter tensors: norms {x.min():.3e} .. {x.max():.3e}, largest deviation "
              f"{np.max(np.abs(x - y) / (2e-2 * np.abs(y) + 1e-9)):.3f} of the band")
        np.testing.assert_allclose(x, y, rtol=2e-2, atol=1e-9)


def _one_step(tr, lab, unl):
    for s in tr.segmentators:
        s.train()
    lb = [lab[i][0][0] for i in range(2)]
    out = tr._run_step([(lb[0][0], lb[0][1]), (lb[1][0], lb[1][1])], (unl[0][0][0], unl[0][0][1]), True, True, (0, 1))
    w = _Digests(digest(torch.cat([p.detach().flatten() for p in s.torchnet.parameters()])) for s in tr.segmentators)
    w.moments = _first_moments(tr)
    return out, w


@pytest.fixture(scope="module")
def weighted_fused_step(golden, tmp_path_factory):
    g = golden("g5_step_unet_adv")
    assert str(g["arch"]) == "unet" and int(g["C"]) == len(WEIGHT)
    tr, lab, unl = _trainer(tmp_path_factory.mktemp("fused"), g, 1, weight=WEIGHT)
    assert tr._fused_ok()                        # a weighted mean criterion stays on the fused step
    out, w = _one_step(tr, lab, unl)
    assert tr.last_route.joint_pass or tr.last_route.model_streams        # (a fused route, not the generic one)
    return out, w


def test_weighted_fused_and_generic_paths_agree(golden, tmp_path, weighted_fused_step):
    """test_fused_and_generic_paths_agree with class weights, at that test's tolerances: the same comparison with one multiply per
    pixel added.  The adversarial value and model a's weights depend on the FGSM generator's cross entropy being weighted too."""
    a, wa = weighted_fused_step
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, fused=False, weight=WEIGHT)
    b, wb = _one_step(tr, lab, unl)
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    _moments_agree(wa, wb)


def test_weights_reach_the_fused_step(golden, tmp_path, weighted_fused_step):
    """No silent fall-through to dct_ce_step: the weighted supervised losses are not the unweighted trainer's."""
    a, _ = weighted_fused_step
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1)
    b, _ = _one_step(tr, lab, unl)
    for x, y in zip(a["sup"], b["sup"]):
        assert abs(x.item() - y.item()) > 1e-3 * abs(y.item()), (x.item(), y.item())


@pytest.mark.parametrize("arch,adv", [("unet", True), ("enet", False)])
def test_weighted_graph_replay_equals_eager_step_sequence(tmp_path, arch, adv):
    """test_graph_replay_equals_eager_step_sequence with a weighted criterion; at step 4 the criterion's device weight buffer changes
    in place as well.  The captured step reads the weights on the device: no new capture, and exactly the eager steps' results."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B, H, n = 3, 2, (176 if arch == "unet" else 64), 7
    res = []
    for use_graph in (False, True):
        segs = []
        for seed in (11, 12):
            torch.manual_seed(seed)
            segs.append(Segmentator({"name": arch, "num_classes": C, "compute_dtype": torch.bfloat16},
                                    {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
        lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(2)]
        unl = FakeLoader(batches(91, n, B, H, C), B)
        crit = {"sup": get_loss_fn("cross_entropy", weight=WEIGHT[:C]), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        tr.use_hip_graph = use_graph
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
    assert a["sups"] == b["sups"]
    for x, y in zip(a["w"] + a["m"], b["w"] + b["m"]):
        assert torch.equal(x, y)


def test_another_criterion_is_another_capture(tmp_path, golden):
    """StepGraphCache._signature carries (ignore_index, weight buffer address): swapping the criterion changes it, changing the weights
    in place does not."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.trainer.step_graph import StepGraphCache
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, weight=WEIGHT)
    _one_step(tr, lab, unl)                      # (flat parameters and gradients exist)
    cache = StepGraphCache(tr)
    lb = [(lab[i][0][0][0].to(DEV), lab[i][0][0][1].to(DEV)) for i in range(2)]

    def sig():
        return cache._signature(lb, None, False, False, None, (0.0, 0.0), "one_graph", tr.last_route)
    s0 = sig()
    tr.criterions["sup"].device_weight(DEV).mul_(0.5)
    assert sig() == s0
    alive = [tr.criterions["sup"]]               # (a freed weight buffer's address may be handed to the next criterion's)
    tr.criterions["sup"] = get_loss_fn("cross_entropy", weight=WEIGHT)
    assert sig() != s0
    s1 = sig()
    alive.append(tr.criterions["sup"])
    tr.criterions["sup"] = get_loss_fn("cross_entropy")
    s2 = sig()
    tr.criterions["sup"] = get_loss_fn("cross_entropy", ignore_index=7)
    assert len({s0, s1, s2, sig()}) == 4


@pytest.mark.parametrize("ce", [dict(size_average=False), dict(reduce=False), dict(weight=WEIGHT, size_average=False)])
def test_sum_and_map_criteria_take_the_generic_route(tmp_path, golden, ce):
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, **ce)
    assert not tr._fused_ok()
    if ce.get("reduce", True):
        out, _ = _one_step(tr, lab, unl)
        r = tr.last_route                        # the generic step's route: one autograd backward behind a zero_grad, nothing forked
        assert r.overwrite == ("none", "none") and not r.model_streams and not r.joint_pass and tr._step_graphs is None
        assert all(np.isfinite(s.item()) and s.item() > 100 for s in out["sup"])         # a sum over the batch's pixels, not a mean
