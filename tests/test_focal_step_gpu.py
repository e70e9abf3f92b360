"""``FocalLoss2d`` in the co-training step: the fused launch sequence (``dct_focal_step`` for the supervised term and for the FGSM
generator's criterion) against the generic step through the public modules, the captured step against eager launches (with the
weights changed in place on the way), the capture signature, and the routes of the sum / map reductions.  The set-ups are
tests/test_weighted_step_gpu.py's: the golden ``g5_step_unet_adv`` trainer and the small two-model UNet / Enet trainers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_step_gpu import _seeded_state  # noqa: E402
from test_weighted_step_gpu import DEV, WEIGHT, _moments_agree, _one_step  # noqa: E402

GAMMA = 2.0


def _trainer(tmp_path, g, n_steps, sup, fused=True):
    """test_weighted_step_gpu's trainer of a golden set-up (fp32), with ``sup`` as the supervised criterion."""
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
    crit = {"sup": sup, "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segmentators=segs, labeled_dataloaders=lab, unlabeled_dataloader=unl, val_dataloader=unl,
                   criterions=crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=list(range(1, C)),
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": float(g["lam_cot"])},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": float(g["lam_adv"])},
                   adv_training_dict={"eplision": float(g["eps"])}, use_tqdm=False, steps_per_epoch=n_steps)
    if not fused:
        tr._fused_ok = lambda: False
    return tr, lab, unl


def _focal(**kw):
    from dct_amd.loss import get_loss_fn
    return get_loss_fn("focal", **{"gamma": GAMMA, "weight": WEIGHT, **kw})


@pytest.fixture(scope="module")
def focal_fused_step(golden, tmp_path_factory):
    g = golden("g5_step_unet_adv")
    assert str(g["arch"]) == "unet" and int(g["C"]) == len(WEIGHT)
    tr, lab, unl = _trainer(tmp_path_factory.mktemp("fused"), g, 1, _focal())
    assert tr._fused_ok()                        # a focal criterion with the mean reduction stays on the fused step
    out, w = _one_step(tr, lab, unl)
    assert tr.last_route.joint_pass or tr.last_route.model_streams        # (a fused route, not the generic one)
    return out, w


def test_focal_fused_and_generic_paths_agree(golden, tmp_path, focal_fused_step):
    """test_weighted_fused_and_generic_paths_agree with gamma = 2 and class weights, at that test's tolerances: both paths run the same
    per-pixel math.  The adversarial value and model a's weights depend on the FGSM generator's criterion being focal too."""
    a, wa = focal_fused_step
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, _focal(), fused=False)
    b, wb = _one_step(tr, lab, unl)
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    _moments_agree(wa, wb)


def test_focal_reaches_the_fused_step(golden, tmp_path, focal_fused_step):
    """No silent fall-through to the cross-entropy kernels: the focal supervised losses are not the weighted CE trainer's."""
    from dct_amd.loss import get_loss_fn
    a, _ = focal_fused_step
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, get_loss_fn("cross_entropy", weight=WEIGHT))
    b, _ = _one_step(tr, lab, unl)
    for x, y in zip(a["sup"], b["sup"]):
        assert abs(x.item() - y.item()) > 1e-3 * abs(y.item()), (x.item(), y.item())


def test_the_fgsm_generator_uses_focal(golden, tmp_path, focal_fused_step):
    """The same fused step with the generator's criterion swapped for the plain cross entropy (the context's focal arguments and
    weights hidden from _fgsm_fused alone).  The fused step is deterministic -- the supervised losses of the two runs are equal bit for
    bit, as the replay tests rely on -- so any difference in the adversarial value is the generator's criterion: the two criteria's
    input gradients differ in sign at some pixels only, and FGSM moves each pixel by eps = 0.03 along the sign, so the value moves
    little; it must move."""
    a, _ = focal_fused_step
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, _focal())
    real = tr._fgsm_fused

    def plain(ctx, *args, **kw):
        keep = ctx.focal, ctx.ce_weight
        ctx.focal = ctx.ce_weight = None
        try:
            return real(ctx, *args, **kw)
        finally:
            ctx.focal, ctx.ce_weight = keep
    tr._fgsm_fused = plain
    b, _ = _one_step(tr, lab, unl)
    assert [s.item() for s in a["sup"]] == [s.item() for s in b["sup"]]
    print(f"adv with a focal generator {a['adv'].item()!r}, with a cross-entropy generator {b['adv'].item()!r}")
    assert a["adv"].item() != b["adv"].item()


@pytest.mark.parametrize("arch,adv", [("unet", True), ("enet", False)])
def test_focal_graph_replay_equals_eager_step_sequence(tmp_path, arch, adv):
    """test_weighted_graph_replay_equals_eager_step_sequence with a focal criterion; at step 4 the learning rate, lambda_cot and the
    criterion's device weight buffer change in place.  No new capture, and exactly the eager steps' results."""
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
        crit = {"sup": get_loss_fn("focal", gamma=GAMMA, weight=WEIGHT[:C]), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        tr.use_hip_graph = use_graph
        for s in segs:
            s.train()
        sups, captures = [], None
        for k in range(n):
            if k == 4:                          # between replays: lr, lambda_cot and the class weights change
                for s in segs:
                    s.optimizer.param_groups[0]["lr"] = 3e-4
                tr.cot_scheduler.max_value = 0.25
                crit["sup"].device_weight(DEV, C).copy_(torch.tensor([2.0, 0.3, 0.75], device=DEV))
                captures = tr._step_graphs.captures if use_graph else None
            lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
            out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, adv, (0, 1) if adv else None)
            sups.append([float(v) for v in out["sup"]])
        torch.cuda.synchronize()
        if use_graph:
            assert tr._step_graphs is not None and tr._step_graphs.captures >= 1 and tr._step_graphs.replays >= 4
            assert tr._step_graphs.captures == captures            # nothing was captured anew after the in-place changes
        res.append(dict(
            w=[torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in segs],
            m=[s.optimizer._m.cpu() for s in segs], steps=[s.optimizer._steps for s in segs],
            dev_steps=[float(s.optimizer._dev_state[0]) for s in segs], sups=sups))
    a, b = res
    assert a["steps"] == b["steps"] == [n, n] and a["dev_steps"] == b["dev_steps"] == [float(n)] * 2
    assert a["sups"] == b["sups"]
    for x, y in zip(a["w"] + a["m"], b["w"] + b["m"]):
        assert torch.equal(x, y)


def test_another_gamma_or_criterion_is_another_capture(tmp_path, golden):
    """StepGraphCache._signature carries the criterion's type and launch arguments: another gamma, or the cross entropy in place of
    the focal loss (on the very same weight buffer), changes it; changing the weights in place does not."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.trainer.step_graph import StepGraphCache
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, _focal())
    _one_step(tr, lab, unl)                      # (flat parameters and gradients exist)
    cache = StepGraphCache(tr)
    lb = [(lab[i][0][0][0].to(DEV), lab[i][0][0][1].to(DEV)) for i in range(2)]

    def sig():
        return cache._signature(lb, None, False, False, None, (0.0, 0.0), "one_graph", tr.last_route)
    focal = tr.criterions["sup"]
    s0 = sig()
    focal.device_weight(DEV).mul_(0.5)
    assert sig() == s0
    focal.gamma = 1.0
    s1 = sig()
    focal.gamma = 0.0
    s2 = sig()
    focal.gamma = GAMMA
    assert sig() == s0
    ce = get_loss_fn("cross_entropy", weight=WEIGHT)
    ce._device_weights = focal._device_weights  # the same buffer: only the criterion's type and arguments tell the two apart
    tr.criterions["sup"] = ce
    assert ce.device_weight(DEV) is focal.device_weight(DEV)
    assert len({s0, s1, s2, sig()}) == 4


@pytest.mark.parametrize("kw", [dict(size_average=False), dict(reduce=False), dict(weight=None, size_average=False)])
def test_sum_and_map_criteria_take_the_generic_route(tmp_path, golden, kw):
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, _focal(**kw))
    assert not tr._fused_ok()
    if kw.get("reduce", True):
        out, _ = _one_step(tr, lab, unl)
        r = tr.last_route                        # the generic step's route: one autograd backward behind a zero_grad, nothing forked
        assert r.overwrite == ("none", "none") and not r.model_streams and not r.joint_pass and tr._step_graphs is None
        assert all(np.isfinite(s.item()) and s.item() > 100 for s in out["sup"])         # a sum over the batch's pixels, not a mean
