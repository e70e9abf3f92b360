"""``TopKCrossEntropyLoss2d`` in the co-training step: the fused launch sequence (``dct_topk_ce_step`` for the supervised term and for
the FGSM generator's criterion) against the generic step through the public module, the captured step against eager launches (with the
weights changed in place on the way), the capture signature, and a default-criteria trainer that routes and launches as it did.  The
set-ups are tests/test_focal_step_gpu.py's: the golden ``g5_step_unet_adv`` trainer and the small two-model UNet trainer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_focal_step_gpu import _trainer  # noqa: E402
from test_weighted_step_gpu import DEV, WEIGHT, _moments_agree, _one_step  # noqa: E402

K_PERCENT = 10


def _topk(**kw):
    from dct_amd.loss import get_loss_fn
    return get_loss_fn("topk_ce", **{"k": K_PERCENT, "weight": WEIGHT, **kw})


def _recorded(monkeypatch):
    """The names of the C-ABI calls issued from here on."""
    from dct_amd import hip_ops
    seen = []
    real = hip_ops.call
    monkeypatch.setattr(hip_ops, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    return seen


@pytest.fixture(scope="module")
def topk_fused_step(golden, tmp_path_factory):
    g = golden("g5_step_unet_adv")
    assert str(g["arch"]) == "unet" and int(g["C"]) == len(WEIGHT)
    sup = _topk()
    tr, lab, unl = _trainer(tmp_path_factory.mktemp("fused"), g, 1, sup)
    assert tr._fused_ok()                        # a top-k criterion stays on the fused step
    out, w = _one_step(tr, lab, unl)
    assert tr.last_route.joint_pass or tr.last_route.model_streams        # (a fused route, not the generic one)
    torch.cuda.synchronize()
    return out, w, sup.last_topk, tr._step_facts(), tr.last_route


def test_topk_fused_and_generic_paths_agree(golden, tmp_path, topk_fused_step):
    """test_focal_fused_and_generic_paths_agree with the top-k criterion (k = 10, class weights), at that test's tolerances.  The
    adversarial value and model a's weights depend on the FGSM generator's criterion being the top-k one too."""
    a, wa, last, _, _ = topk_fused_step
    sup = _topk()
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, sup, fused=False)
    b, wb = _one_step(tr, lab, unl)
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    _moments_agree(wa, wb)
    # last_topk is set from the fused step too: device tensors, K = max(1, int(N k / 100)) of the counted pixels
    for out2, counts4 in (last, sup.last_topk):
        assert out2.is_cuda and counts4.is_cuda and counts4.dtype == torch.int64
        K, N, n_gt, n_eq = counts4.tolist()
        assert N > 0 and K == max(1, int(N * K_PERCENT / 100)) and n_gt < K <= n_gt + n_eq
        assert np.isfinite(out2.cpu().numpy()).all() and out2[0].item() >= out2[1].item()      # the mean of the top K is at least tau


def test_topk_reaches_the_fused_step(golden, tmp_path, topk_fused_step, monkeypatch):
    """No silent fall-through to the cross-entropy kernels: the launches are dct_topk_ce_step's -- the two supervised terms and the
    FGSM generator's criterion --, and the supervised values are not the weighted cross entropy's."""
    from dct_amd.loss import get_loss_fn
    a = topk_fused_step[0]
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, _topk())
    seen = _recorded(monkeypatch)
    _one_step(tr, lab, unl)
    assert seen.count("dct_topk_ce_step") == 3 and not [n for n in seen if n.startswith(("dct_ce_", "dct_focal_"))], seen
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, get_loss_fn("cross_entropy", weight=WEIGHT))
    b, _ = _one_step(tr, lab, unl)
    for x, y in zip(a["sup"], b["sup"]):
        assert abs(x.item() - y.item()) > 1e-3 * abs(y.item()), (x.item(), y.item())


def test_default_criteria_route_and_launch_as_before(golden, tmp_path, topk_fused_step, monkeypatch):
    """A trainer with the default cross entropy sees the planner facts and the route of the top-k trainer (the criterion changes the
    loss launches, nothing else), and issues dct_ce_step where that one issues dct_topk_ce_step: none of the new entry points."""
    from dct_amd.loss import get_loss_fn
    _, _, _, facts, route = topk_fused_step
    tr, lab, unl = _trainer(tmp_path, golden("g5_step_unet_adv"), 1, get_loss_fn("cross_entropy"))
    assert tr._fused_ok()
    seen = _recorded(monkeypatch)
    _one_step(tr, lab, unl)
    assert not [n for n in seen if "topk" in n] and seen.count("dct_ce_step") == 3, seen
    assert tr._step_facts() == facts
    assert tr.last_route == route, (tr.last_route, route)


def test_topk_graph_replay_equals_eager_step_sequence(tmp_path):
    """test_focal_graph_replay_equals_eager_step_sequence with the top-k criterion on the small UNet; at step 4 the learning rate,
    lambda_cot and the criterion's device weight buffer change in place.  Eager launches, the captured step and its replays give the
    same numbers bit for bit, and nothing is captured anew."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B, H, n = 3, 2, 176, 7
    res = []
    for use_graph in (False, True):
        segs = []
        for seed in (11, 12):
            torch.manual_seed(seed)
            segs.append(Segmentator({"name": "unet", "num_classes": C, "compute_dtype": torch.bfloat16},
                                    {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
        lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(2)]
        unl = FakeLoader(batches(91, n, B, H, C), B)
        crit = {"sup": get_loss_fn("topk_ce", k=K_PERCENT, weight=WEIGHT[:C]), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        tr.use_hip_graph = use_graph
        for s in segs:
            s.train()
        sups, counts, captures = [], [], None
        for k in range(n):
            if k == 4:                          # between replays: lr, lambda_cot and the class weights change
                for s in segs:
                    s.optimizer.param_groups[0]["lr"] = 3e-4
                tr.cot_scheduler.max_value = 0.25
                crit["sup"].device_weight(DEV, C).copy_(torch.tensor([2.0, 0.3, 0.75], device=DEV))
                captures = tr._step_graphs.captures if use_graph else None
            lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
            out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, True, (0, 1))
            sups.append([float(v) for v in out["sup"]])
            counts.append(crit["sup"].last_topk[1].tolist())
        torch.cuda.synchronize()
        if use_graph:
            assert tr._step_graphs is not None and tr._step_graphs.captures >= 1 and tr._step_graphs.replays >= 4
            assert tr._step_graphs.captures == captures            # nothing was captured anew after the in-place changes
        res.append(dict(
            w=[torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in segs],
            m=[s.optimizer._m.cpu() for s in segs], steps=[s.optimizer._steps for s in segs],
            dev_steps=[float(s.optimizer._dev_state[0]) for s in segs], sups=sups, counts=counts))
    a, b = res
    assert a["steps"] == b["steps"] == [n, n] and a["dev_steps"] == b["dev_steps"] == [float(n)] * 2
    assert a["sups"] == b["sups"] and a["counts"] == b["counts"]
    assert all(K >= 1 and n_gt < K <= n_gt + n_eq for step in a["counts"] for K, N, n_gt, n_eq in [step])
    for x, y in zip(a["w"] + a["m"], b["w"] + b["m"]):
        assert torch.equal(x, y)


def test_another_k_is_another_capture(tmp_path, golden):
    """StepGraphCache._signature carries the criterion's type and launch arguments: another k, or the cross entropy in place of the
    top-k criterion (on the very same weight buffer), changes it; changing the weights in place does not."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.trainer.step_graph import StepGraphCache
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, _topk())
    _one_step(tr, lab, unl)                      # (flat parameters and gradients exist)
    cache = StepGraphCache(tr)
    lb = [(lab[i][0][0][0].to(DEV), lab[i][0][0][1].to(DEV)) for i in range(2)]

    def sig():
        return cache._signature(lb, None, False, False, None, (0.0, 0.0), "one_graph", tr.last_route)
    topk = tr.criterions["sup"]
    s0 = sig()
    topk.device_weight(DEV).mul_(0.5)
    assert sig() == s0
    topk.k = 25.0
    s1 = sig()
    topk.k = 100.0
    s2 = sig()
    topk.k = float(K_PERCENT)
    assert sig() == s0
    ce = get_loss_fn("cross_entropy", weight=WEIGHT)
    ce._device_weights = topk._device_weights    # the same buffer: only the criterion's type and arguments tell the two apart
    tr.criterions["sup"] = ce
    assert ce.device_weight(DEV) is topk.device_weight(DEV)
    assert len({s0, s1, s2, sig()}) == 4
