"""Host-side logic of the drop-in boundary on CPU: CoTrainer/_run_step op order, iterator
caching, schedulers, registry/CLI helpers, checkpoint format, flat parameter storage.
The arithmetic here comes from INJECTED oracle modules (test doubles) -- the product kernels are
HIP-only and are exercised by the -m gpu tests."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import oracle
from helpers import FakeLoader, batches, digest


# ---- test doubles built on the oracle ------------------------------------------------------------
class OracleCE(nn.Module):
    ignore_index = 255

    def forward(self, outputs, targets):
        return oracle.cross_entropy_2d(outputs, targets)


class OracleJSD(nn.Module):
    def forward(self, probs):
        return oracle.jsd_2d(probs)


class OracleKL(nn.Module):
    def __init__(self, reduce=False, eps=1e-10):
        super().__init__()
        self.reduce, self.eps = reduce, eps

    def forward(self, p, y):
        return oracle.kl_divergence_2d(p, y, self.reduce, self.eps)


class OracleFGSM:
    def __init__(self, net, eplision=0.05):
        self.net, self.eps = net, eplision

    def __call__(self, img, gt, criterion):
        x_adv, noise, probs, _ = oracle.fgsm_generate(self.net, img, gt, self.eps)
        return x_adv, noise, probs


class OracleDice:
    def __init__(self, method='2d', report_axises='all', C=4):
        self.method, self.report_axis, self.C, self.diceLog = method, report_axises, C, []

    def add(self, pred, gt):
        d = oracle.dice_2d(pred, gt) if self.method == '2d' else oracle.dice_3d(pred, gt).unsqueeze(0)
        self.diceLog.append(d)

    def value(self):
        log = torch.cat(self.diceLog) if self.diceLog else torch.zeros(1, self.C)
        rm = log.mean(1) if self.report_axis == 'all' else log[:, self.report_axis].mean(1)
        return (rm.mean(), rm.std()), (log.mean(0), log.std(0))


def _make_trainer(tmp_path, monkeypatch, arch, C, H, B, n_steps, seeds=(21, 22), lam_cot=0.5, lam_adv=0.05, eps=0.03):
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    from dct_amd.trainer import cotraining_totalloss as mod
    monkeypatch.setattr(mod, "DiceMeter", OracleDice)
    segs = []
    for s in seeds:
        torch.manual_seed(s)
        net = oracle.build_net(arch, C, **({"dropout_p": 0.0} if arch == "unet" else {}))
        segs.append(Segmentator({"name": arch, "num_classes": C}, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                                {"name": "StepLR", "step_size": 90, "gamma": 0.1}, torchnet=net,
                                softmax_fn=oracle.softmax_channels))
    lab = [FakeLoader(batches(31 + i, n_steps, B, H, C), B) for i in range(len(seeds))]
    unl = FakeLoader(batches(41, n_steps, B, H, C), B)
    crit = {"sup": OracleCE(), "jsd": OracleJSD(), "adv": OracleJSD()}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device="cpu", axises=list(range(1, C)),
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": lam_cot},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": lam_adv},
                   adv_training_dict={"eplision": eps}, use_tqdm=False, steps_per_epoch=n_steps)
    tr._fsgm_cls = OracleFGSM
    tr._kl_override = OracleKL
    return tr, lab, unl


# ---- the step: host logic == reference's loop body -------------------------------------------------
@pytest.mark.parametrize("tag", ["g5_step_enet_jsd", "g5_step_enet_adv"])
def test_train_loop_host_logic_reproduces_reference_golden(golden, tmp_path, monkeypatch, tag):
    """CoTrainer._train_loop/_run_step (generic path) driven with oracle modules reproduces what the
    reference's own _train_loop produced (captured in tests/golden): same op order, zero_grad after the
    forwards, FGSM on this step's cached batches, one backward, all optimizers stepped."""
    from dct_amd import ModelMode
    g = golden(tag)
    n, adv = int(g["n_steps"]), bool(int(g["train_adv"]))
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", int(g["C"]), int(g["H"]), int(g["B"]), n)
    assert not tr._fused_ok()
    log = []
    orig = tr._run_step
    tr._run_step = lambda *a, **k: log.append(orig(*a, **k)) or log[-1]
    np.random.seed(1234)
    dl, du = tr._train_loop(lab, unl, epoch=0, mode=ModelMode.TRAIN, save=False, train_jsd=True, train_adv=adv)
    for k in range(n):
        np.testing.assert_allclose([s.item() for s in log[k]["sup"]], g["sup"][k][:2], rtol=2e-5)
        np.testing.assert_allclose(log[k]["jsd"].item(), g["jsd"][k], rtol=2e-4, atol=1e-7)
        if adv:
            np.testing.assert_allclose(log[k]["adv"].item(), g["adv"][k], rtol=2e-3, atol=1e-7)
    np.testing.assert_allclose(dl.numpy(), g["dice_lab"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(du.numpy(), g["dice_unl"], rtol=1e-5, atol=1e-6)
    for j, seg in enumerate(tr.segmentators):
        sd = seg.torchnet.state_dict()
        names = list(g[f"m{j}_names"])
        df = np.stack([digest(sd[k]) for k in names])
        for col in (1, 2, 3):
            np.testing.assert_allclose(df[:, col], g[f"m{j}_digest_final"][:, col], rtol=1e-3, atol=1e-5)


def test_run_step_contract_and_rng(tmp_path, monkeypatch):
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", 2, 32, 2, 2)
    for s in tr.segmentators:
        s.train()
    lb = [(lab[i][0][0][0], lab[i][0][0][1]) for i in range(2)]
    ub = (unl[0][0][0], unl[0][0][1])
    np.random.seed(7)
    ref_state = np.random.RandomState(7)
    out = tr._run_step(lb, ub, True, True)          # adv_choice drawn inside: numpy RNG consumed exactly once
    ref_state.choice([0, 1], 2, replace=False)
    assert np.random.randint(1 << 30) == ref_state.randint(1 << 30)
    assert set(out) >= {"sup", "jsd", "adv", "preds", "unlab_probs"}
    assert len(out["sup"]) == 2 and out["preds"][0].shape == (2, 2, 32, 32) and out["unlab_probs"][1].shape == (2, 2, 32, 32)
    np.random.seed(7)
    st = np.random.get_state()[1].copy()
    tr._run_step(lb, ub, True, False)               # no adversarial term -> RNG untouched
    assert (np.random.get_state()[1] == st).all()
    # gradients were zeroed AFTER the forwards and every optimizer stepped once
    for s in tr.segmentators:
        assert all(int(v["step"]) == 2 for v in s.optimizer.state.values())


def test_fsgm_adv_training_reuses_cached_batches(tmp_path, monkeypatch):
    from dct_amd.utils import iterator_
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", 2, 32, 2, 3)
    its = [iterator_(l) for l in lab]
    uit = iterator_(unl)
    for it in its + [uit]:
        it.__next__()
    seen = {}

    class Spy(OracleFGSM):
        def __call__(self, img, gt, criterion):
            seen["img"], seen["gt"] = img.detach().clone(), gt.clone()
            return super().__call__(img, gt, criterion)

    tr._fsgm_cls = Spy
    loss = tr._FSGM_adv_training((tr.segmentators[0], tr.segmentators[1]), its, uit, eplision=0.03)
    assert loss.dim() == 0 and torch.isfinite(loss)
    assert torch.equal(seen["img"], torch.cat((lab[1][0][0][0], unl[0][0][0]), 0))   # labeled batch of model b + unlabeled
    assert torch.equal(seen["gt"], lab[1][0][0][1])
    assert torch.equal(its[1].__cache__()[0][0], lab[1][0][0][0])                    # iterators not advanced


def test_cotrainer_constructor_contract(tmp_path, monkeypatch):
    from dct_amd.trainer import CoTrainer
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", 2, 32, 2, 1)
    segs, crit = tr.segmentators, tr.criterions
    kw = dict(max_epoch=1, save_dir=str(tmp_path), device="cpu", use_tqdm=False,
              cot_scheduler_dict={"name": "RampScheduler", "begin_epoch": 0, "max_epoch": 50, "max_value": 0.5, "ramp_mult": -5},
              adv_scheduler_dict={"name": "RampScheduler", "begin_epoch": 20, "max_epoch": 50, "max_value": 0.05, "ramp_mult": -5})
    with pytest.raises(AssertionError):
        CoTrainer(segs, lab[:1], unl, unl, crit, **kw)                     # S models need S labeled loaders
    with pytest.raises(AssertionError):
        CoTrainer([segs[0], segs[0]], lab, unl, unl, crit, **kw)           # distinct instances
    with pytest.raises(AssertionError):
        CoTrainer(segs, lab, unl, unl, {"sup": crit["sup"], "jsd": crit["jsd"]}, **kw)   # keys == {sup,jsd,adv}
    ok = CoTrainer(segs, lab, unl, unl, crit, **kw)
    assert ok.C == 2 and abs(ok.cot_scheduler.value - 0.00336897) < 1e-8 and ok.adv_scheduler.value == 0.0
    ok.schedulerStep()
    assert ok.cot_scheduler.epoch == 1


def test_eval_loop_and_checkpoint_format(tmp_path, monkeypatch):
    from dct_amd import ModelMode
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", 2, 32, 2, 2)
    with torch.no_grad():
        d2, d3 = tr._eval_loop(unl, epoch=0, mode=ModelMode.EVAL)
    assert d2.shape == (2, 2, 2) and d3.shape == (2, 2, 2)
    tr.checkpoint(torch.tensor([0.5, 0.25]), epoch=3)
    ck = torch.load(os.path.join(str(tmp_path), "best_1.pth"), weights_only=False)
    assert set(ck) == {"segmentator", "best_score", "best_epoch"} and ck["best_epoch"] == 3
    assert set(ck["segmentator"]) == {"arch_dict", "optim_dict", "scheduler_dict", "net_state_dict",
                                      "optim_state_dict", "scheduler_state_dict"}
    tr.checkpoint(torch.tensor([0.4, 0.3]), epoch=4)            # only model 1 improved
    assert torch.load(os.path.join(str(tmp_path), "best_0.pth"), weights_only=False)["best_epoch"] == 3
    assert torch.load(os.path.join(str(tmp_path), "best_1.pth"), weights_only=False)["best_epoch"] == 4
    # DataParallel-style keys are accepted on load (segmentators.py:88-93)
    sd = copy.deepcopy(tr.segmentators[0].state_dict)
    sd["net_state_dict"] = {"module." + k: v for k, v in sd["net_state_dict"].items()}
    tr.segmentators[1].load_state_dict(sd)


# ---- small host utilities -------------------------------------------------------------------------
def test_iterator_wraps_and_caches():
    from dct_amd.utils import iterator_
    it = iterator_([1, 2, 3])
    assert [it.__next__() for _ in range(5)] == [1, 2, 3, 1, 2]
    assert it.__cache__() == 2
    fresh = iterator_([9])
    with pytest.warns(UserWarning):
        assert fresh.__cache__() == 9


def test_schedulers_match_reference_golden(golden):
    from dct_amd.scheduler import RampScheduler, ConstantScheduler, RampDownScheduler
    g = golden("g2_schedulers")
    for tag in ("cot", "adv"):
        s = RampScheduler(*g[tag + "_args"])
        vals = []
        for _ in range(60):
            vals.append(s.value)
            s.step()
        np.testing.assert_allclose(vals, g[tag], rtol=1e-12)
    c = ConstantScheduler(2, 0.3)
    assert [c.value, (c.step(), c.step(), c.value)[2]] == [0.0, 0.3]
    r = RampDownScheduler(10, 1.0, -5, 0.1, 5)
    assert r.value == 1.0
    st = r.state_dict()
    r2 = RampDownScheduler(10, 1.0, -5, 0.1, 5)
    r.step()
    r2.load_state_dict({**st, "epoch": 1})
    assert r.value == r2.value


def test_registry_and_dict_merge():
    from dct_amd.loss import get_loss_fn
    from dct_amd.utils import dict_merge
    with pytest.raises(ValueError):
        get_loss_fn("no_such_loss")
    assert type(get_loss_fn("jsd")).__name__ == "JSD_2D"
    # overrides as a command line delivers them (strings): a replaced leaf takes the type of the value it replaces
    args = {"Trainer": {"max_epoch": "3"}, "Arch": {"name": "unet"}, "StartTraining": {"train_jsd": "True"}, "New": {"k": 1}}
    cfg = {"Trainer": {"max_epoch": 300, "device": "cuda:0"}, "Arch": {"name": "enet", "num_classes": 4},
           "StartTraining": {"train_jsd": False}}
    out = dict_merge(cfg, args, True)
    assert out["Trainer"] == {"max_epoch": 3, "device": "cuda:0"} and out["Arch"] == {"name": "unet", "num_classes": 4}
    assert out["StartTraining"]["train_jsd"] is True and out["New"] == {"k": 1}
    assert dict_merge({"a": 1}, None, True) == {"a": 1} and dict_merge({"a": 1}, {"a": 2}) is None
    # the reference's leaf rule (utils/utils.py:345-349): a value that does not convert is kept AS GIVEN -- '0.5' against an int
    # default stays the string (int('0.5') raises), it does not become 0; bool defaults read 'false' / 'True' in any case
    out = dict_merge({"max_epoch": 300, "lr": 1e-3, "flag": True, "axes": [1, 2], "name": "enet", "none": None},
                     {"max_epoch": "0.5", "lr": "0.01", "flag": "false", "axes": "[1, 2, 3]", "name": 7, "none": "x"}, True)
    assert out == {"max_epoch": "0.5", "lr": 0.01, "flag": False, "axes": [1, 2, 3], "name": "7", "none": "x"}
    assert dict_merge({"flag": False, "n": 3}, {"flag": "TRUE", "n": 4.0}, True) == {"flag": True, "n": 4}
    assert dict_merge({"flag": False}, {"flag": "no_such_name"}, True) == {"flag": "no_such_name"}
    # the trainer's use: per-model report dictionaries merged leaf by leaf (cotraining_totalloss._report_dict)
    assert dict_merge({"S0": {"DSC1": 0.5}}, {"S0": {"DSC": 0.25}}, True) == {"S0": {"DSC1": 0.5, "DSC": 0.25}}


def test_tensor_predicates():
    from dct_amd.utils import class2one_hot, one_hot, probs2one_hot, simplex, sset, uniq
    p = torch.softmax(torch.randn(2, 3, 5, 4), 1)
    assert simplex(p) and not simplex(p * 2)
    oh = probs2one_hot(p)
    assert oh.shape == p.shape and one_hot(oh) and oh.dtype == torch.int32
    seg = torch.randint(0, 3, (5, 4))
    assert class2one_hot(seg, 3).shape == (1, 3, 5, 4) and uniq(seg) <= {0, 1, 2} and sset(seg, range(3))
    assert torch.equal(class2one_hot(seg, 3)[0].argmax(0), seg)


def test_arch_registry_names_match_reference_state_dict():
    from dct_amd.arch import get_arch
    net = get_arch("unet", {"num_classes": 4})
    o = oracle.build_net("unet", 4)
    assert list(net.state_dict()) == list(o.state_dict())
    assert all(net.state_dict()[k].shape == v.shape for k, v in o.state_dict().items())
    with pytest.raises(AssertionError):
        get_arch("fcn8", {"num_classes": 4})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 1, 176, 176))                      # product path never computes on the CPU


def test_flat_params_survive_reallocation():
    from dct_amd.arch import get_arch
    net = get_arch("unet", {"num_classes": 2})
    fp = net.flat_params
    assert fp.ensure() and fp.is_flat() and not fp.ensure()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    w = net.dec2.down.at(0).weight
    assert w.shape == (128, 64, 3, 3) and w.stride() == (576, 1, 192, 64)      # logical OIHW, physical [O][kh][kw][I]
    assert net.center.at(5).weight.shape == (1024, 512, 2, 2)                   # ConvTranspose2d layout
    assert fp.total % 64 == 0 and fp.total >= sum(p.numel() for p in net.parameters())
    net.double().float()                                                        # re-allocates every parameter
    assert not fp.is_flat() and fp.ensure()
    assert all(torch.equal(net.state_dict()[k], v) for k, v in before.items())
    assert fp.ensure_grads() and fp.grads_attached()
    assert w.grad.data_ptr() == fp.gflat.data_ptr() + 4 * fp.offsets[[id(p) for p in fp.params].index(id(w))]
    net.zero_grad()                                                             # set_to_none detaches
    assert not fp.grads_attached()
    sd = oracle.build_net("unet", 2).state_dict()
    net.load_state_dict(sd)
    assert fp.is_flat() and torch.equal(net.final.weight.detach(), sd["final.weight"])


def test_dropout_seed_follows_torch_seed_and_differs_between_models():
    """co-trained models must not share dropout masks; a user seed controls them."""
    from dct_amd.arch import get_arch
    torch.manual_seed(7)
    a, b = get_arch("unet", {"num_classes": 4}), get_arch("unet", {"num_classes": 4})
    torch.manual_seed(7)
    c = get_arch("unet", {"num_classes": 4})
    assert a.dropout_seed != b.dropout_seed
    assert a.dropout_seed == c.dropout_seed
    assert 0 <= a.dropout_seed < 2 ** 62


def test_fused_adam_load_state_dict_takes_the_loaded_step():
    """restoring a checkpoint into an optimizer that already stepped further must take the loaded step count
    (torch.optim.Adam does), not the larger one."""
    from dct_amd.arch import get_arch
    from dct_amd.optim import FusedAdam
    net = get_arch("enet", {"num_classes": 2})
    opt = FusedAdam(net.parameters(), flat=net.flat_params, lr=1e-3)
    opt._ensure_state()
    opt._steps = 5
    sd = copy.deepcopy(opt.state_dict())
    assert all(int(float(st["step"])) == 5 for st in sd["state"].values())
    opt._steps = 40                       # trained on ...
    opt._state_views()
    opt.load_state_dict(sd)               # ... then restored
    opt._ensure_state()
    assert opt._steps == 5
    assert all(int(float(st["step"])) == 5 for st in opt.state_dict()["state"].values())


def test_run_step_normalises_loader_dtypes(tmp_path, monkeypatch):
    """uint8 / int32 labels and double images from a loader are cast once at the step boundary."""
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", 2, 16, 2, 1)
    for s in tr.segmentators:
        s.train()
    lb = []
    for i in range(2):
        img, gt = lab[i][0][0]
        lb.append((img.double(), gt.to(torch.uint8)))
    seen = {}
    orig = tr._run_step_generic

    def spy(lab_, unl_, *a):
        seen["lab"] = [(x.dtype, y.dtype, x.is_contiguous()) for x, y in lab_]
        seen["unl"] = unl_[0].dtype
        return orig(lab_, unl_, *a)
    tr._run_step_generic = spy
    out = tr._run_step(lb, (unl[0][0][0].half(), unl[0][0][1].int()), True, False)
    assert seen["lab"] == [(torch.float32, torch.int64, True)] * 2 and seen["unl"] == torch.float32
    assert all(torch.isfinite(s) for s in out["sup"])


def test_step_scheduling_switches_on_cpu_modules(tmp_path, monkeypatch):
    """The scheduling switches are HIP-path decisions: with plain nn.Modules on the CPU the generic step runs, no layout is
    chosen and no stream is created, whatever the switches say (trainer/stream_sched.py is imported but idle)."""
    from dct_amd.trainer.stream_sched import EagerSchedule
    tr, lab, unl = _make_trainer(tmp_path, monkeypatch, "enet", 2, 32, 2, 2)
    for s in tr.segmentators:
        s.train()
    assert isinstance(tr._sched, EagerSchedule) and tr._sched.capturing is False
    assert tr.segmented_graphs is None and tr._use_segments() is False             # oracle modules do not ask for segments
    tr.segmented_graphs = True
    assert tr._use_segments() is True
    tr.segmented_graphs = None
    lb = [(lab[i][0][0][0], lab[i][0][0][1]) for i in range(2)]
    np.random.seed(3)
    tr._run_step(lb, (unl[0][0][0], unl[0][0][1]), True, True, (0, 1))
    assert tr._step_hint_adv_chain is False        # needs batch-independent HIP networks with gradient overwrite
    assert tr._streams() is None and tr._stream_dealer() is None and tr._step_graphs is None
    # the eager schedule's null stream is a no-op context
    with tr._sched.on(None):
        pass
    tr._sched.wait([])
    seen = []
    tr._sched.call(lambda: seen.append(1))
    assert seen == [1]


# ---- the step's route (trainer/step_route.py).  Expected values: the predicates of the step as they stood when every layout asked for itself
# (_fused_ok, graphable / segmented, _use_segments, fuse, _wide_ok, _group_passes_ok, _adv_chain_ok, the early-backward condition, the three
# unions of the overwrite set, and _capture's pass_streams = False / grad_sync = None / _defer_optimizer = True around a one-graph capture).
def _route_kit():
    from dct_amd.trainer.cotraining_totalloss import ExecutionPlan
    from dct_amd.trainer.step_route import NetFacts, StepFacts
    unet = NetFacts(plan_net=True, batch_independent=True, supports_grad_overwrite=True, supports_forward_reuse=True, grad_buckets=True, training=True, grads_attached=True)
    enet = NetFacts(plan_net=True, supports_pass_streams=True, supports_deferred_running_stats=True, supports_pass_groups=True, prefers_segmented_graphs=True, training=True,
                    grads_attached=True)

    def facts(net, S=2, adv=None, **kw):
        base = dict(S=S, nets=(net,) * S, train_jsd=True, train_adv=adv is not None, adv_choice=adv, unlabeled=True, labeled_shapes_equal=True,
                    labeled_equals_unlabeled=False, labeled_pixels=2 * 64 * 64, gpu=True, fused_criteria=True, optimizers_graphable=True, group_max=4)
        base.update(kw)
        return StepFacts(**base)
    return ExecutionPlan, unet, enet, facts


def _no_probe():
    raise AssertionError("the hardware-queue probe was asked")


def test_step_route_table():
    import dataclasses as dc
    from dct_amd.trainer.step_route import plan_execution, plan_step
    Plan, unet, enet, facts = _route_kit()
    yes, no = (lambda: True), (lambda: False)
    # 1. 2 x UNet, JSD only: one graph, sequential, joint pass, no pass streams
    f = facts(unet)
    assert plan_execution(Plan(), f) == "one_graph"
    r = plan_step(Plan(), f, "one_graph", _no_probe)
    assert (r.kind, r.joint_pass, r.model_streams, any(r.pass_streams), any(r.early_backward)) == ("sequential", True, True, False, False)
    assert r.overwrite == ("first", "first") and r.exchange == ("none", "none") and not r.defer_optimizer and not r.adv_chain_eligible
    assert plan_step(Plan(), f, "eager", _no_probe) == r                      # UNet has no layout that needs four queues without FGSM
    # 2. 2 x UNet + FGSM, pair (0, 1): a program; the adversarial chain layout with four queues, else sequential
    f = facts(unet, adv=(0, 1))
    assert plan_execution(Plan(), f) == "program"
    r = plan_step(Plan(), f, "program", yes)
    assert (r.kind, r.adv_chain_eligible, r.joint_pass, r.share_fgsm_encoder, r.late_b) == ("adv_chain", True, True, True, 2)
    assert r.overwrite == ("first", "first") and not any(r.pass_streams)
    r = plan_step(Plan(), f, "program", no)
    assert (r.kind, r.adv_chain_eligible, r.joint_pass, r.share_fgsm_encoder, r.late_b) == ("sequential", True, True, False, 0)
    assert plan_step(Plan(), f, "eager", yes).kind == "adv_chain"
    assert plan_step(Plan(), f, "one_graph", _no_probe).kind == "sequential"       # (segmented_graphs=False: joins into forked streams stay out of ONE graph)
    assert plan_step(Plan(adv_chain_late_b=1), f, "program", yes).late_b == 1 and plan_step(Plan(adv_chain_late_b=0), f, "program", yes).late_b == 0
    assert not plan_step(Plan(), dc.replace(f, nets=(unet, dc.replace(unet, supports_forward_reuse=False))), "program", yes).share_fgsm_encoder
    # 3. ... not eligible: the same model twice, three models, data parallelism, external dropout masks (these also end the joint pass)
    masks = dc.replace(unet, dropout_masks_set=True)
    for g, joint in ((facts(unet, adv=(0, 0)), True), (facts(unet, S=3, adv=(0, 2)), True), (facts(unet, adv=(0, 1), ddp=True), True),
                     (facts(masks, adv=(0, 1)), False)):
        r = plan_step(Plan(), g, "program", _no_probe)
        assert (r.kind, r.adv_chain_eligible, r.joint_pass) == ("sequential", False, joint), g
        assert plan_execution(Plan(), g) == ("program" if g.ddp else "one_graph")
    # 4. 2 x UNet under data parallelism: a program with the buckets handed out of the backward pass; two graphs when segments are refused
    f = facts(unet, ddp=True)
    assert plan_execution(Plan(), f) == "program"
    r = plan_step(Plan(), f, "program", _no_probe)
    assert (r.kind, r.exchange, r.defer_optimizer, r.overwrite) == ("sequential", ("buckets", "buckets"), False, ("first", "first"))
    assert plan_execution(Plan(segmented_graphs=False), f) == "ddp_two_graphs"
    assert plan_execution(Plan(ddp_segmented_graph=False), f) == "eager"      # no capture holds a collective: without segments the step is launched
    assert plan_step(Plan(ddp_segmented_graph=False), f, "eager", _no_probe).exchange == ("buckets", "buckets")
    for plan in (Plan(segmented_graphs=False), Plan(ddp_segmented_graph=False)):
        r = plan_step(plan, f, "ddp_two_graphs", _no_probe)
        assert (r.kind, r.exchange, r.defer_optimizer, any(r.pass_streams)) == ("sequential", ("two_graphs", "two_graphs"), True, False)
    e = plan_step(Plan(segmented_graphs=False), facts(enet, adv=(0, 1), ddp=True), "ddp_two_graphs", _no_probe)
    assert (e.kind, e.exchange, e.defer_optimizer, any(e.pass_streams), e.overwrite) == ("sequential", ("two_graphs",) * 2, True, False, ("none",) * 2)
    assert plan_step(Plan(), facts(enet, adv=(0, 1), ddp=True), "program", yes).exchange == ("model", "model")
    # 5. 2 x Enet, JSD, with and without FGSM: a program, the grouped four-queue layout
    for adv in (None, (0, 1)):
        f = facts(enet, adv=adv)
        assert plan_execution(Plan(), f) == "program"
        r = plan_step(Plan(), f, "program", yes)
        assert (r.kind, r.joint_pass, r.group_one, r.leaf_offload) == ("wide_grouped", False, False, adv is not None)
        assert r.overwrite == ("buffers", "buffers") and all(r.pass_streams) and not any(r.early_backward)
        assert plan_step(Plan(), dc.replace(f, labeled_equals_unlabeled=True), "program", yes).group_one
        assert not plan_step(Plan(), dc.replace(f, labeled_equals_unlabeled=True, group_max=3), "program", yes).group_one       # 2 S > group_max
        assert plan_step(Plan(), dc.replace(f, group_max=1), "program", yes).kind == "wide"                                  # S > group_max
        assert not plan_step(Plan(), dc.replace(f, lam_adv_zero=True), "program", yes).leaf_offload
        for g, plan in ((f, Plan(group_passes=False)), (dc.replace(f, labeled_shapes_equal=False), Plan())):
            r = plan_step(plan, g, "program", yes)
            assert (r.kind, r.group_one, r.leaf_offload, r.overwrite) == ("wide", False, False, ("buffers", "buffers"))
    # 6. 2 x Enet, segmented_graphs=False: ONE graph holds the sequential step without pass streams; its warm-up steps stay wide
    f = facts(enet, adv=(0, 1))
    assert plan_execution(Plan(segmented_graphs=False), f) == "one_graph"
    r = plan_step(Plan(segmented_graphs=False), f, "one_graph", _no_probe)
    assert (r.kind, any(r.pass_streams), any(r.early_backward), r.overwrite, r.model_streams) == ("sequential", False, False, ("none", "none"), True)
    assert plan_step(Plan(segmented_graphs=False), f, "eager", yes).kind == "wide_grouped"
    # 7. 2 x Enet without four queues: sequential, pass streams, the co-training backward passes beside the adversarial block
    r = plan_step(Plan(), f, "program", no)
    assert (r.kind, r.pass_streams, r.early_backward, r.overwrite) == ("sequential", (True, True), (True, True), ("buffers", "buffers"))
    r = plan_step(Plan(), facts(enet), "program", no)                           # no FGSM: nothing to run beside; two passes per model, in parallel
    assert (r.kind, r.pass_streams, r.early_backward, r.overwrite) == ("sequential", (True, True), (False, False), ("buffers", "buffers"))
    r = plan_step(Plan(), facts(enet, lam_cot_zero=True), "program", no)        # one pass per model: nothing to run in parallel
    assert (r.pass_streams, r.overwrite) == ((True, True), ("none", "none"))
    cold = dc.replace(enet, grads_attached=False)                               # first step: no gradient buffer yet
    r = plan_step(Plan(), facts(cold, adv=(0, 1)), "eager", _no_probe)
    assert (r.kind, r.early_backward, r.overwrite) == ("sequential", (False, False), ("none", "none"))
    # 8. UNet with BatchNorm: the samples of a pass interact -- no joint pass, no adversarial chain
    bn = dc.replace(unet, batch_independent=False)
    r = plan_step(Plan(), facts(bn, adv=(0, 1)), "one_graph", _no_probe)
    assert (r.kind, r.joint_pass, r.adv_chain_eligible, r.overwrite) == ("sequential", False, False, ("first", "first"))
    assert plan_execution(Plan(), facts(bn, adv=(0, 1))) == "one_graph"
    # 9. a network in eval mode, an optimizer that cannot be replayed, use_hip_graph off: launched eagerly
    for net in (unet, enet):
        assert plan_execution(Plan(), facts(net, nets=(net, dc.replace(net, training=False)))) == "eager"
        assert plan_execution(Plan(), facts(net, optimizers_graphable=False)) == "eager"
        assert plan_execution(Plan(use_hip_graph=False), facts(net)) == "eager"
    assert plan_step(Plan(), facts(enet, nets=(enet, dc.replace(enet, training=False))), "eager", _no_probe).kind == "sequential"
    # 10. CPU device, other criteria, plain modules, nine models: the generic step; the probe is never asked
    from dct_amd.trainer.step_route import NetFacts
    for g in (facts(enet, gpu=False), facts(enet, fused_criteria=False), facts(NetFacts(), adv=(0, 1)), facts(unet, S=9)):
        assert plan_execution(Plan(), g) == "generic"
        r = plan_step(Plan(), g, "eager", _no_probe)
        assert (r.kind, r.joint_pass, r.model_streams, any(r.pass_streams), r.overwrite, r.loss_scale) == ("sequential", False, False, False, ("none",) * g.S, 1.0)
    assert plan_step(Plan(), facts(NetFacts(), ddp=True), "eager", _no_probe).exchange == ("model", "model")
    # the fp16 loss scale: a power of two >= the labeled pixel count, within [2^10, 2^24]; forced by the plan
    half = dc.replace(enet, fp16=True)
    assert plan_step(Plan(), facts(half), "eager", no).loss_scale == 2.0 ** 13 and plan_step(Plan(), facts(enet), "eager", no).loss_scale == 1.0
    assert plan_step(Plan(), facts(half, labeled_pixels=100), "eager", no).loss_scale == 2.0 ** 10
    assert plan_step(Plan(), facts(half, labeled_pixels=1 << 30), "eager", no).loss_scale == 2.0 ** 24
    assert plan_step(Plan(force_loss_scale=4.0), facts(enet), "eager", no).loss_scale == 4.0


def test_step_route_each_switch_governs_its_own_fields():
    """Every ExecutionPlan switch turned off alone: the route fields that differ from the default route's, per configuration."""
    import dataclasses as dc
    from dct_amd.trainer.step_route import plan_execution, plan_step
    Plan, unet, enet, facts = _route_kit()

    def changed(f, mode, queues=True, **switch):
        base, r = plan_step(Plan(), f, mode, lambda: queues), plan_step(Plan(**switch), f, mode, lambda: queues)
        return {k: getattr(r, k) for k in (fl.name for fl in dc.fields(r)) if getattr(r, k) != getattr(base, k)}
    e_adv, u_adv, u = facts(enet, adv=(0, 1)), facts(unet, adv=(0, 1)), facts(unet)
    # 2 x Enet + FGSM on four queues (wide_grouped, leaf offload on)
    assert changed(e_adv, "program", leaf_offload=False) == dict(leaf_offload=False)
    assert changed(e_adv, "program", group_passes=False) == dict(kind="wide", leaf_offload=False)
    assert changed(dc.replace(e_adv, labeled_equals_unlabeled=True), "program", group_one=False) == dict(group_one=False)
    assert changed(e_adv, "program", wide_forward=False) == dict(kind="sequential", early_backward=(True, True), leaf_offload=False)
    assert changed(e_adv, "program", pass_streams=False) == dict(kind="sequential", pass_streams=(False, False), leaf_offload=False, overwrite=("none", "none"))
    assert changed(e_adv, "program", model_streams=False) == dict(kind="sequential", model_streams=False, pass_streams=(False, False), leaf_offload=False,
                                                                  overwrite=("none", "none"))
    for name in ("early_backward", "grad_overwrite", "adv_chain_layout", "batch_lab_unlab", "spread_streams", "segmented_graphs", "use_hip_graph",
                 "ddp_segmented_graph", "fgsm_shares_encoder", "adv_chain_late_b"):
        assert changed(e_adv, "program", **{name: False}) == {}, name
    # ... without four queues (sequential, pass streams, early backward)
    assert changed(e_adv, "program", queues=False, early_backward=False) == dict(early_backward=(False, False))
    assert changed(e_adv, "program", queues=False, pass_streams=False) == dict(pass_streams=(False, False), early_backward=(False, False), overwrite=("none", "none"))
    for name in ("wide_forward", "group_passes", "group_one", "leaf_offload", "grad_overwrite"):
        assert changed(e_adv, "program", queues=False, **{name: False}) == {}, name
    # 2 x UNet + FGSM on four queues (adv_chain)
    seq = dict(kind="sequential", share_fgsm_encoder=False, late_b=0)
    assert changed(u_adv, "program", adv_chain_layout=False) == dict(seq, adv_chain_eligible=False)
    assert changed(u_adv, "program", model_streams=False) == dict(seq, adv_chain_eligible=False, model_streams=False)
    assert changed(u_adv, "program", batch_lab_unlab=False) == dict(seq, adv_chain_eligible=False, joint_pass=False)
    assert changed(u_adv, "program", grad_overwrite=False) == dict(seq, overwrite=("none", "none"))
    assert changed(u_adv, "program", fgsm_shares_encoder=False) == dict(share_fgsm_encoder=False)
    assert changed(u_adv, "program", adv_chain_late_b=1) == dict(late_b=1)
    for name in ("pass_streams", "early_backward", "wide_forward", "group_passes", "group_one", "leaf_offload", "spread_streams"):
        assert changed(u_adv, "program", **{name: False}) == {}, name
    # 2 x UNet, JSD only, inside one graph
    assert changed(u, "one_graph", batch_lab_unlab=False) == dict(joint_pass=False)
    assert changed(u, "one_graph", grad_overwrite=False) == dict(overwrite=("none", "none"))
    assert changed(u, "one_graph", model_streams=False) == dict(model_streams=False)
    assert changed(u, "one_graph", force_loss_scale=8.0) == dict(loss_scale=8.0)
    # the switches that govern the replay, not the layout
    assert plan_execution(Plan(use_hip_graph=False), u_adv) == "eager" and plan_execution(Plan(adv_chain_layout=False), u_adv) == "one_graph"
    assert plan_execution(Plan(segmented_graphs=True), u) == "program" and plan_execution(Plan(segmented_graphs=False), e_adv) == "one_graph"
    assert plan_execution(Plan(model_streams=False), u_adv) == "one_graph" and plan_execution(Plan(batch_lab_unlab=False), u_adv) == "one_graph"


# ---- the UNet pass's route (arch/unet_route.py).  Expected values: the predicates of UNet._run_forward / _run_backward as they stood when the
# two read the switches as they went, restated here with every "x is (not) None" test as a boolean.
_UNET_FWD = ("relu_bits", "pool_codes", "fuse_pool", "pool_only", "fuse_drop_pool", "batch_skip_resize", "late_packs", "save", "keep_predrop",
             "reuse_offered", "net_training", "dropout_on", "batchnorm", "masks_external", "masks_recorded", "debug")
_UNET_BWD = ("fuse_skip_grad", "fuse_stem_wgrad", "batch_bias_grads", "wgrad_side_stream", "need_dx", "need_dw", "overwrite", "bf16", "batchnorm",
             "debug", "grad_hook_set")


def _unet_forward_as_it_stood(relu_bits, pool_codes, fuse_pool, pool_only, fuse_drop_pool, batch_skip_resize, late_packs, save, keep_predrop,
                              reuse_offered, net_training, dropout_on, batchnorm, masks_external, masks_recorded, debug):
    """-> (the route's fields, "pc1..4 are all in the tape")."""
    external_is_none, masks_out_is_none, debug_is_none = not masks_external, not masks_recorded, not debug
    training = net_training and dropout_on
    reuse = bool(reuse_offered and (training and not batchnorm and external_is_none and masks_out_is_none and debug_is_none))
    pool, codes_kept, d4pre = [], [], False
    for lvl in (1, 2, 3, 4):
        if reuse:                                   # levels 1-3 from the tape (whose pc1..3 the offer checked); level 4: dropout + pool, codes always
            pool.append("reused" if lvl < 4 else "dropout_pool")
            codes_kept.append(True)
            continue
        codes = bool(save and pool_codes)           # "codes is not None"
        fuse = fuse_pool and not (lvl == 4 and (training or not external_is_none))
        only = fuse and pool_only and (codes or not save) and debug_is_none
        drop_pool = (lvl == 4 and not fuse and training and fuse_drop_pool and external_is_none and masks_out_is_none
                     and codes and debug_is_none)
        if drop_pool and keep_predrop and save:
            d4pre = True
        pool.append("conv_only" if only else "conv" if fuse else "dropout_pool" if drop_pool else "separate")
        codes_kept.append(codes)
    drop = "external" if not external_is_none else ("device" if training else "none")     # dropout(): the masks first, then "if not training"
    fields = dict(training=training, drop=drop, scale_by_keep=bool(training or not external_is_none), keep_bits=bool(save and relu_bits),
                  keep_codes=bool(save and pool_codes), reuse=reuse, pool=tuple(pool), keep_d4pre=d4pre, batch_skip_resize=batch_skip_resize,
                  late_packs=late_packs)
    return fields, all(codes_kept)


def _unet_backward_as_it_stood(codes_on_every_level, fuse_skip_grad, fuse_stem_wgrad, batch_bias_grads, wgrad_side_stream, need_dx, need_dw,
                               overwrite, bf16, batchnorm, debug, grad_hook_set):
    side_is_none = not (need_dw and wgrad_side_stream)              # side = self._side_stream(dev) if need_dw else None
    hook_is_none = not (need_dw and grad_hook_set)                  # hook = self._grad_hook if need_dw else None
    return dict(side_stream=not side_is_none, accumulate=not (overwrite and need_dw), bias_in_wgrad=bf16,
                skip_fused=bool(fuse_skip_grad and codes_on_every_level),
                try_stem_fusion=bool(need_dw and not need_dx and fuse_stem_wgrad and bf16 and side_is_none and not batchnorm and not debug),
                bucket_hooks=not hook_is_none and side_is_none, batch_bias_grads=batch_bias_grads)


def test_unet_route_table():
    import dataclasses as dc
    import itertools
    from dct_amd.arch.unet_route import BackwardFacts, ForwardFacts, plan_backward_pass, plan_forward_pass
    assert tuple(f.name for f in dc.fields(ForwardFacts)) == _UNET_FWD and tuple(f.name for f in dc.fields(BackwardFacts))[1:] == _UNET_BWD
    # every forward row: 2^16
    routes = {}
    for row in itertools.product((False, True), repeat=len(_UNET_FWD)):
        r = plan_forward_pass(ForwardFacts(*row))
        want, codes = _unet_forward_as_it_stood(*row)
        assert dc.asdict(r) == want, dict(zip(_UNET_FWD, row))
        assert routes.setdefault(r, codes) == codes, r        # (what the backward pass needs to know of the codes is in the route)
    # every backward row, 2^11, over forward routes of both kinds (codes on every level or not), with and without a shared encoder;
    # then every distinct forward route under the default backward facts and each single flip of them
    some = sorted(routes, key=repr)[::max(1, len(routes) // 48)]
    assert {routes[r] for r in some} == {False, True} and {r.reuse for r in some} == {False, True}
    for fwd in some:
        for row in itertools.product((False, True), repeat=len(_UNET_BWD)):
            assert dc.asdict(plan_backward_pass(BackwardFacts(fwd, *row))) == _unet_backward_as_it_stood(routes[fwd], *row), (fwd, row)
    base = BackwardFacts(None)
    flips = [{}] + [{k: not getattr(base, k)} for k in _UNET_BWD]
    for fwd, codes in routes.items():
        for flip in flips:
            f = dc.replace(base, forward=fwd, **flip)
            assert dc.asdict(plan_backward_pass(f)) == _unet_backward_as_it_stood(codes, *dc.astuple(f)[1:]), (fwd, flip)
    # named rows.  The benchmarked training pass (cfg2 / cfg3: bf16, train mode, p = 0.5, every switch at its default)
    for keep in (False, True):
        r = plan_forward_pass(ForwardFacts(keep_predrop=keep))
        assert r.pool == ("conv_only", "conv_only", "conv_only", "dropout_pool") and r.keep_d4pre == keep
        assert (r.training, r.drop, r.scale_by_keep, r.keep_bits, r.keep_codes, r.reuse) == (True, "device", True, True, True, False)
    b = plan_backward_pass(BackwardFacts(r, overwrite=True))
    assert (b.skip_fused, b.try_stem_fusion, b.bias_in_wgrad, b.accumulate, b.side_stream, b.bucket_hooks) == (True, True, True, False, False, False)
    # ... its second pass over the same input, handed the first one's tape
    r = plan_forward_pass(ForwardFacts(reuse_offered=True, keep_predrop=True))
    assert r.reuse and r.pool == ("reused", "reused", "reused", "dropout_pool") and not r.keep_d4pre
    for refusal in ("batchnorm", "masks_external", "masks_recorded", "debug"):
        assert not plan_forward_pass(ForwardFacts(reuse_offered=True, **{refusal: True})).reuse
    assert not plan_forward_pass(ForwardFacts(reuse_offered=True, net_training=False)).reuse
    # an eval pass that saves nothing
    r = plan_forward_pass(ForwardFacts(net_training=False, save=False))
    assert r.pool == ("conv_only",) * 4 and (r.drop, r.scale_by_keep, r.keep_bits, r.keep_codes) == ("none", False, False, False)
    # recorded masks, external masks: the fourth level's dropout is a launch of its own
    r = plan_forward_pass(ForwardFacts(masks_recorded=True))
    assert r.pool == ("conv_only", "conv_only", "conv_only", "separate") and r.drop == "device"
    r = plan_forward_pass(ForwardFacts(masks_external=True))
    assert r.pool[3] == "separate" and r.drop == "external" and r.scale_by_keep
    assert plan_forward_pass(ForwardFacts(masks_external=True, net_training=False)).drop == "external"
    # fp32 backward; the side stream
    fwd = plan_forward_pass(ForwardFacts())
    b = plan_backward_pass(BackwardFacts(fwd, bf16=False))
    assert not b.try_stem_fusion and not b.bias_in_wgrad
    b = plan_backward_pass(BackwardFacts(fwd, wgrad_side_stream=True, grad_hook_set=True))
    assert b.side_stream and not b.try_stem_fusion and not b.bucket_hooks
    assert plan_backward_pass(BackwardFacts(fwd, grad_hook_set=True)).bucket_hooks
    assert not plan_backward_pass(BackwardFacts(fwd, wgrad_side_stream=True, need_dw=False)).side_stream


def test_unet_route_each_switch_governs_its_own_fields():
    """Every UNet switch flipped alone: the route fields that differ from the default route's."""
    import dataclasses as dc
    from dct_amd.arch.unet_route import BackwardFacts, ForwardFacts, plan_backward_pass, plan_forward_pass

    def diff(r, base):
        return {f.name: getattr(r, f.name) for f in dc.fields(r) if getattr(r, f.name) != getattr(base, f.name)}

    def changed(base_facts=ForwardFacts(), back=None, **switch):
        """-> (forward fields, backward fields) that a switch of either pass changes."""
        fwd_sw = {k: v for k, v in switch.items() if k in _UNET_FWD}
        bwd_sw = {k: v for k, v in switch.items() if k not in fwd_sw}
        f0, f1 = plan_forward_pass(base_facts), plan_forward_pass(dc.replace(base_facts, **fwd_sw))
        b0, b1 = plan_backward_pass(BackwardFacts(f0, **(back or {}))), plan_backward_pass(BackwardFacts(f1, **dict(back or {}, **bwd_sw)))
        return diff(f1, f0), diff(b1, b0)
    # a training pass that saves (default pools: conv_only x 3, dropout_pool)
    assert changed(relu_bits=False) == (dict(keep_bits=False), {})
    assert changed(pool_codes=False) == (dict(keep_codes=False, pool=("conv", "conv", "conv", "separate")), dict(skip_fused=False))
    assert changed(fuse_pool=False) == (dict(pool=("separate", "separate", "separate", "dropout_pool")), {})
    assert changed(pool_only=False) == (dict(pool=("conv", "conv", "conv", "dropout_pool")), {})
    assert changed(fuse_drop_pool=False) == (dict(pool=("conv_only", "conv_only", "conv_only", "separate")), {})
    assert changed(batch_skip_resize=False) == (dict(batch_skip_resize=False), {})
    assert changed(late_packs=False) == (dict(late_packs=False), {})
    assert changed(fuse_skip_grad=False) == ({}, dict(skip_fused=False))
    assert changed(fuse_stem_wgrad=False) == ({}, dict(try_stem_fusion=False))
    assert changed(batch_bias_grads=False) == ({}, dict(batch_bias_grads=False))
    assert changed(wgrad_side_stream=True) == ({}, dict(side_stream=True, try_stem_fusion=False))
    assert changed(back=dict(grad_hook_set=True), wgrad_side_stream=True) == ({}, dict(side_stream=True, try_stem_fusion=False, bucket_hooks=False))
    assert changed(back=dict(need_dw=False), wgrad_side_stream=True) == ({}, {})
    # an eval pass (all four pools ride in their convolutions): the dropout + pool switch governs nothing
    ev = ForwardFacts(net_training=False)
    assert changed(ev, fuse_drop_pool=False) == ({}, {})
    assert changed(ev, fuse_pool=False) == (dict(pool=("separate",) * 4), {})
    assert changed(ev, pool_only=False) == (dict(pool=("conv",) * 4), {})
    assert changed(ev, pool_codes=False) == (dict(keep_codes=False, pool=("conv",) * 4), dict(skip_fused=False))
    # ... that saves nothing: no codes to keep, nothing for the backward pass to need
    assert changed(dc.replace(ev, save=False), pool_codes=False) == ({}, {}) and changed(dc.replace(ev, save=False), relu_bits=False) == ({}, {})
    # a pass over a shared encoder: only what lies behind the first dropout can still be switched
    sh = ForwardFacts(reuse_offered=True)
    for name in ("fuse_pool", "pool_only", "fuse_drop_pool"):
        assert changed(sh, **{name: False}) == ({}, {}), name
    assert changed(sh, pool_codes=False) == (dict(keep_codes=False), {})          # (the tape's codes and the dropout + pool launch's are there)


def test_refused_capture_filter_recognises_the_runtime_messages():
    """step_graph keeps a step shape on eager launches only for refused captures; the library's own launch errors propagate."""
    from dct_amd.trainer.step_graph import _is_refused_capture
    for msg in ("HIP error: operation not permitted when stream is capturing", "capturing stream has unjoined work",
                "operation would make the legacy stream depend on a capturing blocking stream", "hipGraphInstantiate failed"):
        assert _is_refused_capture(RuntimeError(msg)), msg
    for msg in ("dct_amd: dct_conv2d failed (DCT_ERR_BAD_ARG)", "shape mismatch", "dct_amd: dct_enet_conv failed (DCT_ERR_LAUNCH)"):
        assert not _is_refused_capture(RuntimeError(msg)), msg


def test_bench_dump_outputs_writes_the_step_arrays(tmp_path):
    """bench.py --dump-outputs: every array of the step's result as float32 .npy; above the byte limit a seeded sample that is the same
    from run to run and keeps the dump under the limit."""
    import json
    import bench
    g = torch.Generator().manual_seed(3)
    out = dict(sup=[torch.rand((), generator=g), torch.rand((), generator=g)], jsd=torch.rand((), generator=g), adv=0,
               preds=[torch.rand(2, 3, 64, 64, generator=g).bfloat16() for _ in range(2)],
               unlab_probs=[torch.rand(4, 3, 64, 64, generator=g) for _ in range(2)])
    full = tmp_path / "full"
    bench.dump_outputs(out, str(full))
    names = sorted(p.name for p in full.glob("*.npy"))
    assert names == sorted(f"{n}.npy" for n in ["adv", "jsd", "sup_0", "sup_1", "preds_0", "preds_1", "unlab_probs_0", "unlab_probs_1"])
    p0 = np.load(full / "preds_0.npy")
    assert p0.dtype == np.float32 and p0.shape == (2, 3, 64, 64)
    assert np.array_equal(p0, out["preds"][0].float().numpy())
    assert float(np.load(full / "adv.npy")) == 0.0 and float(np.load(full / "jsd.npy")) == float(out["jsd"])
    limit = (1 << 20) + 64 * 1024                   # room for 16 K float32 elements of the ~74 K returned
    cut = [tmp_path / "cut_a", tmp_path / "cut_b"]
    for d in cut:
        bench.dump_outputs(out, str(d), limit=limit)
    assert sum(p.stat().st_size for p in cut[0].glob("*.npy")) <= limit
    man = json.loads((cut[0] / "manifest.json").read_text())
    assert man["unlab_probs_1"]["sampled"] and man["unlab_probs_1"]["shape"] == [4, 3, 64, 64]
    u = np.load(cut[0] / "unlab_probs_1.npy")
    assert u.size == man["unlab_probs_1"]["elements"] < 4 * 3 * 64 * 64 and np.isin(u, out["unlab_probs"][1].numpy()).all()
    for p in cut[0].glob("*.npy"):
        assert np.array_equal(np.load(p), np.load(cut[1] / p.name))


def test_bench_plain_run_takes_no_step_behind_the_timed_regions():
    """bench.py without --full: measure() runs the W warm-up steps and the timed regions over the same step indices as with --full, hands the
    last timed step's outputs to --dump-outputs, and takes no further step, meter or profiler leg; --full runs them all after that."""
    import argparse
    import bench

    def run(full):
        calls, legs_run = [], []
        args = argparse.Namespace(warmup=2, steps=3, repeats=3, full=full, no_clock_probe=False, no_kernel_events=False)
        res = bench.measure(args, None, lambda i: calls.append(i) or {"i": i}, bench.DryLegs(), 0, 1, False,
                            meters_leg=lambda base: legs_run.append("meters") or 1.0, operand_leg=lambda: legs_run.append("operand") or {},
                            enter_event_leg=lambda: legs_run.append("events"), last_step=lambda out: legs_run.append(("dump", out["i"], len(calls))))
        return calls, legs_run, res
    calls, legs_run, res = run(False)
    assert calls == list(range(2 + 3 * 3)) and legs_run == [("dump", 10, 11)] and res["out"] == {"i": 10}
    assert res["prof"] is None and res["clock"] is None and res["meters_ms"] is None and res["operand_stats"] is None
    fcalls, flegs, fres = run(True)
    assert fcalls[:11] == calls and len(fcalls) == 11 + 3 + 3           # the clock leg's and the event leg's K steps
    assert flegs == [("dump", 10, 11), "meters", "operand", "events"] and fres["prof"] is not None and fres["out"] == {"i": 10}


# dct_conv2d_workspace_bytes for (B, Cin, H, W of the input, Cout), descriptor fields / planner knobs -> bytes.  The numbers were read from the
# library as it stood before dct_conv2d got its one planner (plan_conv, csrc/igemm.hip), whose largest need over the routes this query returns.
_CONV_WS_KNOBS = {"IGEMM_SPLIT": (1, -1), "IGEMM_HALO": (7, 1), "IGEMM_PACKED": (10, 1), "IGEMM_SPLIT_TARGET": (16, 450), "IGEMM_PACKED_SPLIT": (23, 160),
                  "IGEMM_PACKED_FILL": (24, 50), "SPLIT_MAX_TILES": (1002, 96), "SPLIT_MIN_KITERS": (1003, 4)}      # name -> (knob, shipped value)
_CONV_WS_TABLE = [
    # per-tap, bf16: the split-K edges (tile-count threshold, K-step floor, forced factors, 2x2 stride 2)
    ((2, 320, 12, 12, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0), 819200),
    ((2, 320, 12, 12, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, IGEMM_SPLIT=2), 204800),
    ((2, 320, 12, 12, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, IGEMM_SPLIT=4), 409600),
    ((2, 320, 12, 12, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, IGEMM_SPLIT=7), 716800),
    ((1, 192, 14, 14, 64), dict(IGEMM_HALO=0, IGEMM_PACKED=0, pad=1, IGEMM_SPLIT=5), 250880),
    ((1, 64, 97, 130, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0), 12451840),
    ((1, 64, 98, 130, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0), 0),
    ((1, 64, 97, 130, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, SPLIT_MAX_TILES=95), 0),
    ((1, 64, 98, 130, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, SPLIT_MAX_TILES=97), 12582912),
    ((1, 192, 10, 10, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, R=1), 0),
    ((1, 448, 10, 10, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, R=1), 0),
    ((1, 512, 10, 10, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, R=1), 102400),
    ((1, 448, 10, 10, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, R=1, SPLIT_MIN_KITERS=1), 0),
    ((1, 512, 10, 10, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, R=1, SPLIT_MIN_KITERS=9), 0),
    ((2, 128, 20, 18, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, R=2, stride=2, IGEMM_SPLIT=3), 276480),
    ((2, 320, 12, 12, 128), dict(IGEMM_HALO=0, IGEMM_PACKED=0, IGEMM_SPLIT_TARGET=256), 819200),
    # per-tap, fp32
    ((1, 272, 12, 12, 64), dict(dtype=0), 409600),
    ((1, 256, 12, 12, 128), dict(dtype=0), 819200),
    ((1, 144, 12, 12, 64), dict(dtype=0), 358400),
    ((2, 64, 40, 40, 128), dict(dtype=0), 13307904),
    ((2, 32, 30, 30, 64), dict(dtype=0, IGEMM_SPLIT=11), 3612672),
    ((2, 64, 258, 258, 64), dict(dtype=0), 0),
    # shared halo: no workspace; with the stem's weight gradient one record per patch and the fold's scratch -- also where the layer
    # cannot take it (the call then fails before it looks at the workspace)
    ((8, 64, 254, 254, 64), dict(), 0),
    ((4, 128, 83, 147, 128), dict(), 0),
    ((3, 192, 98, 130, 256), dict(), 0),
    ((16, 64, 258, 258, 64), dict(), 0),
    ((8, 64, 254, 254, 64), dict(pad=2, stem=1), 10813440),
    ((8, 64, 198, 198, 64), dict(pad=2, stem=1), 6983680),
    ((4, 128, 83, 147, 128), dict(stem=1), 1454080),
    ((2, 64, 12, 12, 64), dict(stem=1), 337920),
    ((2, 64, 12, 12, 64), dict(stem=1, dtype=0), 460800),
    # packed rows: channel-slice splits, beside a split or an unsplit per-tap plan (the larger need counts), and the knobs that move them
    ((100, 576, 13, 13, 128), dict(), 30976000),
    ((60, 896, 13, 13, 128), dict(), 29736960),
    ((40, 1024, 13, 13, 256), dict(), 29736960),
    ((20, 704, 27, 27, 128), dict(), 12800000),
    ((16, 1024, 11, 11, 1024), dict(), 26542080),
    ((16, 1024, 11, 11, 1024), dict(IGEMM_PACKED=0), 26542080),
    ((16, 1024, 11, 11, 1024), dict(IGEMM_HALO=0), 26542080),
    ((8, 512, 29, 29, 512), dict(), 0),
    ((8, 512, 29, 29, 512), dict(IGEMM_PACKED_SPLIT=400), 23887872),
    ((8, 512, 29, 29, 512), dict(IGEMM_PACKED_SPLIT=100), 0),
    ((8, 1024, 11, 11, 1024), dict(), 21233664),
    ((8, 1024, 11, 11, 1024), dict(IGEMM_PACKED_FILL=76), 21233664),
    ((8, 1024, 11, 11, 1024), dict(IGEMM_SPLIT=2), 10616832),
    ((2, 320, 12, 12, 128), dict(), 819200),
    ((8, 256, 61, 61, 256), dict(), 0),
    ((8, 256, 61, 61, 256), dict(IGEMM_PACKED_FILL=100), 0),
    # the up-convolutions (2x2 scatter) and their data gradients
    ((8, 1024, 9, 9, 512), dict(R=1, scatter=1), 0),
    ((8, 128, 84, 84, 64), dict(R=1, scatter=1), 0),
    ((8, 512, 18, 18, 1024), dict(R=2, stride=2), 21233664),
    # channel counts no tile takes
    ((2, 16, 12, 12, 64), dict(), 0),
    ((2, 64, 12, 12, 32), dict(), 0),
    ((2, 8, 12, 12, 64), dict(dtype=0), 0),
]


def test_conv2d_workspace_bytes_table():
    """The planner's workspace size on every route and on both sides of the split edges.  The query reads shapes only: the views carry
    made-up pointers, and dct_conv2d itself is never called with them."""
    import ctypes as C
    from dct_amd import _lib
    lib = _lib.load()

    def ws(B, Cin, H, W, Cout, R=3, stride=1, pad=0, dtype=_lib.BF16, scatter=0, stem=0, **knobs):
        Ho, Wo = (2 * H, 2 * W) if scatter else ((H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1)
        x = _lib.View(4096, B, H, W, Cin, H * W * Cin, W * Cin, Cin)
        y = _lib.View(4096, B, Ho, Wo, Cout, Ho * Wo * Cout, Wo * Cout, Cout)
        d = _lib.ConvDesc(R, R, stride, 1, pad, pad, 0, scatter, 0, 0, 1.0, None, None, None, None, 0, 4096 if stem else None, None, None, 0)
        try:
            for k, v in knobs.items():
                assert lib.dct_tune_set(_CONV_WS_KNOBS[k][0], v) == 0, (k, v)
            return lib.dct_conv2d_workspace_bytes(C.byref(x), C.byref(y), C.byref(d), dtype)
        finally:
            for k in knobs:
                lib.dct_tune_set(*_CONV_WS_KNOBS[k])

    got = [(shape, kw, ws(*shape, **kw)) for shape, kw, _ in _CONV_WS_TABLE]
    assert got == _CONV_WS_TABLE, [(g, w[2]) for g, w in zip(got, _CONV_WS_TABLE) if g != w]
    assert sum(1 for _, _, n in _CONV_WS_TABLE if n) >= 30 and sum(1 for _, _, n in _CONV_WS_TABLE if not n) >= 15


# dct_conv2d_wgrad_workspace_bytes for (n, H, W, C of dy, C of x), descriptor fields / planner knobs -> bytes.  The numbers were read from the
# library built from the commit before dct_conv2d_wgrad got its one planner (plan_wgrad, csrc/wgrad.hip), never from the planner itself: the
# query returns 16 for a direct plan and counts the bias rows of every slab whether or not the call will ask for db.
_WGRAD_WS_KNOBS = {"WGRAD_CHUNKS": (3, -1), "WGRAD_ROWS": (8, 1), "WGRAD_ROWS_FILL": (9, 70), "WGRAD_TARGET": (14, 256), "WGRAD3_TARGET": (15, 768),
                   "LEAN": (38, 31)}      # name -> (knob, shipped value)
_WGRAD_WS_TABLE = [
    # per-tap (filter rows off, or not 3x3 stride 1): direct, natural and forced chunk counts, the 64-chunk and the 192 MiB caps, 2x2 stride 2
    ((2, 30, 30, 512, 512), dict(WGRAD_ROWS=0, WGRAD_CHUNKS=1), 16),
    ((8, 9, 9, 1024, 1024), dict(), 16),
    ((8, 9, 9, 1024, 1024), dict(WGRAD_ROWS_FILL=30), 16),
    ((3, 33, 29, 256, 256), dict(WGRAD_ROWS=0), 16522240),
    ((4, 60, 60, 128, 128), dict(WGRAD_ROWS=0), 14758400),
    ((2, 21, 23, 256, 256), dict(WGRAD_ROWS=0, WGRAD_CHUNKS=3), 7080960),
    ((2, 37, 41, 128, 128), dict(WGRAD_ROWS=0, WGRAD_CHUNKS=13), 7084032),
    ((8, 64, 64, 64, 64), dict(R=1), 1064960),
    ((8, 22, 22, 1024, 1024), dict(WGRAD_ROWS=0, WGRAD_TARGET=8192), 188764160),
    ((8, 22, 22, 1024, 1024), dict(WGRAD_ROWS=0), 16),
    ((4, 33, 35, 64, 128), dict(R=2, stride=2), 2495232),
    ((8, 18, 18, 1024, 512), dict(R=2, stride=2), 16785408),
    # filter-row, wide rows (the padded case runs the plain loop: its fill counts whole steps)
    ((2, 40, 130, 64, 64), dict(), 4431360),
    ((2, 40, 130, 64, 64), dict(WGRAD_ROWS=0), 4135936),
    ((3, 31, 200, 128, 64), dict(), 12407808),
    ((2, 33, 200, 64, 128), dict(pad=2), 9740544),
    ((3, 50, 130, 64, 64), dict(WGRAD_CHUNKS=11), 1624832),
    ((8, 256, 254, 64, 64), dict(), 18907136),
    ((8, 256, 254, 64, 64), dict(WGRAD3_TARGET=4096), 37814272),
    ((8, 126, 126, 128, 128), dict(), 18890752),
    # filter-row, narrow rows; the fill threshold from both sides
    ((5, 21, 20, 64, 64), dict(), 590848),
    ((4, 45, 48, 64, 64), dict(), 2954240),
    ((4, 45, 48, 64, 64), dict(WGRAD_CHUNKS=7), 1033984),
    ((8, 61, 61, 256, 256), dict(), 18882560),
    ((8, 40, 40, 64, 64), dict(), 3692800),
    ((8, 40, 40, 64, 64), dict(WGRAD_ROWS_FILL=30), 5908480),
    ((8, 40, 40, 64, 64), dict(WGRAD_ROWS_FILL=70), 3692800),
    # the loop form in the fill: 84-pixel rows are 88 % full counted in sub-steps (LEAN 31), 66 % in whole steps (14: no filter-row lean loop)
    ((4, 40, 84, 64, 64), dict(LEAN=31), 5908480),
    ((4, 40, 84, 64, 64), dict(LEAN=14), 3988224),
    ((4, 40, 84, 64, 64), dict(LEAN=15), 3988224),
    ((4, 40, 84, 64, 64), dict(pad=1), 3988224),
    ((2, 40, 130, 64, 64), dict(LEAN=14), 4135936),
    # the guards of the LDS-DMA kernels: rows of 2^29 elements per image, M < 2^24 pixels, 2^30 elements per tensor
    ((1, 2890, 2894, 64, 64), dict(), 18907136),
    ((1, 2898, 2898, 64, 64), dict(), 4135936),
    ((63, 510, 510, 64, 64), dict(), 18907136),
    ((65, 510, 510, 64, 64), dict(), 25258752),
    ((2, 1024, 1024, 512, 64), dict(), 50812928),
    # fp32
    ((2, 30, 30, 64, 64), dict(dtype=0), 2215680),
    ((2, 62, 62, 128, 128), dict(dtype=0), 36010496),
    ((4, 33, 35, 64, 128), dict(R=2, stride=2, dtype=0), 4859136),
    ((1, 7, 9, 64, 64), dict(dtype=0), 147712),
    # channel counts no tile takes
    ((2, 12, 12, 32, 64), dict(), 0),
    ((2, 12, 12, 64, 96), dict(), 0),
    ((2, 12, 12, 16, 64), dict(dtype=0), 0),
]


def test_conv2d_wgrad_workspace_bytes_table():
    """The weight-gradient planner's workspace size on every route and on both sides of its edges (chunk caps, forced chunks, the fill
    threshold and the loop form that enters it, the 32-bit guards).  The query reads shapes only: the views carry made-up pointers, and
    dct_conv2d_wgrad itself is never called with them."""
    import ctypes as C
    from dct_amd import _lib
    lib = _lib.load()

    def ws(n, Hp, Wp, Cp, Cq, R=3, stride=1, pad=0, dtype=_lib.BF16, **knobs):
        Hq, Wq = (Hp - 1) * stride + R - 2 * pad, (Wp - 1) * stride + R - 2 * pad
        p = _lib.View(4096, n, Hp, Wp, Cp, Hp * Wp * Cp, Wp * Cp, Cp)
        q = _lib.View(4096, n, Hq, Wq, Cq, Hq * Wq * Cq, Wq * Cq, Cq)
        d = _lib.ConvDesc(R, R, stride, 1, pad, pad, 0, 0, 0, 0, 1.0, None, None, None, None, 0, None, None, None, 0)
        try:
            for k, v in knobs.items():
                assert lib.dct_tune_set(_WGRAD_WS_KNOBS[k][0], v) == 0, (k, v)
            return lib.dct_conv2d_wgrad_workspace_bytes(C.byref(p), C.byref(q), C.byref(d), dtype)
        finally:
            for k in knobs:
                lib.dct_tune_set(*_WGRAD_WS_KNOBS[k])

    got = [(shape, kw, ws(*shape, **kw)) for shape, kw, _ in _WGRAD_WS_TABLE]
    assert got == _WGRAD_WS_TABLE, [(g, w[2]) for g, w in zip(got, _WGRAD_WS_TABLE) if g != w]
    assert len(_WGRAD_WS_TABLE) >= 25 and sum(1 for _, _, n in _WGRAD_WS_TABLE if n in (0, 16)) >= 5
    # the loop form moves the choice on 84-pixel rows, the fill threshold on 40-pixel ones
    by = {(s, tuple(sorted(kw.items()))): n for s, kw, n in _WGRAD_WS_TABLE}
    assert by[((4, 40, 84, 64, 64), (("LEAN", 31),))] != by[((4, 40, 84, 64, 64), (("LEAN", 14),))]
    assert by[((8, 40, 40, 64, 64), (("WGRAD_ROWS_FILL", 30),))] != by[((8, 40, 40, 64, 64), (("WGRAD_ROWS_FILL", 70),))]
