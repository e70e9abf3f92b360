"""``'cross_mse'`` / ``'mean_mse'`` as the consistency criterion of the co-training step: the fused launch sequence
(``dct_mse_logits_step`` behind ``CoTrainer._jsd``) against the generic step through the public modules, the captured step against
eager launches, the captured-step signature, and a short run.  Method, helpers, tolerances and golden set-ups are
tests/test_soft_label_step_gpu.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_step_gpu import _trainer as _step_trainer  # noqa: E402
from test_weighted_step_gpu import DEV, _moments_agree, _one_step  # noqa: E402

# Golden set-up, criterion, threshold of the fused-vs-generic comparison: the ensemble threshold is the one test_soft_label_step_gpu
# uses on this set-up (no confidence within NEAR of it, asserted again below from this file's own run).
NEAR = 1e-6
ENET, UNET = "g5_step_enet_adv", "g5_step_unet_adv"
CONS = [(ENET, "cross_mse", 0.0), (ENET, "mean_mse", 0.32), (UNET, "mean_mse", 0.0)]
OTHERS = [(ENET, "jsd", 0.0), (ENET, "cps", 0.0), (ENET, "soft_cps", 0.0), (ENET, "mean_mse", 0.0)]


def _cons(name, tau, generic=False):
    """The registry's criterion; ``generic``: as an instance of a subclass of its type, which the fused step does not know by type
    and therefore leaves to the module (the generic step) -- the planner's own rule, not a switch of the tests."""
    from dct_amd.loss import get_loss_fn
    crit = get_loss_fn(name) if name == "jsd" else get_loss_fn(name, threshold=tau)
    if generic:
        crit.__class__ = type("Users" + type(crit).__name__, (type(crit),), {})
    return crit


def _trainer(tmp_path, g, n_steps, cons):
    """test_step_gpu's trainer of a golden set-up (fp32, plain cross entropy) with ``cons`` as the consistency criterion."""
    tr, lab, unl = _step_trainer(tmp_path, g, torch.float32, n_steps)
    tr.criterions["jsd"] = cons
    return tr, lab, unl


def _near(probs, name, tau):
    """Pixels whose teacher's confidence is within NEAR of ``tau``: there the mask could differ between two routes that differ in the
    last bits.  ``probs``: the step's [B, C, H, W] softmax maps."""
    ps = [p.detach().double().permute(0, 2, 3, 1).reshape(-1, p.shape[1]).cpu() for p in probs]
    vecs = ps if name == "cross_mse" else [sum(ps) / len(ps)]
    flag = torch.zeros(ps[0].shape[0], dtype=torch.bool)
    if tau > 0:
        for v in vecs:
            flag |= (v.max(1).values - tau).abs() < NEAR
    return int(flag.sum()), flag.numel()


@pytest.fixture(scope="module")
def fused_steps(golden, tmp_path_factory):
    """One fused step per set-up and consistency criterion: (tag, name, tau) -> (step output, weight digests, kept fraction)."""
    res = {}
    for tag, name, tau in OTHERS + CONS:
        tr, lab, unl = _trainer(tmp_path_factory.mktemp(name), golden(tag), 1, _cons(name, tau))
        assert tr._fused_ok()                    # the MSE criteria stay on the fused step
        out, w = _one_step(tr, lab, unl)
        assert tr.last_route.joint_pass or tr.last_route.model_streams        # (a fused route, not the generic one)
        kept = None
        if name != "jsd":
            kept = tr.criterions["jsd"].last_kept
            assert torch.is_tensor(kept) and kept.is_cuda
            kept = kept.item()
        res[(tag, name, tau)] = (out, w, kept)
    return res


@pytest.mark.parametrize("tag,name,tau", CONS)
def test_mse_fused_and_generic_paths_agree(golden, tmp_path, fused_steps, tag, name, tau):
    """test_spl_fused_and_generic_paths_agree with a softmax-MSE criterion, at that test's tolerances; the generic step is reached the
    way a user reaches it, with a subclass of the criterion.  No pixel's confidence may sit within 1e-6 of the threshold (asserted)."""
    a, wa, kept_a = fused_steps[(tag, name, tau)]
    near, P = _near(a["unlab_probs"], name, tau)
    print(f"{tag} {name} tau={tau}: {near} of {P} pixels within {NEAR} of the threshold; kept {kept_a}; value {a['jsd'].item()}")
    assert P == (8192 if tag == ENET else 30976) and near == 0
    if tau == 0.0:
        assert kept_a == 1.0
    else:
        assert 0.2 < kept_a < 0.8                # the threshold masks some teachers and keeps some
    tr, lab, unl = _trainer(tmp_path, golden(tag), 1, _cons(name, tau, generic=True))
    assert not tr._fused_ok()
    b, wb = _one_step(tr, lab, unl)
    r = tr.last_route                            # the generic step's route: one autograd backward, nothing forked, nothing captured
    assert not r.model_streams and not r.joint_pass and tr._step_graphs is None
    np.testing.assert_allclose(tr.criterions["jsd"].last_kept.item(), kept_a, rtol=1e-6)
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    _moments_agree(wa, wb)


def test_mse_criteria_reach_the_fused_step(fused_steps):
    """No silent fall-through: the consistency value is neither a 'jsd', 'cps' or 'soft_cps' trainer's nor the other mode's or the other
    threshold's, it respects the rule's bound 2 / C, and the model weights after the update differ as well."""
    enet = {k: v for k, v in fused_steps.items() if k[0] == ENET}
    keys = list(enet)
    assert len(keys) == 6
    vals = {k: enet[k][0]["jsd"].item() for k in keys}
    for i, x in enumerate(keys):
        assert np.isfinite(vals[x])
        if x[1].endswith("mse"):
            C = enet[x][0]["unlab_probs"][0].shape[1]
            assert 0.0 < vals[x] <= 2.0 / C
        for y in keys[i + 1:]:
            if x[1].endswith("mse") or y[1].endswith("mse"):
                assert abs(vals[x] - vals[y]) > 1e-3 * abs(vals[y]), (x, y, vals[x], vals[y])
                assert any(not np.array_equal(a, b) for a, b in zip(enet[x][1], enet[y][1])), (x, y)


@pytest.mark.parametrize("arch,adv,name,tau", [("unet", True, "cross_mse", 0.0), ("enet", False, "mean_mse", 0.34)])
def test_mse_graph_replay_equals_eager_step_sequence(tmp_path, arch, adv, name, tau):
    """test_spl_graph_replay_equals_eager_step_sequence with a softmax-MSE criterion: the captured step (lr and lambda_cot change between
    replays) gives exactly the eager steps' values, kept fractions, weights and moments."""
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
        crit = {"sup": get_loss_fn("cross_entropy"), "jsd": _cons(name, tau), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        tr.use_hip_graph = use_graph
        assert tr._fused_ok()
        for s in segs:
            s.train()
        vals = []
        for k in range(n):
            if k == 4:                          # between replays: lr and lambda_cot change
                for s in segs:
                    s.optimizer.param_groups[0]["lr"] = 3e-4
                tr.cot_scheduler.max_value = 0.25
            lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
            out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, adv, (0, 1) if adv else None)
            vals.append([float(v) for v in out["sup"]] + [float(out["jsd"]), float(crit["jsd"].last_kept)])
        torch.cuda.synchronize()
        if use_graph:
            assert tr._step_graphs is not None and tr._step_graphs.captures >= 1 and tr._step_graphs.replays >= 4
        res.append(dict(
            w=[torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in segs],
            m=[s.optimizer._m.cpu() for s in segs], steps=[s.optimizer._steps for s in segs], vals=vals))
    a, b = res
    assert a["steps"] == b["steps"] == [n, n]
    assert a["vals"] == b["vals"] and all(np.isfinite(v) for s in a["vals"] for v in s)
    if tau == 0.0:
        assert all(s[-1] == 1.0 for s in a["vals"])
    for x, y in zip(a["w"] + a["m"], b["w"] + b["m"]):
        assert torch.equal(x, y)


def test_another_threshold_is_another_capture(tmp_path, golden):
    """StepGraphCache._signature carries the consistency criterion's type and launch arguments: another threshold or teacher is another
    capture -- and so are the hard and the soft criterion of the same teacher and threshold -- while the same criterion object (whose
    ``last_kept`` changes with every step) is not."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.trainer.step_graph import StepGraphCache
    g = golden("g5_step_unet_adv")
    tr, lab, unl = _trainer(tmp_path, g, 1, _cons("cross_mse", 0.5))
    _one_step(tr, lab, unl)                      # (flat parameters and gradients exist; last_kept is set)
    cache = StepGraphCache(tr)
    lb = [(lab[i][0][0][0].to(DEV), lab[i][0][0][1].to(DEV)) for i in range(2)]

    def sig():
        return cache._signature(lb, None, False, False, None, (0.0, 0.0), "one_graph", tr.last_route)
    s0 = sig()
    tr.criterions["jsd"].last_kept = None
    assert sig() == s0
    assert s0[-1] == ("CrossMSE_2D", (("tau", 0.5), ("teacher", 0)))
    sigs = [s0]
    for cons in (_cons("cross_mse", 0.6), _cons("cross_mse", 0.0), _cons("mean_mse", 0.5), _cons("cps", 0.5), _cons("soft_cps", 0.5),
                 get_loss_fn("jsd")):
        tr.criterions["jsd"] = cons
        sigs.append(sig())
    assert len(set(sigs)) == len(sigs)
    assert sigs[-1][-1] is None and all(s[:-1] == s0[:-1] for s in sigs)       # only the appended entry tells them apart


def test_short_run_and_the_jsd_trainer_beside_it(tmp_path, golden, monkeypatch):
    """Four steps on one unlabeled batch with lambda_cot = 0.5 stay finite.  A 'jsd' trainer built beside it launches what it launched
    before the MSE criteria existed -- ``hip_ops.jsd_logits_step`` with the same arguments, never ``mse_logits_step``,
    ``spl_logits_step`` or ``pl_logits_step`` -- and gives bit for bit the values and weights of a trainer whose ``_jsd`` is that earlier
    method; a 'cps' trainer launches ``pl_logits_step`` and never ``mse_logits_step``."""
    from dct_amd import hip_ops as K
    from dct_amd.loss.loss import _nchw
    g = golden("g5_step_unet_adv")
    n = 4
    for d in ("cross_mse", "mean_mse", "cps", "jsd", "jsd_before"):
        (tmp_path / d).mkdir()

    def run(tr, lab, unl):
        for s in tr.segmentators:
            s.train()
        lb = [lab[i][0][0] for i in range(2)]
        vals = []
        for _ in range(n):
            out = tr._run_step([(lb[0][0], lb[0][1]), (lb[1][0], lb[1][1])], (unl[0][0][0], unl[0][0][1]), True, False, None)
            vals.append(out["jsd"].item())
        w = [torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in tr.segmentators]
        return vals, w

    calls = {"jsd": 0, "pl": 0, "spl": 0, "mse": 0}
    jsd_step = K.jsd_logits_step

    def spy(key, f):
        def g_(*a, **k):
            calls[key] += 1
            return f(*a, **k)
        return g_
    for key in calls:
        monkeypatch.setattr(K, key + "_logits_step", spy(key, getattr(K, key + "_logits_step")))

    def others(before, but):
        return all(calls[k] == before[k] for k in calls if k != but)

    for name in ("cross_mse", "mean_mse"):
        before = dict(calls)
        tr, lab, unl = _trainer(tmp_path / name, g, 1, _cons(name, 0.0))
        vals, w = run(tr, lab, unl)
        print(name, vals)
        assert all(np.isfinite(vals)) and all(torch.isfinite(x).all() for x in w), (name, vals)
        assert all(0.0 <= v <= 2.0 / tr.C for v in vals), (name, vals)
        assert calls["mse"] > before["mse"] and others(before, "mse")

    before = dict(calls)
    tr, lab, unl = _trainer(tmp_path / "cps", g, 1, _cons("cps", 0.0))
    run(tr, lab, unl)
    assert calls["pl"] > before["pl"] and others(before, "pl")

    before = dict(calls)
    tr, lab, unl = _trainer(tmp_path / "jsd", g, 1, _cons("jsd", 0.0))
    va, wa = run(tr, lab, unl)
    assert calls["jsd"] > before["jsd"] and others(before, "jsd")

    def jsd_before(ctx, lps, dl_outs):          # CoTrainer._jsd as it was before the pseudo-label criteria
        jsd1, probs = jsd_step(lps, tr2.C, dl_outs if ctx.lam_cot != 0.0 else None, True, **ctx.g_cot)
        return jsd1[0], [_nchw(p_) for p_ in probs]
    tr2, lab, unl = _trainer(tmp_path / "jsd_before", g, 1, _cons("jsd", 0.0))
    tr2._jsd = jsd_before
    vb, wb = run(tr2, lab, unl)
    assert va == vb and all(torch.equal(x, y) for x, y in zip(wa, wb))
