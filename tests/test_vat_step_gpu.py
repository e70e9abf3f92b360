"""``generator='vat'`` in ``CoTrainer.adv_training_dict``: the fused launch sequence (``CoTrainer._vat_fused``) against the generic step
through ``VATGenerator``, the route it takes, the captured step against eager launches, and the untouched FGSM default.  Golden set-ups,
helpers and tolerances are tests/test_step_gpu.py's and tests/test_mse_consistency_step_gpu.py's.  eplision = xi = 0.03 sqrt(per) gives
the golden FGSM's per-pixel size."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_step_gpu import _trainer as _step_trainer  # noqa: E402
from test_weighted_step_gpu import DEV, _moments_agree, _one_step  # noqa: E402

ENET, UNET = "g5_step_enet_adv", "g5_step_unet_adv"
NOISE_SEED = 0x51F15EED


def _vat_dict(g, **kw):
    per = int(g["H"]) ** 2                      # one input channel
    e = 0.03 * math.sqrt(per)
    return dict(dict(generator="vat", eplision=e, xi=e, ip=1), **kw)


def _trainer(tmp_path, g, adv_dict, generic=False, lam_adv=None):
    from dct_amd.utils.AEGenerator import VATNoise
    tr, lab, unl = _step_trainer(tmp_path, g, torch.float32, 1)
    tr.adv_training_dict = adv_dict
    tr.vat_noise = VATNoise(seed=NOISE_SEED)
    if lam_adv is not None:
        tr.adv_scheduler.max_value = lam_adv
    if generic:         # a subclass of the supervised criterion: the fused step does not know it by type (the planner's own rule)
        sup = tr.criterions["sup"]
        sup.__class__ = type("Users" + type(sup).__name__, (type(sup),), {})
    return tr, lab, unl


@pytest.fixture(scope="module")
def fused_steps(golden, tmp_path_factory):
    """One fused step per set-up and generator: (tag, generator) -> (step output, weight digests, trainer)."""
    res = {}
    for tag in (ENET, UNET):
        g = golden(tag)
        for name, d in (("vat", _vat_dict(g)), ("fgsm", {"eplision": float(g["eps"])})):
            tr, lab, unl = _trainer(tmp_path_factory.mktemp(name), g, d)
            assert tr._fused_ok()
            out, w = _one_step(tr, lab, unl)
            res[(tag, name)] = (out, w, tr)
    return res


@pytest.mark.parametrize("tag", [ENET, UNET])
def test_vat_fused_and_generic_paths_agree(golden, tmp_path, fused_steps, tag):
    """test_mse_fused_and_generic_paths_agree's comparison and tolerances with VAT making the adversarial examples; both trainers draw
    from the same noise seed."""
    a, wa, tr_a = fused_steps[(tag, "vat")]
    tr, lab, unl = _trainer(tmp_path, golden(tag), _vat_dict(golden(tag)), generic=True)
    assert not tr._fused_ok()
    b, wb = _one_step(tr, lab, unl)
    r = tr.last_route
    assert not r.model_streams and not r.joint_pass and tr._step_graphs is None
    assert tr.vat_noise._calls == tr_a.vat_noise._calls == 1
    assert int(tr.vat_noise.state(DEV).item()) == int(tr_a.vat_noise.state(DEV).item()) == 1
    print(f"{tag}: adv fused {a['adv'].item():.6e} generic {b['adv'].item():.6e}")
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    _moments_agree(wa, wb)


@pytest.mark.parametrize("tag", [ENET, UNET])
def test_vat_reaches_the_sequential_fused_step(fused_steps, tag):
    """No silent fall-through to FGSM: the route is the sequential one, and the adversarial value and the updated weights are not an FGSM
    trainer's."""
    v, wv, tr_v = fused_steps[(tag, "vat")]
    f, wf, tr_f = fused_steps[(tag, "fgsm")]
    assert tr_v.last_route.kind == "sequential" and not tr_v.last_route.adv_chain_eligible
    assert tr_v.last_route.joint_pass or tr_v.last_route.model_streams           # (a fused route, not the generic one)
    assert tr_f.vat_noise._calls == 0 and tr_f.vat_noise._seed == NOISE_SEED      # the FGSM trainer never touched its noise object
    av, af = v["adv"].item(), f["adv"].item()
    assert np.isfinite(av) and av > 0 and abs(av - af) > 1e-3 * abs(af), (av, af)
    assert any(np.max(np.abs(np.asarray(x) - np.asarray(y)) / (np.abs(np.asarray(y)) + 1e-30)) > 1e-3 for x, y in zip(wv.moments, wf.moments))
    assert any(not np.array_equal(x, y) for x, y in zip(wv, wf))


def _small_trainer(tmp_path, arch, adv_dict, use_graph, n, lam_adv=0.05, noise=True):
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    from dct_amd.utils.AEGenerator import VATNoise
    C, B, H = 3, 2, (176 if arch == "unet" else 64)
    segs = []
    for seed in (11, 12):
        torch.manual_seed(seed)
        segs.append(Segmentator({"name": arch, "num_classes": C, "compute_dtype": torch.bfloat16},
                                {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(2)]
    unl = FakeLoader(batches(91, n, B, H, C), B)
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": lam_adv},
                   adv_training_dict=adv_dict, use_tqdm=False, steps_per_epoch=n)
    tr.use_hip_graph = use_graph
    if noise:
        tr.vat_noise = VATNoise(seed=NOISE_SEED)
    for s in segs:
        s.train()
    return tr, segs, lab, unl


def _step(tr, lab, unl, k):
    lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
    return tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, True, (0, 1))


def _state(segs):
    return dict(w=[torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in segs],
                m=[s.optimizer._m.cpu() for s in segs])


@pytest.mark.parametrize("arch", ["unet", "enet"])
def test_vat_graph_replay_equals_eager_step_sequence(tmp_path, arch):
    """test_graph_replay_equals_eager_step_sequence with VAT: seven steps (two eager, the capture, four replays; lr and both loss weights
    change on the way) leave exactly the values, weights and moments of seven eager steps -- every replay drew fresh noise -- and the
    host mirror of the draw counter equals the device word."""
    n = 7
    H = 176 if arch == "unet" else 64
    e = 0.03 * H
    res = []
    for use_graph in (False, True):
        tr, segs, lab, unl = _small_trainer(tmp_path, arch, dict(generator="vat", eplision=e, xi=e, ip=1), use_graph, n)
        vals = []
        for k in range(n):
            if k == 4:
                for s in segs:
                    s.optimizer.param_groups[0]["lr"] = 3e-4
                tr.cot_scheduler.max_value = 0.25
                tr.adv_scheduler.max_value = 0.1
            out = _step(tr, lab, unl, k)
            assert tr.last_route.kind == "sequential"
            vals.append([float(v) for v in out["sup"]] + [float(out["jsd"]), float(out["adv"])])
        torch.cuda.synchronize()
        if use_graph:
            assert tr._step_graphs is not None and tr._step_graphs.captures == 1 and tr._step_graphs.replays >= 4
        assert tr.vat_noise._calls == n == int(tr.vat_noise.state(DEV).item())
        res.append(dict(_state(segs), vals=vals))
    a, b = res
    assert a["vals"] == b["vals"]
    assert len({v[3] for v in a["vals"]}) == n                                   # (seven different adversarial values)
    for x, y in zip(a["w"] + a["m"], b["w"] + b["m"]):
        assert torch.equal(x, y)


def test_vat_runs_with_lambda_adv_zero_and_another_xi_is_another_capture(tmp_path):
    """lambda_adv = 0: the generator still runs (the value is reported), nothing reads the weight; changing xi between replays leads to a
    second capture, not to a replay with the old radius."""
    n = 8
    e = 0.03 * 64
    tr, segs, lab, unl = _small_trainer(tmp_path, "enet", dict(generator="vat", eplision=e, xi=e, ip=2), True, n, lam_adv=0.0)
    vals = []
    for k in range(n):
        if k == 4:
            tr.adv_training_dict = dict(tr.adv_training_dict, xi=0.25 * e)
        vals.append(float(_step(tr, lab, unl, k)["adv"]))
        assert tr.vat_noise._calls == k + 1
    torch.cuda.synchronize()
    assert all(np.isfinite(v) and v > 0 for v in vals)
    assert int(tr.vat_noise.state(DEV).item()) == n
    assert tr._step_graphs.captures == 2 and tr._step_graphs.replays >= 2


def test_fgsm_default_is_untouched(tmp_path):
    """The default dictionary names no generator and runs what it ran: the same route and bit-equal results with the generator named
    explicitly, and with or without an unused VATNoise attached (whose seed is never drawn)."""
    res = []
    for d, noise in (({"eplision": 0.03}, False), ({"eplision": 0.03}, True), ({"generator": "fgsm", "eplision": 0.03, "xi": 1.0, "ip": 3}, False)):
        tr, segs, lab, unl = _small_trainer(tmp_path, "unet", d, True, 4, noise=False)
        if noise:
            from dct_amd.utils.AEGenerator import VATNoise
            tr.vat_noise = VATNoise()
        rng = torch.get_rng_state()
        vals = []
        for k in range(4):
            out = _step(tr, lab, unl, k)
            vals.append([float(v) for v in out["sup"]] + [float(out["jsd"]), float(out["adv"])])
        torch.cuda.synchronize()
        assert torch.equal(torch.get_rng_state(), rng)
        if noise:
            assert tr.vat_noise._seed is None and tr.vat_noise._calls == 0 and tr.vat_noise._state is None
        else:
            assert tr.vat_noise is None
        res.append(dict(_state(segs), vals=vals, route=tr.last_route, captures=tr._step_graphs.captures))
    for other in res[1:]:
        assert other["vals"] == res[0]["vals"] and other["route"] == res[0]["route"] and other["captures"] == res[0]["captures"] == 1
        for x, y in zip(other["w"] + other["m"], res[0]["w"] + res[0]["m"]):
            assert torch.equal(x, y)
    assert res[0]["route"].kind == "adv_chain" or res[0]["route"].adv_chain_eligible
