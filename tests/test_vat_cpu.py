"""VAT as the second generator of the adversarial term, the parts that need no GPU: the float64 reference of tests/vat_ref.py checks
itself, the planner keeps every FGSM route and sends VAT steps down the sequential layout, the settings are validated, and the
captured step's signature tells the settings apart."""
import dataclasses
import itertools
import math
import types

import numpy as np
import pytest
import torch

import vat_ref


# ------------------------------------------------------------------------------------------------ the reference checks itself
@pytest.mark.parametrize("eps", [0.5, 10.0])
def test_reference_perturbation_has_the_radius(eps):
    x, d = vat_ref.toy_case(0)
    xo, r, nrm = vat_ref.perturb(x, d * 1e-7, eps)
    got = vat_ref.norms(r)
    assert torch.all((got - eps).abs() <= 1e-12 * eps), got
    assert torch.equal(xo, x + r)
    np.testing.assert_allclose(nrm.numpy(), 1e-7 * vat_ref.norms(d).numpy(), rtol=1e-14)


def test_reference_zero_and_inf_samples_get_no_perturbation():
    x, d = vat_ref.toy_case(1)
    d[0].zero_()
    d[2, 1, 2, 3] = float("inf")
    xo, r, nrm = vat_ref.perturb(x, d, 0.5)
    assert nrm[0] == 0 and math.isinf(nrm[2])
    for n in (0, 2):
        assert torch.equal(xo[n], x[n]) and torch.count_nonzero(r[n]) == 0
    assert abs(vat_ref.norms(r)[1].item() - 0.5) <= 1e-12


def test_reference_noise_moments():
    """|mean| < 5 / sqrt(n) and |var - 1| < 5 sqrt(2 / n) over 2^20 elements (this seed: 1.1e-4 and 9.8e-4 against 4.9e-3 and 6.9e-3)."""
    n = 1 << 20
    z = vat_ref.noise((n,), seed=0x1234567 + (5 << 32), call=3)
    mean, var = z.mean(), z.var()
    print(f"noise over 2^20 elements: |mean| {abs(mean):.2e} (limit {5 / math.sqrt(n):.2e}), |var - 1| {abs(var - 1):.2e} "
          f"(limit {5 * math.sqrt(2 / n):.2e})")
    assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)
    assert np.all(np.isfinite(z))
    # another call, another seed: other draws; a prefix of a longer draw: the same draws
    assert not np.array_equal(z[:64], vat_ref.noise((64,), 0x1234567 + (5 << 32), 4))
    assert not np.array_equal(z[:64], vat_ref.noise((64,), 0x1234568 + (5 << 32), 3))
    assert np.array_equal(z[:61], vat_ref.noise((61,), 0x1234567 + (5 << 32), 3))


@pytest.mark.parametrize("ip", [1, 2])
def test_reference_generator_beats_a_random_step(ip):
    """The property the generator exists for, on the reference: for every sample KL at x + r is more than 1.5 x KL at the equally long
    random step eps d0 / ||d0|| (worst ratio over these 20 seeds: 1.84 for ip = 1, 1.94 for ip = 2)."""
    net = vat_ref.ToyNet()
    worst = float("inf")
    for seed in range(20):
        x, d0 = vat_ref.toy_case(seed)
        x_adv, r, probs = vat_ref.generate(net, x, d0, xi=0.01, eps=0.5, ip=ip)
        with torch.no_grad():
            l = net(x)
            ratio = vat_ref.kl_per_sample(l, net(x_adv)) / vat_ref.kl_per_sample(l, net(vat_ref.perturb(x, d0, 0.5)[0]))
        worst = min(worst, ratio.min().item())
        assert torch.all((vat_ref.norms(r) - 0.5).abs() <= 1e-12)
        assert torch.allclose(probs.sum(1), torch.ones_like(probs.sum(1)))
    print(f"ip = {ip}: worst KL ratio over 20 seeds {worst:.3f}")
    assert worst > 1.5


# ------------------------------------------------------------------------------------------------ planner
def _facts_grid():
    from dct_amd.trainer.step_route import NetFacts, StepFacts
    unet = NetFacts(plan_net=True, batch_independent=True, supports_grad_overwrite=True, supports_forward_reuse=True, grads_attached=True)
    enet = NetFacts(plan_net=True, supports_pass_streams=True, supports_deferred_running_stats=True, supports_pass_groups=True,
                    prefers_segmented_graphs=True, grads_attached=True)
    other = NetFacts()
    for nets, train_jsd, train_adv, unlabeled, lam_adv_zero, ddp in itertools.product(
            ((unet, unet), (enet, enet), (unet, enet), (other, other), (unet, unet, unet)), (False, True), (False, True), (False, True),
            (False, True), (False, True)):
        if (train_jsd or train_adv) and not unlabeled:
            continue
        yield dict(S=len(nets), nets=nets, train_jsd=train_jsd, train_adv=train_adv, adv_choice=(0, 1) if train_adv else None,
                   unlabeled=unlabeled, labeled_equals_unlabeled=True, labeled_pixels=2 * 64 * 64, lam_adv_zero=lam_adv_zero, gpu=True,
                   fused_criteria=True, ddp=ddp, optimizers_graphable=True, group_max=8)


def _plans():
    from dct_amd.trainer.cotraining_totalloss import ExecutionPlan
    return [ExecutionPlan(), ExecutionPlan(use_hip_graph=False), ExecutionPlan(wide_forward=False), ExecutionPlan(adv_chain_layout=False),
            ExecutionPlan(group_passes=False)]


def test_default_generator_is_fgsm_and_every_route_is_unchanged():
    from dct_amd.trainer.step_route import StepFacts, plan_execution, plan_step
    assert StepFacts(S=1, nets=()).adv_generator == "fgsm"
    assert [f.name for f in dataclasses.fields(StepFacts)][-1] == "adv_generator"       # appended: positional construction is unchanged
    n = 0
    kinds = set()
    for plan in _plans():
        for kw in _facts_grid():
            a, b = StepFacts(**kw), StepFacts(adv_generator="fgsm", **kw)
            assert a == b
            ex = plan_execution(plan, a)
            assert ex == plan_execution(plan, b)
            for mode in {"eager", "eager" if ex == "generic" else ex}:
                ra = plan_step(plan, a, mode, lambda: True)
                assert ra == plan_step(plan, b, mode, lambda: True)
                kinds.add(ra.kind)
                n += 1
    assert n > 200 and kinds == {"sequential", "wide", "wide_grouped", "adv_chain"}      # the grid reaches every layout


def test_vat_steps_are_routed_sequentially():
    from dct_amd.trainer.step_route import StepFacts, adv_chain_eligible, plan_execution, plan_step
    n = changed = 0
    for plan in _plans():
        for kw in _facts_grid():
            if not kw["train_adv"]:
                # without an adversarial term the generator is not looked at
                a, v = StepFacts(**kw), StepFacts(adv_generator="vat", **kw)
                assert plan_execution(plan, a) == plan_execution(plan, v)
                assert plan_step(plan, a, "eager", lambda: True) == plan_step(plan, v, "eager", lambda: True)
                continue
            f, v = StepFacts(**kw), StepFacts(adv_generator="vat", **kw)
            assert not adv_chain_eligible(plan, v)
            ex = plan_execution(plan, v)
            if adv_chain_eligible(plan, f) and plan_execution(plan, f) == "program":
                assert ex == "one_graph"          # the execution follows: no chain to give a hardware queue to
            for mode in {"eager", "eager" if ex == "generic" else ex}:
                r = plan_step(plan, v, mode, lambda: True)
                assert r.kind == "sequential" and not r.adv_chain_eligible and not r.share_fgsm_encoder and not r.leaf_offload
                changed += r != plan_step(plan, f, mode, lambda: True)
                n += 1
    assert n > 100 and changed > 10


# ------------------------------------------------------------------------------------------------ settings
def test_adv_settings_defaults_and_errors():
    from dct_amd.trainer.step_route import adv_settings
    assert adv_settings({}) == ("fgsm", None, 0.05, None) == adv_settings(None)
    assert adv_settings({"eplision": 0.03}) == ("fgsm", None, 0.03, None)
    assert adv_settings({"generator": "fgsm", "xi": 3.0, "ip": 4, "eplision": 0.1}) == ("fgsm", None, 0.1, None)
    assert adv_settings({"generator": "vat"}) == ("vat", 10.0, 10.0, 1)
    assert adv_settings({"generator": "vat", "xi": 0.5, "eplision": 2, "ip": 3}) == ("vat", 0.5, 2.0, 3)
    for bad in ({"generator": "pgd"}, {"generator": "VAT"}, {"eplision": 0.0}, {"eplision": -1.0}, {"eplision": float("nan")},
                {"generator": "vat", "xi": 0.0}, {"generator": "vat", "xi": -1e-6}, {"generator": "vat", "eplision": 0},
                {"generator": "vat", "ip": 0}, {"generator": "vat", "ip": -2}, {"generator": "vat", "ip": 1.5},
                {"generator": "vat", "xi": float("inf")}):
        with pytest.raises(ValueError, match="adv_training_dict"):
            adv_settings(bad)


def test_generator_arguments_are_validated_without_a_device():
    from dct_amd.utils.AEGenerator import VATGenerator, VATNoise
    net = torch.nn.Identity()
    for kw in (dict(xi=0.0), dict(eplision=-1.0), dict(ip=0), dict(ip=1.5)):
        with pytest.raises(ValueError):
            VATGenerator(net, **kw)
    g = VATGenerator(net)
    assert (g.xi, g.eplision, g.ip) == (10.0, 10.0, 1) and isinstance(g.noise, VATNoise)


def test_noise_seed_is_drawn_lazily_and_mixed_by_rank():
    from dct_amd.utils.AEGenerator import VATNoise
    torch.manual_seed(7)
    before = torch.get_rng_state()
    a = VATNoise()
    fixed = VATNoise(seed=99)
    assert torch.equal(torch.get_rng_state(), before)          # constructing draws nothing
    assert fixed.seed == 99 and torch.equal(torch.get_rng_state(), before)
    s = a.seed
    assert not torch.equal(torch.get_rng_state(), before) and 0 <= s < 2 ** 62 and a.seed == s
    r0, r1, r2 = VATNoise(seed=5), VATNoise(seed=5), VATNoise(seed=5)
    r0.mix_rank(0), r1.mix_rank(1), r2.mix_rank(2)
    r1.mix_rank(1)                                              # once only
    assert r0.seed == 5 and len({r0.seed, r1.seed, r2.seed}) == 3 and all(0 <= r.seed < 2 ** 62 for r in (r1, r2))
    assert a._calls == 0


def test_step_reads_and_validates_the_dictionary(tmp_path, monkeypatch):
    """An unknown generator and a non-positive xi / eplision / ip raise where the step reads the dictionary, before anything runs."""
    from test_host_logic_cpu import _make_trainer
    tr = _make_trainer(tmp_path, monkeypatch, "enet", 3, 32, 2, 1)[0]
    for bad in ({"generator": "pgd"}, {"generator": "vat", "xi": 0.0}, {"generator": "vat", "eplision": -3.0}, {"generator": "vat", "ip": 0}):
        tr.adv_training_dict = bad
        with pytest.raises(ValueError, match="adv_training_dict"):
            tr._run_step([], None, False, True, (0, 1))
    tr.adv_training_dict = {"generator": "vat", "xi": 2.0}
    assert tr._step_facts().adv_generator == "vat"
    tr.adv_training_dict = {"eplision": 0.05}
    assert tr._step_facts().adv_generator == "fgsm" and tr.vat_noise is None


# ------------------------------------------------------------------------------------------------ the captured step's signature
def _signature(adv, train_adv=True, noise=None):
    from dct_amd.trainer.step_graph import StepGraphCache
    from dct_amd.trainer.step_route import StepRoute
    sup = types.SimpleNamespace(ignore_index=-100, device_weight=lambda device, C: None)
    tr = types.SimpleNamespace(segmentators=[], criterions={"sup": sup, "jsd": object()}, device=torch.device("cpu"), C=3,
                               adv_training_dict=adv, vat_noise=noise)
    return StepGraphCache(tr)._signature([], None, True, train_adv, (0, 1) if train_adv else None, (0.5, 0.05), "one_graph", StepRoute())


def test_signature_tells_the_settings_apart():
    from dct_amd.utils.AEGenerator import VATNoise
    base = {"generator": "vat", "xi": 1.0, "eplision": 2.0, "ip": 1}
    s0 = _signature(base)
    assert s0 == _signature(dict(base)) and hash(s0) == hash(_signature(dict(base)))
    for other in (dict(base, xi=1.5), dict(base, eplision=2.5), dict(base, ip=2), {"eplision": 2.0}, {"generator": "fgsm", "eplision": 2.0}):
        assert _signature(other) != s0
    assert _signature({"eplision": 2.0}) == _signature({"generator": "fgsm", "eplision": 2.0, "xi": 9.0, "ip": 7})   # FGSM reads neither
    assert _signature({"eplision": 0.03}) != _signature({"eplision": 0.05})
    # without an adversarial term the dictionary is not part of the step
    assert _signature(base, train_adv=False) == _signature({"eplision": 0.03}, train_adv=False)
    # another noise object (seed, counter word) is another capture; an FGSM step does not look at it (and draws no seed)
    n1, n2 = VATNoise(seed=1), VATNoise(seed=2)
    assert _signature(base, noise=n1) != _signature(base, noise=n2)
    lazy = VATNoise()
    assert _signature({"eplision": 0.03}, noise=lazy) == _signature({"eplision": 0.03}) and lazy._seed is None
