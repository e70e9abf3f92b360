"""The co-training step on the GPU (fused HIP path behind CoTrainer._run_step/_train_loop) against
golden vectors captured from the reference's own CoTrainer._train_loop (tests/golden/g5_step_unet_*)
and against the CPU oracle.  fp32 mode carries the parity claim."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from helpers import FakeLoader, batches, digest  # noqa: E402

DEV = "cuda:0"


def _seeded_state(arch, C, seed):
    torch.manual_seed(seed)
    kw = {"dropout_p": 0.0} if arch == "unet" else {}
    return oracle.build_net(arch, C, **kw).state_dict()


def _trainer(tmp_path, g, dtype, n_steps, fused=True):
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, H, B = int(g["C"]), int(g["H"]), int(g["B"])
    arch = str(g["arch"])
    segs = []
    for s in g["net_seeds"]:
        arch_dict = {"name": arch, "num_classes": C, "compute_dtype": dtype}
        if arch == "unet":
            arch_dict["dropout_p"] = 0.0
        seg = Segmentator(arch_dict, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                          {"name": "StepLR", "step_size": 90, "gamma": 0.1})
        seg.torchnet.load_state_dict(_seeded_state(arch, C, int(s)))
        segs.append(seg)
    lab = [FakeLoader(batches(int(s), n_steps, B, H, C), B) for s in g["lab_seeds"]]
    unl = FakeLoader(batches(int(g["unl_seed"]), n_steps, B, H, C), B)
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segmentators=segs, labeled_dataloaders=lab, unlabeled_dataloader=unl, val_dataloader=unl,
                   criterions=crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=list(range(1, C)),
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": float(g["lam_cot"])},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": float(g["lam_adv"])},
                   adv_training_dict={"eplision": float(g["eps"])}, use_tqdm=False, steps_per_epoch=n_steps)
    if not fused:
        tr._fused_ok = lambda: False
    return tr, lab, unl


@pytest.mark.parametrize("tag", ["g5_step_unet_jsd", "g5_step_unet_adv", "g5_step_enet_jsd", "g5_step_enet_adv"])
def test_train_loop_fp32_matches_reference_golden(golden, tmp_path, tag):
    from dct_amd import ModelMode
    g = golden(tag)
    n, adv = int(g["n_steps"]), bool(int(g["train_adv"]))
    tr, lab, unl = _trainer(tmp_path, g, torch.float32, n)
    assert tr._fused_ok()
    log = []
    orig = tr._run_step

    def rec(*a, **k):
        out = orig(*a, **k)
        log.append(out)
        return out

    tr._run_step = rec
    np.random.seed(1234)
    dice_lab, dice_unl = tr._train_loop(lab, unl, epoch=0, mode=ModelMode.TRAIN, save=False, train_jsd=True, train_adv=adv)
    assert len(log) == n
    # Enet (84 train-mode BatchNorms over 2x8x8 .. 2x32x32 samples) amplifies last-bit differences far more
    # than UNet (tests/test_enet_gpu.py): 5x looser on everything after the first update
    enet = str(g["arch"]) == "enet"
    loose = 5.0 if enet else 1.0
    for k in range(n):
        # step 0 starts from identical weights: fp32 kernels vs ATen -> 1e-5; later steps inherit Adam's
        # lr*sign(g)-like first updates (chaotic in the last bits of g) -> 2e-3
        tol = (2e-5 if enet else 1e-5) if k == 0 else 2e-3 * loose
        np.testing.assert_allclose([s.item() for s in log[k]["sup"]], g["sup"][k][:2], rtol=tol)
        np.testing.assert_allclose(log[k]["jsd"].item(), g["jsd"][k], rtol=max(tol, 1e-4), atol=1e-8)
        if adv:
            # FGSM sign() flips where |grad_x| ~ 0 change x_adv by 2*eps on isolated pixels
            np.testing.assert_allclose(log[k]["adv"].item(), g["adv"][k], rtol=2e-2, atol=1e-7)
    # _train_loop's return value: per-class (mean, std) of the 2-D Dice, [S, C, 2]
    assert dice_lab.shape == (2, int(g["C"]), 2)
    np.testing.assert_allclose(dice_lab[..., 0].numpy(), g["dice_lab"][..., 0], atol=2e-3 * loose)
    np.testing.assert_allclose(dice_unl[..., 0].numpy(), g["dice_unl"][..., 0], atol=2e-3 * loose)
    for j, seg in enumerate(tr.segmentators):
        names = list(g[f"m{j}_names"])
        sd = seg.torchnet.state_dict()
        df = np.stack([digest(sd[k]) for k in names])
        # conv biases in front of a BatchNorm have a mathematically-zero gradient; Adam turns its rounding noise
        # into +-lr steps of arbitrary sign (chaotic parity points): bound those by n*lr per element
        noise = np.array([enet and k.endswith(".bias") and not k.endswith(".1.bias") and "batch_norm" not in k
                          and not k.startswith("decoder.layers.5") or (enet and k.endswith("middle_block.0.1.bias"))
                          for k in names])
        numel = np.array([sd[k].numel() for k in names], dtype=np.float64)
        step_bound = 1.5 * n * 1e-3
        for col, mult in ((1, numel), (2, np.sqrt(numel)), (3, np.ones_like(numel))):   # abs-sum, l2, max-abs after the last step
            ref = g[f"m{j}_digest_final"][:, col]
            # Enet: BatchNorm betas start at 0 and sit at O(n*lr) after n Adam steps, so a relative tolerance alone is
            # meaningless for them: allow a fifth of the maximal Adam displacement on top
            atol = 1e-5 + (0.2 * n * 1e-3 * mult[~noise] if enet else 0.0)
            err = np.abs(df[~noise, col] - ref[~noise])
            # Running statistics after three chaotic Adam steps: 3 % for every BatchNorm; ONE running variance of the last
            # encoder block (the deepest, smallest sample: 2 x 8 x 8) was measured at 3.05 % -- at most one such outlier is
            # let through, and only up to 5 %.
            kept = np.array(names)[~noise]
            is_run = np.array([enet and "running_" in k for k in kept])
            rtol = np.where(is_run, 3e-2, 2e-3 * loose)
            bad = err > rtol * np.abs(ref[~noise]) + atol
            outliers = bad & is_run & (err <= 5e-2 * np.abs(ref[~noise]) + atol)
            if outliers.sum() <= 1:
                bad = bad & ~outliers
            assert not bad.any(), (col, [names[i] for i in np.flatnonzero(~noise)[bad]][:8], err[bad][:8], ref[~noise][bad][:8])
            assert np.all(np.abs(df[noise, col] - ref[noise]) <= step_bound * mult[noise] + 1e-6)
        st = seg.optimizer.state
        ea = np.stack([digest(st[p]["exp_avg"]) for p in seg.torchnet.parameters()])
        if not enet:
            np.testing.assert_allclose(ea[:, 2], g[f"m{j}_exp_avg_digest"][:, 2], rtol=2e-2, atol=1e-9)
        else:
            # early-layer Enet gradients are chaotic in the last bits of the forward (tests/test_enet_gpu.py: a 1e-6
            # perturbation moves them by tens of percent), and steps 2-3 start from Adam's sign-like first update:
            # the first moments are compared in aggregate only
            ref = g[f"m{j}_exp_avg_digest"][:, 2]
            assert np.all(np.isfinite(ea))
            assert abs(np.linalg.norm(ea[:, 2]) / np.linalg.norm(ref) - 1.0) < 0.1


def test_fused_and_generic_paths_agree(golden, tmp_path):
    """same step through (a) the fused kernels + one autograd.backward and (b) the public module
    APIs (Segmentator.predict, loss modules, FSGMGenerator, total.backward())"""
    g = golden("g5_step_unet_adv")
    outs = []
    for fused in (True, False):
        tr, lab, unl = _trainer(tmp_path, g, torch.float32, 1, fused=fused)
        for s in tr.segmentators:
            s.train()
        lb = [lab[i][0][0] for i in range(2)]
        out = tr._run_step([(lb[0][0], lb[0][1]), (lb[1][0], lb[1][1])], (unl[0][0][0], unl[0][0][1]), True, True, (0, 1))
        w = [digest(torch.cat([p.detach().flatten() for p in s.torchnet.parameters()])) for s in tr.segmentators]
        # Adam's first update moves every weight by lr * sign(g): the weights cannot show a wrong gradient scale, the first moments
        # (0.1 x the step's total gradient) do -- per parameter tensor, their l2 norm
        m = [np.array([digest(s.optimizer.state[p]["exp_avg"])[2] for p in s.torchnet.parameters()]) for s in tr.segmentators]
        outs.append((out, w, m))
    (a, wa, ma), (b, wb, mb) = outs
    np.testing.assert_allclose([s.item() for s in a["sup"]], [s.item() for s in b["sup"]], rtol=1e-6)
    np.testing.assert_allclose(a["jsd"].item(), b["jsd"].item(), rtol=1e-5)
    np.testing.assert_allclose(a["adv"].item(), b["adv"].item(), rtol=1e-4)
    for x, y in zip(wa, wb):
        np.testing.assert_allclose(x[1:], y[1:], rtol=1e-5)
    for x, y in zip(ma, mb):        # the UNet band of test_train_loop_fp32_matches_reference_golden
        assert x.shape == y.shape and len(x) > 10 and np.all(np.isfinite(x)) and x.max() > 1e-6
        np.testing.assert_allclose(x, y, rtol=2e-2, atol=1e-9)


def test_bf16_step_tracks_oracle(tmp_path, golden):
    """bf16 compute (the benchmarked configuration): losses of the first step vs the fp32 oracle"""
    g = golden("g5_step_unet_jsd")
    tr, lab, unl = _trainer(tmp_path, g, torch.bfloat16, 1)
    for s in tr.segmentators:
        s.train()
    lb = [lab[i][0][0] for i in range(2)]
    out = tr._run_step([(lb[0][0], lb[0][1]), (lb[1][0], lb[1][1])], (unl[0][0][0], unl[0][0][1]), True, False)
    # bf16 activations: logits carry ~2e-3 relative error -> losses within 1e-2
    np.testing.assert_allclose([s.item() for s in out["sup"]], g["sup"][0][:2], rtol=1e-2)
    np.testing.assert_allclose(out["jsd"].item(), g["jsd"][0], rtol=5e-2, atol=1e-6)
    for s in tr.segmentators:
        for p in s.torchnet.parameters():
            assert torch.isfinite(p).all()


def test_rccl_gradient_exchange_single_rank(tmp_path, golden):
    """The N>1 code path of bench.py on the one GPU a test box has: a world_size-1 RCCL process group, flat
    gradient all-reduce (SUM, async; 1/world in Adam) out of the flat buffers, per-model wait + fused Adam.  With one
    rank the exchange must leave the step bit-identical to the single-process step."""
    import os
    import torch.distributed as dist
    from dct_amd.ddp import FlatGradSync
    g = golden("g5_step_unet_jsd")
    res = []
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    created = False
    if not dist.is_initialized():
        dist.init_process_group(backend="nccl", rank=0, world_size=1)
        created = True
    try:
        for sync in (False, True):
            tr, lab, unl = _trainer(tmp_path, g, torch.bfloat16, 1)
            for s in tr.segmentators:
                s.train()
            if sync:
                tr.grad_sync = FlatGradSync(tr.segmentators)
            lb = [lab[i][0][0] for i in range(2)]
            tr._run_step([(lb[0][0], lb[0][1]), (lb[1][0], lb[1][1])], (unl[0][0][0], unl[0][0][1]), True, False)
            torch.cuda.synchronize()
            if sync:        # UNet gradients go out in three buckets per model from inside the backward pass
                assert tr.grad_sync.bucket_calls == 6
            res.append([torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu() for s in tr.segmentators])
    finally:
        if created:
            dist.destroy_process_group()
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("arch,H,pair,S", [("enet", 64, (0, 2), 3), ("unet", 176, (1, 2), 3), ("enet", 64, None, 4), ("enet", 64, None, 6)])
def test_multi_view_step_vs_oracle(tmp_path, arch, H, pair, S):
    """S = 3, 4, 6 co-training (the multi-view runs of script/ACDC/5_run_multiple_view.sh:27-33, script/GM/run_multiview.sh:2-6;
    BASELINE configs[4]): JSD over all S models, FGSM on a pair (a, b) -- given, or drawn as the reference draws it
    (cotraining_totalloss.py:230-236: np.random.choice) --, one backward, S Adam steps: fp32 fused path vs the oracle step."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B = 3, 1
    segs, omodels = [], []
    for seed in range(5, 5 + S):
        sd = _seeded_state(arch, C, seed)
        torch.manual_seed(seed)
        onet = oracle.build_net(arch, C, **({"dropout_p": 0.0} if arch == "unet" else {})).train()
        onet.load_state_dict(sd)
        arch_dict = {"name": arch, "num_classes": C, "compute_dtype": torch.float32}
        if arch == "unet":
            arch_dict["dropout_p"] = 0.0
        seg = Segmentator(arch_dict, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                          {"name": "StepLR", "step_size": 90, "gamma": 0.1})
        seg.torchnet.load_state_dict(sd)
        segs.append(seg)
        omodels.append(oracle.OracleModel.make(onet))
    lab = [FakeLoader(batches(61 + i, 1, B, H, C), B) for i in range(S)]
    unl = FakeLoader(batches(71, 1, B, H, C), B)
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                   adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=1)
    assert tr._fused_ok()
    for s in segs:
        s.train()
    if pair is None:
        np.random.seed(1234 + S)
        pair = tr._draw_adv_choice()
        assert 0 <= pair[0] < pair[1] < S
    lb = [(lab[i][0][0][0], lab[i][0][0][1]) for i in range(S)]
    ub = (unl[0][0][0], unl[0][0][1])
    out = tr._run_step(lb, ub, True, True, pair)
    ref = oracle.cotrain_step(omodels, lb, ub[0], True, True, lam_cot=0.5, lam_adv=0.05, eps=0.03, adv_choice=pair)
    np.testing.assert_allclose([s.item() for s in out["sup"]], [s.item() for s in ref["sup"]], rtol=2e-5)
    np.testing.assert_allclose(out["jsd"].item(), ref["jsd"].item(), rtol=1e-4)
    np.testing.assert_allclose(out["adv"].item(), ref["adv"].item(), rtol=3e-2)      # FGSM sign flips at |grad| ~ 0
    for seg, om in zip(segs, omodels):
        a = torch.cat([p.detach().flatten().cpu() for p in seg.torchnet.parameters()]).double()
        b = torch.cat([p.detach().flatten() for p in om.net.parameters()]).double()
        # the first Adam step moves every weight by +-lr whatever its gradient's size: a weight whose gradient is rounding noise
        # (|g| ~ 1e-9) may take the other sign, 2e-3 per flip -- 0.6 % of Enet's weights do at S = 4 (measured 1.05e-3 relative)
        assert ((a - b).norm() / b.norm()).item() < (1e-3 if S == 3 else 2e-3)


@pytest.mark.parametrize("arch,adv", [("unet", True), ("enet", False)])
def test_graph_replay_equals_eager_step_sequence(tmp_path, arch, adv):
    """trainer/step_graph.py: seven steps (two eager, the capture, four replays) with fresh batches every step, dropout on
    (UNet), a learning-rate change and a loss-weight change on the way must leave exactly the weights, Adam moments and
    step counts of seven eagerly launched steps -- i.e. nothing a step depends on was baked into the captured graph."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B, H, n = 3, 2, (176 if arch == "unet" else 64), 7
    res = []
    for use_graph in (False, True):
        segs = []
        for seed in (11, 12):
            torch.manual_seed(seed)
            seg = Segmentator({"name": arch, "num_classes": C, "compute_dtype": torch.bfloat16},
                              {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                              {"name": "StepLR", "step_size": 90, "gamma": 0.1})
            segs.append(seg)
        lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(2)]
        unl = FakeLoader(batches(91, n, B, H, C), B)
        crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        tr.use_hip_graph = use_graph
        for s in segs:
            s.train()
        sups = []
        for k in range(n):
            if k == 4:                          # a scheduler step between replays: lr and lambda_cot change
                for s in segs:
                    s.optimizer.param_groups[0]["lr"] = 3e-4
                tr.cot_scheduler.max_value = 0.25
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


@pytest.mark.parametrize("H,B_l,B_u,C", [(200, 3, 5, 2), (176, 1, 2, 4), (264, 2, 2, 3)])
def test_unet_bf16_step_odd_shapes(tmp_path, H, B_l, B_u, C):
    """Planner robustness: image sizes / batch sizes other than the benchmark's (GM 200 x 200, the 176 minimum, a
    non-multiple-of-16 size; ragged patches, runs and tiles everywhere): five bf16 steps (eager, capture, replays) stay
    finite and step 0's losses match the fp32 kernels on the same weights to bf16 accuracy."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    n = 5
    first = {}
    for dtype in (torch.float32, torch.bfloat16):
        segs = []
        for seed in (31, 32):
            torch.manual_seed(seed)
            segs.append(Segmentator({"name": "unet", "num_classes": C, "compute_dtype": dtype, "dropout_p": 0.0},
                                    {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                                    {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
        lab = [FakeLoader(batches(51 + i, n, B_l, H, C), B_l) for i in range(2)]
        unl = FakeLoader(batches(61, n, B_u, H, C), B_u)
        crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
        tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=list(range(1, C)),
                       cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                       adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                       adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
        for s in segs:
            s.train()
        steps = n if dtype == torch.bfloat16 else 1
        for k in range(steps):
            lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
            out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, True, (0, 1))
            vals = [float(v) for v in out["sup"]] + [float(out["jsd"]), float(out["adv"])]
            assert all(np.isfinite(v) for v in vals), (dtype, k, vals)
            if k == 0:
                first[dtype] = vals
    a, b = first[torch.float32], first[torch.bfloat16]
    np.testing.assert_allclose(b[:2], a[:2], rtol=2e-2)              # supervised losses
    np.testing.assert_allclose(b[2], a[2], rtol=0.25, atol=1e-7)      # JSD of two near-uniform predictions: tiny, relative noise is large
