"""The seam of the fused co-training step: the logit gradient ``dl`` that ``CoTrainer`` hands to each network's ``plan_backward``, and the loss
values it reports, against a float64 restatement of the whole step in plain torch (tests/criteria_ref.py).

How the seam is recorded.  For ONE eager fused step (``use_hip_graph = False``) ``_Spy`` wraps every network instance's ``plan_forward`` and
``plan_backward`` and records, in call order: the input batch, the returned logits, and per backward call a clone of ``dl`` with ``need_dx`` /
``need_dw``.  ``plan_backward`` (arch/unet.py, arch/enet.py) is a plain host function that launches its kernels on the CURRENT stream, and
the layouts of trainer/cotraining_totalloss.py call it on a stream that is already ordered behind every writer of ``dl`` (the loss kernel of
the same stream, or a ``wait`` / ``wait_event`` on the JSD's and the forward pass's marks issued before the call) -- it could not read a
finished ``dl`` itself otherwise.  A ``clone()`` issued at the call, on that current stream and in front of the pass's own launches, therefore
sees the finished ``dl`` (and is not touched by whatever the pass does to its argument afterwards).  Enet runs with ``group_passes = False``:
inside a ``PassGroup`` launches are deferred and a torch clone would not be ordered with them (grouped against ungrouped is held
bit-identical by tests/test_stream_sched_gpu.py).

What is rebuilt.  From the recorded fp32 logits alone, as float64 leaves on the CPU:
    total = sum_i sup_i(labeled rows of model i) + lambda_cot * cons(unlabeled rows of all S)
            + lambda_adv * KL(softmax(adversarial logits of a) || softmax(clean logits of b over [lab_b; unl]).detach())
and, separately, the FGSM generator's criterion: ``sup`` over b's clean logits with [gt_b; first-maximum argmax of the unlabeled tail] as
targets, the mean over all those rows.  Every recorded ``dl / loss_scale`` must equal the autograd gradient of that total with respect to
the pass's logits element by element (the generator's ``need_dx`` call against the generator criterion's gradient), exactly 0.0 wherever
the reference gradient is exactly 0 (unlabeled rows at lambda_cot = 0, every channel of an ignored pixel, targets of a class of weight 0
under CE / focal), and the number and kind of backward calls per pass is what the step's definition implies.

Tolerances.  Every bound is the one the criterion's kernel test already derives as a function of the inputs, imported: ``focal_ref.Ref`` /
``ce_bounds``, ``_Bounds`` of test_dice_loss_gpu.py and ``pseudo_label_ref`` through ``criteria_ref``, ``_jsd_ref`` and ``_kl_ref`` of
test_loss_kernels_scale_gpu.py.  Every row of a pass carries exactly one term (labeled rows the supervised one, unlabeled rows the
consistency one; the adversarial and the generator's pass one each), so no sum of bounds arises.  No tolerance is measured, and nothing is
derived from the fused step's own output.  (A bound of 8 x the deviation of an fp32 CPU evaluation of the restatement from its float64 value was tried for the JSD and KL terms first.
It held for every gradient and is no bound for a value: over these cases that deviation of a mean over 1e4 .. 1e5 pixels lies anywhere
between 2.3e-10 and 3.5e-9 (JSD) and between 2.0e-11 and 4.5e-8 (KL) for one kind of input, by how the fp32 rounding errors happen to
cancel, while the kernels' values are a steady 4e-9 .. 2.6e-8 (JSD) and 2e-9 .. 2.8e-8 (KL) from float64 -- a tenth of one fp32 rounding
of the entropies of ~1.4 that either value is a difference of -- and missed 8 x the deviation in 3 of the first 4 JSD cases and in 3 KL
cases.  The kernel tests' own bounds put 5e-6 around these values.)

Near ties.  A pseudo-label teacher (or the generator's argmax) can sit on a rounding edge: such pixels (``NEAR``) are left out of the
element-wise check, widen the value bound by their largest possible contribution, and may be at most ``NEAR_SHARE`` of a case's pixels."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import criteria_ref as CR  # noqa: E402
from helpers import FakeLoader, blob_batches  # noqa: E402
from test_loss_kernels_scale_gpu import SUM_DEPTH, _check, _jsd_ref, _kl_ref  # noqa: E402
from test_pseudo_label_step_gpu import NEAR  # noqa: E402
from test_step_gpu import _seeded_state  # noqa: E402
from test_stream_sched_gpu import four_queues  # noqa: E402,F401  (the fixture)

DEV = "cuda:0"
C = 4
IGN = CR.IGN
U = CR.U
NEAR_SHARE = 1e-4
WEIGHT = [0.1, 1, 2.5, 0]           # tests/test_weighted_step_gpu.py's: a class of weight 0

SUP = {
    "ce": CR.Supervised("cross_entropy"),
    "ce_w": CR.Supervised("cross_entropy", weight=WEIGHT),
    "focal": CR.Supervised("focal", gamma=2.0, weight=WEIGHT),
    "ce_dice": CR.Supervised("ce_dice", weight=WEIGHT, classes=[1, 2, 3]),
    "ce_dice_pi": CR.Supervised("ce_dice", weight=WEIGHT, classes=[1, 2, 3], per_image=True),
    "dice_pi": CR.Supervised("dice", classes=[1, 2, 3], per_image=True),
}
# layout -> (arch, S, B_l, B_u, adversarial pair or None, expected route kind, joint pass)
LAYOUTS = {
    "unet_chain": ("unet", 2, 2, 2, (0, 1), "adv_chain", True),
    "unet_joint": ("unet", 2, 1, 3, None, "sequential", True),        # the B_l-against-(B_l + B_u) denominator case
    "unet_s3": ("unet", 3, 1, 1, (1, 2), "sequential", True),
    "enet_wide": ("enet", 2, 2, 2, (0, 1), "wide", False),
    "enet_s3": ("enet", 3, 2, 2, None, "wide", False),
}
# The networks are untrained: a UNet's confidences then lie within a few hundredths of 1 / C, and with some initialisations (seed 12: an
# estimated 1.8e-4 of the pixels) its two best classes sit within NEAR of each other far more often than NEAR_SHARE allows.  These seeds
# give networks whose best class is set apart (none of 123,904 pixels of the oracle's forward pass within 1e-4).
NET_SEEDS = {"unet": (11, 13, 14), "enet": (18, 20, 31)}
BOTH, NO_COT, NO_ADV = (0.5, 0.05), (0.0, 0.05), (0.5, 0.0)

Case = collections.namedtuple("Case", "layout sup cons tau lam dtype", defaults=(torch.float32,))
CASES = [
    # every layout: the plain pair and the two crossed pairs; lambda_cot = 0 / lambda_adv = 0 / both non-zero spread over them
    Case("unet_chain", "ce", "jsd", 0.0, BOTH), Case("unet_chain", "focal", "cps", 0.0, NO_COT),
    Case("unet_chain", "ce_dice_pi", "pseudo_label", 0.0, NO_ADV),
    Case("unet_joint", "ce", "jsd", 0.0, NO_COT), Case("unet_joint", "focal", "cps", 0.0, BOTH),
    Case("unet_joint", "ce_dice_pi", "pseudo_label", 0.0, BOTH),
    Case("unet_s3", "ce", "jsd", 0.0, NO_ADV), Case("unet_s3", "focal", "cps", 0.0, BOTH),
    Case("unet_s3", "ce_dice_pi", "pseudo_label", 0.0, NO_COT),
    Case("enet_wide", "ce", "jsd", 0.0, NO_COT), Case("enet_wide", "focal", "cps", 0.36, NO_ADV),
    Case("enet_wide", "ce_dice_pi", "pseudo_label", 0.34, BOTH),
    Case("enet_s3", "ce_dice_pi", "pseudo_label", 0.34, BOTH), Case("enet_s3", "focal", "cps", 0.0, BOTH),
    # each supervised criterion with JSD (cross_entropy: the plain pairs above)
    Case("unet_chain", "ce_w", "jsd", 0.0, BOTH), Case("unet_joint", "focal", "jsd", 0.0, BOTH),
    Case("enet_wide", "ce_dice", "jsd", 0.0, BOTH), Case("unet_s3", "dice_pi", "jsd", 0.0, BOTH),
    # each consistency criterion with plain cross entropy (jsd: the plain pairs above)
    Case("unet_chain", "ce", "cps", 0.0, BOTH), Case("enet_wide", "ce", "cps", 0.36, BOTH),
    Case("unet_joint", "ce", "pseudo_label", 0.0, BOTH), Case("enet_s3", "ce", "pseudo_label", 0.34, BOTH),
]
# the loss scale: each supervised and each consistency criterion once, forced to 4096, bit-equal to 4096 x the unscaled run
SCALE_CASES = [Case("enet_wide", "ce", "jsd", 0.0, BOTH), Case("unet_chain", "ce_w", "cps", 0.0, BOTH),
               Case("enet_wide", "focal", "cps", 0.36, BOTH), Case("unet_joint", "ce_dice", "pseudo_label", 0.0, BOTH),
               Case("enet_wide", "dice_pi", "pseudo_label", 0.34, BOTH)]
# fp16 Enet: the automatic loss scale reaching every supervised criterion's step kernel
F16_CASES = [Case("enet_wide", s, "jsd", 0.0, BOTH, torch.float16) for s in ("ce", "ce_w", "focal", "ce_dice", "dice_pi")]


def _id(c):
    lam = {BOTH: "both", NO_COT: "cot0", NO_ADV: "adv0"}[c.lam]
    return f"{c.layout}-{c.sup}-{c.cons}{c.tau:g}-{lam}" + ("-f16" if c.dtype == torch.float16 else "")


def _ignore_some(batch_list, seed):
    """About 3 % of the labeled pixels to ``ignore_index``: a contiguous band of rows plus scattered single pixels."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for [[img, gt], meta, names] in batch_list:
        gt = gt.clone()
        H = gt.shape[2]
        rows = max(1, round(0.025 * H))
        gt[:, :, H // 3:H // 3 + rows, :] = IGN
        gt[torch.rand(gt.shape, generator=g) < 0.005] = IGN
        share = (gt == IGN).double().mean().item()
        assert 0.02 < share < 0.04, share
        out.append([[img, gt], meta, names])
    return out


def _trainer(tmp_path, case, loss_scale=None):
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    from dct_amd.loss import get_loss_fn
    arch, S, B_l, B_u, pair, _, _ = LAYOUTS[case.layout]
    H = 176 if arch == "unet" else 64
    segs = []
    for i in range(S):
        arch_dict = {"name": arch, "num_classes": C, "compute_dtype": case.dtype}
        if arch == "unet":
            arch_dict["dropout_p"] = 0.0
        seg = Segmentator(arch_dict, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1})
        seg.torchnet.load_state_dict(_seeded_state(arch, C, NET_SEEDS[arch][i]))
        segs.append(seg)
    lab = [FakeLoader(_ignore_some(blob_batches(81 + i, 1, B_l, H, C), 181 + i), B_l) for i in range(S)]
    unl = FakeLoader(blob_batches(91, 1, B_u, H, C), B_u)
    crit = {"sup": SUP[case.sup].module(), "jsd": CR.Consistency(case.cons, case.tau).module(), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2, 3],
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": case.lam[0]},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": case.lam[1]},
                   adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=1)
    tr.plan.use_hip_graph = False
    tr.plan.group_passes = False
    tr.force_loss_scale = loss_scale
    for s in segs:              # gradient buffers and moments exist before the step: the first step takes the route of every later one
        s.train()
        s.torchnet.flat_params.ensure()
        s.torchnet.flat_params.ensure_grads()
        s.optimizer._ensure_state()
    return tr, lab, unl


class _Spy:
    """Wraps ``plan_forward`` / ``plan_backward`` of every network instance; ``passes``: one record per forward call, in call order."""

    def __init__(self, nets):
        self.passes = []
        for i, net in enumerate(nets):
            self._wrap(i, net)

    def _wrap(self, i, net):
        fwd, bwd = net.plan_forward, net.plan_backward

        def plan_forward(x, *a, **k):
            lp, tape = fwd(x, *a, **k)
            self.passes.append(dict(model=i, B=int(x.shape[0]), x=x, logits=lp, tape=tape, bwd=[]))
            return lp, tape

        def plan_backward(tape, dl, need_dx=False, need_dw=True, **k):
            rec = [r for r in self.passes if r["tape"] is tape]
            assert len(rec) == 1, "plan_backward on a tape no recorded plan_forward returned"
            assert dl.shape == rec[0]["logits"].shape and dl.dtype == torch.float32
            rec[0]["bwd"].append(dict(dl=dl.clone(), need_dx=bool(need_dx), need_dw=bool(need_dw)))     # on the current stream, at the call
            return bwd(tape, dl, need_dx=need_dx, need_dw=need_dw, **k)

        net.plan_forward, net.plan_backward = plan_forward, plan_backward


def _run(tmp_path, case, loss_scale=None):
    """One eager fused step under the spy -> (trainer, step output on the CPU, passes with roles, the batches)."""
    arch, S, B_l, B_u, pair, kind, joint = LAYOUTS[case.layout]
    tr, lab, unl = _trainer(tmp_path, case, loss_scale)
    assert tr._fused_ok()
    spy = _Spy([s.torchnet for s in tr.segmentators])
    lb = [(lab[i][0][0][0], lab[i][0][0][1]) for i in range(S)]
    ub = (unl[0][0][0], unl[0][0][1])
    out = tr._run_step(lb, ub, True, pair is not None, pair)
    torch.cuda.synchronize()
    r = tr.last_route
    want_scale = loss_scale if loss_scale is not None else (
        float(2 ** max(10, (B_l * lb[0][0].shape[2] * lb[0][0].shape[3] - 1).bit_length())) if case.dtype == torch.float16 else 1.0)
    assert (r.kind, r.joint_pass, r.loss_scale) == (kind, joint, want_scale), (r.kind, r.joint_pass, r.loss_scale)
    assert tr._step_graphs is None
    # the role of every pass: the generator's is the one whose backward asks for the input gradient; the others by their input
    for p in spy.passes:
        x, i = p["x"].cpu(), p["model"]
        p["logits"] = p["logits"].detach().float().cpu()
        for b in p["bwd"]:
            b["dl"] = b["dl"].cpu()
        if any(b["need_dx"] for b in p["bwd"]):
            p["role"] = "gen"
        elif x.shape[0] == B_l and torch.equal(x, lb[i][0]):
            p["role"] = "lab"
        elif x.shape[0] == B_u and torch.equal(x, ub[0]):
            p["role"] = "unl"
        elif x.shape[0] == B_l + B_u and torch.equal(x, torch.cat((lb[i][0], ub[0]))):
            p["role"] = "joint"
        else:
            p["role"] = "adv"
        del p["x"], p["tape"]
    vals = dict(sup=[float(v) for v in out["sup"]], jsd=float(out["jsd"]), adv=float(out["adv"]) if pair is not None else None,
                kept=float(tr.criterions["jsd"].last_kept) if case.cons != "jsd" else None)
    return tr, vals, spy.passes, lb, ub


def _expect_calls(case, passes):
    """The number and kind of passes and backward calls per model that the step's definition implies."""
    arch, S, B_l, B_u, pair, kind, joint = LAYOUTS[case.layout]
    lam_cot, lam_adv = case.lam
    dw, dx = [(False, True)], [(True, False)]
    for i in range(S):
        want = {"joint": dw} if joint else {"lab": dw, "unl": dw if lam_cot != 0 else []}
        if pair is not None and i == pair[1]:
            want["gen"] = dx
        if pair is not None and i == pair[0]:
            want["adv"] = dw if lam_adv != 0 else []        # no adversarial weight-gradient pass at lambda_adv = 0
        got = [p for p in passes if p["model"] == i]
        assert sorted(p["role"] for p in got) == sorted(want), (i, [p["role"] for p in got])
        for p in got:               # (a list of at most one call: no pass is issued twice)
            assert [(b["need_dx"], b["need_dw"]) for b in p["bwd"]] == want[p["role"]], (i, p["role"], p["bwd"])
            assert p["B"] == {"lab": B_l, "unl": B_u}.get(p["role"], B_l + B_u)


def _by_role(passes, i, role):
    (p,) = [p for p in passes if p["model"] == i and p["role"] == role]
    return p


def _check_rows(what, got, ref, bound, skip=None):
    """|got - ref| <= bound element by element, exactly 0.0 where the reference is exactly 0; ``skip`` [rows] bool: rows left out."""
    got, ref = got.double().reshape(-1, C), ref.reshape(-1, C)
    bound = bound.reshape(-1, C) if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    if skip is not None:
        got, ref, bound = got[~skip], ref[~skip], bound[~skip]
    zero = ref == 0
    assert (got[zero] == 0).all(), f"{what}: {int((got[zero] != 0).sum())} elements are not exactly 0 where the reference is"
    worst = ((got - ref).abs() / bound.clamp(min=1e-300))[~zero]
    print(f"    {what}: {ref.numel()} elements, {int(zero.sum())} exactly 0, max |err| / bound {worst.max().item() if worst.numel() else 0.0:.3f}")
    _check(got, ref, bound, what)


def _verify(case, vals, passes, lb, ub, scale):
    arch, S, B_l, B_u, pair, kind, joint = LAYOUTS[case.layout]
    lam_cot, lam_adv = case.lam
    sup, cons = SUP[case.sup], CR.Consistency(case.cons, case.tau)
    _expect_calls(case, passes)
    lab_p = [_by_role(passes, i, "joint" if joint else "lab") for i in range(S)]
    unl_p = lab_p if joint else [_by_role(passes, i, "unl") for i in range(S)]
    for p in passes:
        p["leaf"] = p["logits"].double().requires_grad_(True)
    gts = [lb[i][1][:, 0] for i in range(S)]

    def lab_rows(p, leaf=True):
        return (p["leaf"] if leaf else p["logits"])[:B_l]

    def unl_rows(p, leaf=True):
        x = p["leaf"] if leaf else p["logits"]
        return x[B_l:] if joint else x

    # ---- the supervised terms
    total = 0.0
    for i in range(S):
        v = sup.value(lab_rows(lab_p[i]), gts[i])
        tol, gb = sup.bounds(lab_rows(lab_p[i], leaf=False), gts[i])
        print(f"  sup[{i}] {vals['sup'][i]!r} ref {v.item()!r} err {abs(vals['sup'][i] - v.item()):.3e} of {tol:.3e}")
        assert abs(vals["sup"][i] - v.item()) <= tol, ("sup", i, vals["sup"][i], v.item(), tol)
        lab_p[i]["lab_bound"] = gb
        total = total + v
    # ---- the consistency term over the unlabeled rows of all S
    x32u = [unl_rows(p, leaf=False) for p in unl_p]
    P = x32u[0].reshape(-1, C).shape[0]
    near = torch.zeros(P, dtype=torch.bool)
    if case.cons == "jsd":
        # tests/test_loss_kernels_scale_gpu.py::test_jsd_at_scale's bounds (``_jsd_ref``: per pixel; the gradient's for a factor 1 / P)
        jmap, jb, _, jgb, _ = _jsd_ref([x.reshape(-1, C) for x in x32u], C)
        cv = CR.jsd([unl_rows(p) for p in unl_p])
        assert abs(jmap.mean().item() - cv.item()) <= 1e-12
        ctol = (jb.sum().item() + SUM_DEPTH * U * jmap.abs().sum().item()) / P + 2 * U * abs(cv.item())
        cgb = [abs(lam_cot) * gb + 1e-30 for gb in jgb]
    else:
        n, kept, near = cons.decide(x32u, NEAR)
        assert int(near.sum()) <= NEAR_SHARE * P, f"{int(near.sum())} of {P} unlabeled pixels within {NEAR} of a tie or of tau: change the seed"
        q = [torch.from_numpy(CR.softmax32(x)).max(1).values for x in x32u]
        print(f"  {case.cons} tau={case.tau}: confidences {min(v.min().item() for v in q):.3f} .. {max(v.max().item() for v in q):.3f}, "
              f"kept {vals['kept']!r} ref {kept!r}, {int(near.sum())} near-tie pixels of {P}")
        if case.tau > 0:
            assert 0.05 < kept < 0.95, kept                 # the threshold sits inside the case's confidence range
        else:
            assert kept == 1.0
        # whole numbers summed in fp32 (exact below 2^24) and one fp32 division; a near-tie pixel may move its T of the P T teacher terms
        assert abs(vals["kept"] - kept) <= 2 * U * kept + int(near.sum()) / P, (vals["kept"], kept)
        cv = cons.value([unl_rows(p) for p in unl_p], n)
        ctol, cgb = cons.bounds(x32u, n, lam_cot)
        ctol += cons.near_value_slack(x32u, near)
    print(f"  cons {vals['jsd']!r} ref {cv.item()!r} err {abs(vals['jsd'] - cv.item()):.3e} of {ctol:.3e}")
    assert abs(vals["jsd"] - cv.item()) <= ctol, ("cons", vals["jsd"], cv.item(), ctol)
    total = total + lam_cot * cv
    # ---- the adversarial term and the generator's criterion
    if pair is not None:
        a, b = pair
        adv_p, gen_p = _by_role(passes, a, "adv"), _by_role(passes, b, "gen")
        y32 = gen_p["logits"]
        # tests/test_loss_kernels_scale_gpu.py::test_kl_at_scale's bounds (``_kl_ref``: per pixel; the gradient's for the factor lambda_adv / P)
        Pa = y32.reshape(-1, C).shape[0]
        kmap, kb, _, agb, _, _ = _kl_ref(adv_p["logits"].reshape(-1, C), y32.reshape(-1, C), C, lam_adv / Pa)
        av = CR.kl(adv_p["leaf"], gen_p["leaf"].detach())
        assert abs(kmap.mean().item() - av.item()) <= 1e-12
        atol = (kb.sum().item() + SUM_DEPTH * U * kmap.abs().sum().item()) / Pa + 2 * U * abs(av.item())
        print(f"  adv {vals['adv']!r} ref {av.item()!r} err {abs(vals['adv'] - av.item()):.3e} of {atol:.3e}")
        assert abs(vals["adv"] - av.item()) <= atol, ("adv", vals["adv"], av.item(), atol)
        total = total + lam_adv * av
        tail = y32[B_l:].reshape(-1, C)
        t_gen = torch.cat((gts[b].reshape(-1), CR.first_max(tail))).reshape(B_l + B_u, *gts[b].shape[1:])
        top = torch.softmax(tail, 1).double().topk(2, dim=1).values
        gen_near = torch.cat((torch.zeros(gts[b].numel(), dtype=torch.bool), (top[:, 0] - top[:, 1]) < NEAR))
        assert int(gen_near.sum()) <= NEAR_SHARE * gen_near.numel(), f"{int(gen_near.sum())} generator pixels within {NEAR} of an argmax tie: change the seed"
        gen_total = sup.value(gen_p["leaf"], t_gen)
        _, gen_gb = sup.bounds(y32, t_gen)
        (gen_ref,) = torch.autograd.grad(gen_total, gen_p["leaf"])
    grads = torch.autograd.grad(total, [p["leaf"] for p in passes], allow_unused=True)
    # ---- every recorded dl / loss_scale against the gradient of the total with respect to that pass's logits
    checked = 0
    for p, g in zip(passes, grads):
        for bw in p["bwd"]:
            dl = bw["dl"].double() / scale
            what = f"model {p['model']} {p['role']} pass"
            assert torch.isfinite(dl).all(), what
            if p["role"] == "gen":
                _check_rows(what, dl, gen_ref, gen_gb, skip=gen_near)
            elif p["role"] == "adv":
                _check_rows(what, dl, g, agb)
            else:
                g = torch.zeros_like(p["leaf"]) if g is None else g
                i = p["model"]
                if p["role"] in ("lab", "joint"):
                    _check_rows(what + " labeled rows", dl[:B_l], g[:B_l], p["lab_bound"])
                if p["role"] in ("unl", "joint"):
                    rows = slice(B_l, None) if joint else slice(None)
                    bound = cgb[i] if lam_cot != 0 else 0.0
                    _check_rows(what + " unlabeled rows", dl[rows], g[rows], bound, skip=near)
            checked += 1
    assert checked == sum(len(p["bwd"]) for p in passes) and checked >= S
    return passes


@pytest.mark.parametrize("case", CASES + F16_CASES, ids=_id)
def test_step_seam_matches_float64_step(tmp_path, four_queues, case):
    """One eager fused step: route, loss values, kept fraction, the backward calls issued and every ``dl / loss_scale`` against the
    float64 step rebuilt from the recorded logits (module docstring).  ``plan_backward`` launches on the current stream, which the
    layouts order behind every writer of ``dl`` before they call it, so the clone taken at the call sees the finished ``dl``."""
    tr, vals, passes, lb, ub = _run(tmp_path, case)
    print(f"{_id(case)}: route {tr.last_route.kind} joint {tr.last_route.joint_pass} loss scale {tr.last_route.loss_scale}")
    _verify(case, vals, passes, lb, ub, tr.last_route.loss_scale)


@pytest.mark.parametrize("case", SCALE_CASES, ids=_id)
def test_forced_loss_scale_is_exact_at_the_seam(tmp_path, four_queues, case):
    """``force_loss_scale = 4096``: the same logits, the same loss values, and every recorded ``dl`` bit-equal to 4096 x the unscaled run's
    (whose values are normal numbers: a subnormal would have lost bits the scaled run keeps); the unscaled run is held to the float64
    step like every other case."""
    SCALE = 4096.0
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    tr, vals, passes, lb, ub = _run(tmp_path / "a", case)
    _verify(case, vals, passes, lb, ub, 1.0)
    tr2, vals2, passes2, _, _ = _run(tmp_path / "b", case, SCALE)
    assert tr2.last_route.loss_scale == SCALE and vals2 == vals
    assert [(p["model"], p["role"]) for p in passes] == [(p["model"], p["role"]) for p in passes2]
    n = 0
    for p, p2 in zip(passes, passes2):
        assert torch.equal(p["logits"], p2["logits"])
        assert len(p["bwd"]) == len(p2["bwd"])
        for bw, bw2 in zip(p["bwd"], p2["bwd"]):
            d = bw["dl"]
            assert not ((d != 0) & (d.abs() < 2.0 ** -126)).any(), "subnormals in the unscaled gradient"
            assert torch.equal(bw2["dl"], d * SCALE), (p["model"], p["role"], (bw2["dl"] - d * SCALE).abs().max().item())
            n += 1
    assert n >= LAYOUTS[case.layout][1]
