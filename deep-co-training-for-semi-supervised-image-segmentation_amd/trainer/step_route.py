"""The route of one co-training step: every layout decision, taken once, before anything is launched (table: DESIGN.md 4.3).

Pure Python over plain values -- no torch, no HIP -- so the decision table is tested on the CPU (tests/test_host_logic_cpu.py).
``CoTrainer._step_facts`` gathers a ``StepFacts`` once per ``_run_step`` call; from it and the ``ExecutionPlan`` switches
``plan_execution`` says how the step is replayed and ``plan_step`` what ONE issue of it does under a given mode (a warm-up step is
issued under "eager", a capture under the mode ``plan_execution`` returned): a ``StepRoute``, which the layouts of
trainer/cotraining_totalloss.py follow without asking again and which is the captured step's signature (trainer/step_graph.py).
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Optional, Tuple

MAX_FUSED_MODELS = 8


@dataclasses.dataclass(frozen=True)
class NetFacts:
    """Fields named like a network attribute hold ``bool(getattr(net, name, False))`` (``NET_ATTRS``)."""
    plan_net: bool = False                      # flat_params and plan_forward present: the fused step can drive it
    batch_independent: bool = False
    supports_grad_overwrite: bool = False
    supports_pass_streams: bool = False
    supports_deferred_running_stats: bool = False
    supports_pass_groups: bool = False
    supports_forward_reuse: bool = False
    prefers_segmented_graphs: bool = False
    training: bool = True
    grad_buckets: bool = False                  # grad_bucket_ranges present: data parallelism hands buckets out of the backward pass
    grads_attached: bool = False
    dropout_masks_set: bool = False             # external_dropout_masks is not None
    fp16: bool = False


NET_ATTRS = tuple(f.name for f in dataclasses.fields(NetFacts))[1:9]


@dataclasses.dataclass(frozen=True)
class StepFacts:
    S: int
    nets: Tuple[NetFacts, ...]
    train_jsd: bool = False
    train_adv: bool = False
    adv_choice: Optional[Tuple[int, int]] = None
    unlabeled: bool = False                     # an unlabeled batch is present
    labeled_shapes_equal: bool = True
    labeled_equals_unlabeled: bool = False      # ... and equal to the unlabeled batch's shape
    labeled_pixels: int = 0                     # B * H * W of a labeled batch (fp16 loss scale)
    lam_cot_zero: bool = False
    lam_adv_zero: bool = False
    gpu: bool = False
    fused_criteria: bool = False
    ddp: bool = False
    optimizers_graphable: bool = False
    group_max: int = 0                          # members the library packs into one grouped launch
    adv_generator: str = "fgsm"                 # who makes the adversarial examples: fgsm | vat (adv_settings)


@dataclasses.dataclass(frozen=True)
class StepRoute:
    kind: str = "sequential"                    # sequential | wide | wide_grouped | adv_chain
    adv_chain_eligible: bool = False            # two batch-independent nets + FGSM (before the queue probe): such steps replay as a program
    joint_pass: bool = False                    # labeled + unlabeled batch as ONE pass per network
    model_streams: bool = False
    pass_streams: Tuple[bool, ...] = ()         # per model: two backward-pass streams
    early_backward: Tuple[bool, ...] = ()       # per model: labeled / unlabeled backward passes start beside the adversarial block
    group_one: bool = False
    leaf_offload: bool = False
    share_fgsm_encoder: bool = False
    late_b: int = 0                             # adv_chain: model b's backward behind the JSD (0), the adversarial batch (1), a's adversarial forward (2)
    overwrite: Tuple[str, ...] = ()             # per model: none (zero_grad + accumulate) | first (pass overwrites) | buffers (sum of pass buffers)
    exchange: Tuple[str, ...] = ()              # per model: none | model | buckets (from inside the backward pass) | two_graphs (between them)
    defer_optimizer: bool = False               # the step ends after the backward passes (first of two graphs)
    loss_scale: float = 1.0


ADV_GENERATORS = ("fgsm", "vat")


def adv_settings(adv_training_dict) -> Tuple[str, Optional[float], float, Optional[int]]:
    """``CoTrainer.adv_training_dict`` as (generator, xi, eplision, ip), validated: what the adversarial block of a step is issued
    with, and part of a captured step's signature.  'fgsm' (the default): eplision is the per-pixel step (0.05), xi and ip are None.
    'vat' (utils/AEGenerator.py::VATGenerator): eplision is the L2 radius per image (10), xi the probe radius (10), ip the number of
    power iterations (1).  ValueError for an unknown generator and for an xi, eplision or ip that is not positive."""
    d = dict(adv_training_dict or {})
    gen = d.get("generator", "fgsm")
    if gen not in ADV_GENERATORS:
        raise ValueError(f"dct_amd: adv_training_dict['generator'] is {gen!r}; known generators: {', '.join(ADV_GENERATORS)}")
    vat = gen == "vat"

    def positive(name, default):
        v = float(d.get(name, default))
        if not (v > 0.0) or v == float("inf"):
            raise ValueError(f"dct_amd: adv_training_dict[{name!r}] must be positive and finite, got {d.get(name)!r}")
        return v
    eps = positive("eplision", 10.0 if vat else 0.05)
    if not vat:
        return gen, None, eps, None
    xi = positive("xi", 10.0)
    ip = d.get("ip", 1)
    if isinstance(ip, bool) or int(ip) != ip or int(ip) < 1:
        raise ValueError(f"dct_amd: adv_training_dict['ip'] must be a whole number >= 1, got {ip!r}")
    return gen, xi, eps, int(ip)


def fused(facts: StepFacts) -> bool:
    return bool(facts.gpu and facts.fused_criteria and all(n.plan_net for n in facts.nets) and facts.S <= MAX_FUSED_MODELS)


def adv_chain_eligible(plan, facts: StepFacts) -> bool:
    c = facts.adv_choice
    if facts.train_adv and facts.adv_generator != "fgsm":
        return False            # the layout is scheduled around FGSM's single forward pass and its tape; VAT has 1 + ip passes on model b
    return bool(plan.adv_chain_layout and facts.train_jsd and facts.train_adv and facts.unlabeled and c is not None and
                facts.S == 2 and c[0] != c[1] and plan.batch_lab_unlab and plan.model_streams and not facts.ddp and
                all(n.batch_independent and n.supports_grad_overwrite and not n.dropout_masks_set for n in facts.nets))


def segmented(plan, facts: StepFacts, eligible: bool) -> bool:
    """A program of per-stream graphs (True) or one graph with forked streams inside."""
    if plan.segmented_graphs is not None:
        return bool(plan.segmented_graphs)
    # two batch-independent nets + FGSM: the adversarial chain gets a hardware queue; data parallelism: the gradient exchanges are
    # host callbacks BETWEEN graph segments; else by network
    return bool(eligible or (facts.ddp and plan.ddp_segmented_graph) or any(n.prefers_segmented_graphs for n in facts.nets))


def plan_execution(plan, facts: StepFacts) -> str:
    """generic | eager | one_graph | program | ddp_two_graphs."""
    if not fused(facts):
        return "generic"
    # replay needs every per-step scalar on the device (only the fused Adam keeps its step count / lr there); the RCCL all-reduces
    # are never captured: under data parallelism the step is a program whose exchanges are host callbacks, or two graphs around them
    if not (plan.use_hip_graph and facts.optimizers_graphable and (not facts.ddp or plan.ddp_segmented_graph) and
            all(n.training for n in facts.nets)):
        return "eager"
    if segmented(plan, facts, adv_chain_eligible(plan, facts)):
        return "program"
    return "ddp_two_graphs" if facts.ddp else "one_graph"


def _loss_scale(plan, facts: StepFacts) -> float:
    # fp16 networks: per-pixel gradients of a mean over ~1e6 pixels sit in half's subnormal range, so every loss gradient is scaled
    # by a power of two (>= the pixel count of a labeled batch) and the optimizers divide it out again (include/dct.h, DCT_F16).
    # 1.0 -- and bit-identical arithmetic -- for bf16 / fp32 networks.
    if plan.force_loss_scale is not None:
        return float(plan.force_loss_scale)
    if any(n.fp16 for n in facts.nets):
        return float(2 ** min(24, max(10, (facts.labeled_pixels - 1).bit_length())))
    return 1.0


def plan_step(plan, facts: StepFacts, mode: str, four_queues: Callable[[], bool]) -> StepRoute:
    """What one issue of the step does under ``mode`` (eager | one_graph | program | ddp_two_graphs).  ``four_queues`` (the
    hardware-queue probe) is asked last, and only when a layout that needs four queues is otherwise eligible."""
    eligible = adv_chain_eligible(plan, facts)
    nets, S = facts.nets, facts.S
    off = (False,) * S
    if not fused(facts):        # the generic step: one backward through autograd, zero_grad before it, one exchange per model behind it
        return StepRoute(adv_chain_eligible=eligible, pass_streams=off, early_backward=off, overwrite=("none",) * S,
                         exchange=("model" if facts.ddp else "none",) * S)
    # ONE graph being captured: only the model streams fork inside it.  Pass streams, the JSD's join into a forked stream (wide) and
    # the joins of the adversarial-chain layout add marks that forked streams wait for; hipStreamEndCapture / hipGraphLaunch of such
    # captures have crashed on ROCm 7.2, and the sequential accumulation they replace is bit-identical
    one_graph = mode in ("one_graph", "ddp_two_graphs")
    two_graphs = mode == "ddp_two_graphs"
    ddp = facts.ddp and not two_graphs                  # exchanges issued from inside the step
    model_streams = bool(plan.model_streams and S >= 2)
    pass_on = bool(model_streams and plan.pass_streams and not one_graph)
    jsd = facts.train_jsd and facts.unlabeled
    # networks whose samples do not interact (UNet: no BatchNorm) run the labeled and the unlabeled batch as ONE pass
    joint = bool(jsd and plan.batch_lab_unlab and all(n.batch_independent and not n.dropout_masks_set for n in nets))
    ready = all(n.training and n.grads_attached for n in nets)
    adv_pass = facts.train_adv and not facts.lam_adv_zero
    common = dict(adv_chain_eligible=eligible, joint_pass=joint, model_streams=model_streams, defer_optimizer=two_graphs,
                  loss_scale=_loss_scale(plan, facts))

    # (the four-queue layouts give the adversarial chain's queue to FGSM's one forward + input-gradient pass: another generator stays sequential)
    fgsm = not facts.train_adv or facts.adv_generator == "fgsm"

    if (fgsm and plan.wide_forward and pass_on and jsd and not joint and
            all(n.supports_deferred_running_stats and n.supports_pass_streams for n in nets) and ready and four_queues()):
        grouped = bool(plan.group_passes and all(n.supports_pass_groups for n in nets) and facts.labeled_shapes_equal and S <= facts.group_max)
        return StepRoute(kind="wide_grouped" if grouped else "wide", pass_streams=(True,) * S, early_backward=off,
                         group_one=bool(grouped and plan.group_one and facts.labeled_equals_unlabeled and 2 * S <= facts.group_max),
                         leaf_offload=bool(grouped and plan.leaf_offload and adv_pass),
                         overwrite=("buffers",) * S, exchange=("model" if ddp else "none",) * S, **common)

    if joint and eligible and model_streams and plan.grad_overwrite and not one_graph and ready and four_queues():
        b = nets[facts.adv_choice[1]]
        late = int(plan.adv_chain_late_b)
        return StepRoute(kind="adv_chain", pass_streams=off, early_backward=off,
                         share_fgsm_encoder=bool(plan.fgsm_shares_encoder and b.supports_forward_reuse and b.training),
                         late_b=2 if late == 2 else (1 if late else 0),
                         overwrite=("first",) * S, exchange=("none",) * S, **common)

    # sequential: per model, how many backward passes are left when the backward phase starts
    n_cot = 1 if joint else 1 + int(bool(jsd and not facts.lam_cot_zero))
    a = facts.adv_choice[0] if facts.train_adv else None
    early_on = bool(facts.train_adv and plan.early_backward and facts.train_jsd and pass_on)
    early, overwrite, exchange = [], [], []
    for i, n in enumerate(nets):
        e = bool(early_on and n.supports_pass_streams and n.grads_attached and not (ddp and n.grad_buckets))
        left = int(adv_pass and i == a) + (0 if e else n_cot)
        parallel = e or bool(pass_on and n.supports_pass_streams and 1 < left <= 3 and n.grads_attached)
        early.append(e)
        # pass-parallel models write the whole gradient buffer as the sum of their pass buffers; nets whose every parameter gets a
        # gradient in every pass let the first pass overwrite: neither needs the zero fill
        overwrite.append("buffers" if parallel else
                         "first" if (plan.grad_overwrite and n.supports_grad_overwrite and n.grads_attached) else "none")
        exchange.append("two_graphs" if (two_graphs and facts.ddp) else "none" if not ddp else
                        "buckets" if (n.grad_buckets and not parallel) else "model")
    return StepRoute(kind="sequential", pass_streams=tuple(bool(pass_on and n.supports_pass_streams) for n in nets), early_backward=tuple(early),
                     overwrite=tuple(overwrite), exchange=tuple(exchange), **common)
