"""HIP-graph replay of the fused co-training step.

The fused step (CoTrainer._run_step_fused) is a fixed launch sequence for fixed batch shapes: ~340 launches for
2 x UNet, ~5000 for 2 x Enet, each costing 15-20 us of Python + ctypes on the host -- more than the kernels take
on an MI355X, so the eager step is launch-bound.  Here the sequence is captured ONCE per step signature into a HIP
graph (torch.cuda.CUDAGraph == hipGraph on ROCm; the per-model streams fork and join inside the capture) and
replayed with one launch per step.

What makes the step replayable -- nothing in a launch may depend on a per-step host value:
  * Adam's bias-correction scalars and step count live on the device (optim.FusedAdam, dct_adam_flat_dev);
  * the dropout call counter lives on the device (dct_dropout_fwd_dev);
  * the loss weights lambda_cot / lambda_adv are read from a device tensor (the ``gscale`` argument of the loss
    backward kernels), refreshed only when a scheduler changes them;
  * the mini-batches are copied into static input buffers before each replay.
Host-side counters that the captured Python code advanced once (optimizer step count, dropout calls) are advanced
by the same amount after every replay, and the optimizers' "weights updated" callback to the networks is repeated (the UNet's
weight packs are keyed on the host: an evaluation or an eager step of another shape between two replays must repack).

A signature is captured after WARMUP eager steps (which are ordinary training steps), so lazy initialisation
(flat buffers, weight packs, kernel attributes) has happened and the capture sees the steady-state sequence.
Anything that re-allocates the weights, gradients or moments (load_state_dict, .to()) changes the signature and
leads to a new capture.

Two capture forms (step_route.plan_execution chooses; the step is then routed for that mode by step_route.plan_step):
  * ONE graph (UNet): the per-model streams fork and join inside the capture; only the model streams -- such a step is routed
    without pass streams (their cross-stream marks have crashed hipStreamEndCapture / hipGraphLaunch on ROCm 7.2);
  * a PROGRAM of per-stream graphs (trainer/stream_sched.py; Enet, 2 x UNet + FGSM, every data-parallel step): one hipGraphLaunch
    feeds one hardware queue, so chains that should overlap are captured as separate graphs and launched on their own streams,
    with the cross-stream waits and the host callbacks (gradient exchange) replayed between them.

Data parallelism: the RCCL all-reduces are never captured; they are host callbacks of the program (UNet: one per gradient bucket,
issued from inside the backward pass; Enet: one per model).  ``segmented_graphs=False`` falls back to two graphs -- [forwards,
losses, backward passes] and [optimizer steps] -- around one eager (un-bucketed) all-reduce per model.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .step_route import adv_settings, plan_step


def _is_refused_capture(err: BaseException) -> bool:
    """True for the errors HIP / torch raise when a stream capture is refused or invalidated ("operation not permitted when stream is
    capturing", "capturing stream has unjoined work", "... graph ..."), False for the library's own launch / argument errors
    ("dct_amd: ... failed"), which must reach the user."""
    msg = str(err).lower()
    if "dct_amd:" in msg and "captur" not in msg:
        return False
    return "captur" in msg or "graph" in msg


class _Captured(object):
    __slots__ = ("graph", "graph_opt", "program", "lab", "unl", "out", "counters")


class StepGraphCache(object):
    WARMUP = 2
    MAX_GRAPHS = 8

    def __init__(self, trainer):
        self.tr = trainer
        self._seen: Dict[tuple, int] = {}
        self._graphs: Dict[tuple, _Captured] = {}
        self._lam_dev: Optional[torch.Tensor] = None
        self._lam_host: Tuple[float, float] = (float("nan"), float("nan"))
        self.replays = 0
        self.captures = 0

    # ------------------------------------------------------------------------------ signature
    def _signature(self, lab, unl, train_jsd, train_adv, adv_choice, lam, execution, route) -> tuple:
        """What a capture is valid for: the route (every layout decision: a frozen dataclass, compared field by field), what the step
        computes, the batch shapes and the identity of every buffer the launches point into."""
        tr = self.tr
        sig: List = [execution, route, bool(train_jsd), bool(train_adv), tuple(adv_choice) if adv_choice is not None else None,
                     lam[0] != 0.0, lam[1] != 0.0]
        # the adversarial block: (generator, xi, eplision, ip) are launch arguments and a launch count, so another value is another
        # capture; VAT's seed and the address of its draw counter are launch arguments too (the counter's value is read on the device)
        if train_adv:
            adv = adv_settings(tr.adv_training_dict)
            noise = getattr(tr, "vat_noise", None) if adv[0] == "vat" else None
            sig.append(adv + ((noise.seed, noise.state(tr.device).data_ptr()) if noise is not None else ()))
        else:
            sig.append(None)
        for img, gt in lab:
            sig.append((tuple(img.shape), img.dtype, tuple(gt.shape), gt.dtype))
        if unl is not None:
            sig.append((tuple(unl[0].shape), unl[0].dtype))
        for seg in tr.segmentators:
            net, opt = seg.torchnet, seg.optimizer
            fp = net.flat_params
            sig.append((id(net), net.training, fp.version,
                        fp.flat.data_ptr() if fp.flat is not None else 0,
                        fp.gflat.data_ptr() if fp.gflat is not None else 0,
                        opt._m.data_ptr() if getattr(opt, "_m", None) is not None else 0,
                        getattr(net, "external_dropout_masks", None) is None,
                        bool(getattr(net, "record_dropout_masks", False)),
                        # the optimizer's guard: its record's address (0 when off) and the two switches are launch arguments, so
                        # switching it is another capture; max_grad_norm is read on the device, so changing it is not
                        opt._guard.data_ptr() if getattr(opt, "_guard", None) is not None and opt.guarded else 0,
                        getattr(opt, "max_grad_norm", None) is not None, bool(getattr(opt, "skip_nonfinite", False))))
        # the supervised criterion's launch arguments: another criterion (ignore_index, weight buffer; for CE + Dice its module type, the
        # two coefficients, mask, smooth and per_image; for the Tversky family also alpha, beta and gamma) is another capture; the weights
        # themselves are read on the device, so changing them in place is not
        sup = tr.criterions['sup']
        w = sup.device_weight(tr.device, tr.C)
        rule = sup.launch_args(tr.C) if hasattr(sup, "launch_args") else None
        sig.append((sup.ignore_index, w.data_ptr() if w is not None else 0, type(sup).__name__,
                    tuple(sorted(rule.items())) if rule is not None else None))
        # the consistency criterion: a pseudo-label one's type and launch arguments (teacher, threshold, eps: another value is another
        # capture); JSD_2D has none to tell apart, its entry is a constant
        cons = tr.criterions['jsd']
        sig.append((type(cons).__name__, tuple(sorted(cons.launch_args().items()))) if hasattr(cons, "launch_args") else None)
        return tuple(sig)

    def _lam(self) -> torch.Tensor:
        tr = self.tr
        lam = (float(tr.cot_scheduler.value), float(tr.adv_scheduler.value))
        if self._lam_dev is None or self._lam_dev.device != tr.device:
            self._lam_dev = torch.tensor(lam, dtype=torch.float32, device=tr.device)
            self._lam_host = lam
        elif lam != self._lam_host:              # once per epoch at most: two async fills
            self._lam_dev[0:1].fill_(lam[0])
            self._lam_dev[1:2].fill_(lam[1])
            self._lam_host = lam
        return self._lam_dev

    def _counters(self):
        out = []
        for seg in self.tr.segmentators:
            out.append((seg.optimizer, "_steps"))
            if hasattr(seg.torchnet, "_drop_calls"):
                out.append((seg.torchnet, "_drop_calls"))
        if getattr(self.tr, "vat_noise", None) is not None:     # (made before a VAT step is routed: CoTrainer._run_step)
            out.append((self.tr.vat_noise, "_calls"))
        return out

    # ------------------------------------------------------------------------------ run
    def run(self, lab, unl, train_jsd, train_adv, adv_choice, facts, execution, route) -> dict:
        """``route``: the step routed for ``execution`` (one_graph | program | ddp_two_graphs), which a capture issues and a replay
        repeats.  Warm-up steps (and shapes that stay uncaptured) are ordinary eager steps, routed as such."""
        tr = self.tr

        def eager():
            tr.last_route = plan_step(tr.plan, facts, "eager", tr._four_queues)
            return tr._run_step_fused(lab, unl, train_jsd, train_adv, adv_choice, tr.last_route, lam_dev=lam_dev)
        lam_dev = self._lam()
        for seg in tr.segmentators:
            if hasattr(seg.optimizer, "refresh_lr"):
                seg.optimizer.refresh_lr()
        sig = self._signature(lab, unl, train_jsd, train_adv, adv_choice, self._lam_host, execution, route)
        cap = self._graphs.get(sig)
        if cap is None:
            n = self._seen.get(sig, 0)
            self._seen[sig] = n + 1
            if n < self.WARMUP or len(self._graphs) >= self.MAX_GRAPHS:
                return eager()
            cap = self._capture(sig, lab, unl, train_jsd, train_adv, adv_choice, lam_dev, execution, route)
            if cap is None:
                return eager()
            first = True
        else:
            first = False
        # The mini-batches into the static input buffers: ONE multi-tensor copy per dtype instead of 2 S + 1 launches -- the replays are
        # pipelined, and whatever is queued between two graph launches sits on the critical path (tools/phase_stamps.py: 60 us between
        # one step's last optimizer and the next step's first kernel, with five copies and three result clones in it)
        dsts = [t for pair in cap.lab for t in pair] + ([cap.unl[0]] if cap.unl is not None else [])
        srcs = [t for pair in lab for t in pair] + ([unl[0]] if cap.unl is not None else [])
        try:
            torch._foreach_copy_(dsts, srcs, non_blocking=True)
        except (RuntimeError, TypeError, AttributeError):
            for d, s_ in zip(dsts, srcs):
                d.copy_(s_, non_blocking=True)
        if cap.program is not None:            # one graph per stream segment, launched on the segments' own streams
            cap.program.replay()
        else:
            cap.graph.replay()
        if cap.graph_opt is not None:          # data parallelism: exchange the gradients between the two graphs
            for i in range(len(tr.segmentators)):
                tr.grad_sync.begin(i)
            tr.grad_sync.finish()
            cap.graph_opt.replay()
        self.replays += 1
        if not first:                     # the capture pass already advanced the host counters once
            for (obj, name), d in zip(self._counters(), cap.counters):
                setattr(obj, name, getattr(obj, name) + d)
            # ... and told the networks that their weights were rewritten (UNet: drops the key of its weight packs).  The replay repacked
            # in front of its forward passes and updated the weights behind them: without this, packs that an evaluation between two
            # replays built (and keyed) would pass for current after the next replay -- in the following evaluation, and in an eager
            # step of another shape.  Host attributes only: nothing is launched between two replays.
            for seg in tr.segmentators:
                if hasattr(seg.optimizer, "repeat_step_callback"):
                    seg.optimizer.repeat_step_callback()
        o = cap.out
        # the small results are copied out (callers may keep them across steps) -- as ONE stacked tensor: one launch between two replays
        # instead of one per scalar; the prediction maps are the graph's static buffers, valid until the next step
        scalars = list(o["sup"]) + [o[k] for k in ("jsd", "adv") if torch.is_tensor(o[k])]
        vals = torch.stack([v.reshape(()) for v in scalars])
        n = len(o["sup"])
        rest = iter(vals[n:])
        return dict(sup=[vals[i] for i in range(n)],
                    jsd=next(rest) if torch.is_tensor(o["jsd"]) else o["jsd"],
                    adv=next(rest) if torch.is_tensor(o["adv"]) else o["adv"],
                    preds=o["preds"], unlab_probs=o["unlab_probs"])

    def _capture(self, sig, lab, unl, train_jsd, train_adv, adv_choice, lam_dev, execution, route) -> Optional[_Captured]:
        tr = self.tr
        cap = _Captured()
        cap.lab = [(torch.empty_like(img), torch.empty_like(gt)) for img, gt in lab]
        cap.unl = (torch.empty_like(unl[0]), None) if unl is not None else None
        before = [getattr(o, n) for o, n in self._counters()]
        side = [getattr(seg.torchnet, "wgrad_side_stream", None) for seg in tr.segmentators]
        for seg in tr.segmentators:          # a fork nested inside a forked stream crashes hipStreamEndCapture (ROCm 7.2)
            if (tr.model_streams or tr._use_segments()) and hasattr(seg.torchnet, "wgrad_side_stream"):   # (nor may a segment end with unjoined work)
                seg.torchnet.wgrad_side_stream = False
        for seg in tr.segmentators:          # the replays follow weight updates: the captured pass must pack the weights even if an
            if hasattr(seg.torchnet, "repack_in_next_pass"):     # evaluation has just done so (and a pass of its own would find them current)
                seg.torchnet.repack_in_next_pass()
        torch.cuda.synchronize(tr.device)
        graph = torch.cuda.CUDAGraph()
        cap.graph_opt = None
        cap.program = None
        # no garbage collection while a capture is open: a collected object of an earlier trainer (streams, events, graphs)
        # would be destroyed with HIP calls that are not permitted during capture
        import gc
        gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            if execution == "program":
                from .stream_sched import EagerSchedule, SegmentRecorder
                rec = SegmentRecorder(tr.device)
                tr._sched = rec
                try:
                    rec.start()
                    cap.out = tr._run_step_fused(cap.lab, cap.unl, train_jsd, train_adv, adv_choice, route, lam_dev=lam_dev)
                    cap.program = rec.finish()
                except RuntimeError as e:
                    # a capture the runtime refuses must not take the training down: nothing was launched while recording, the
                    # host counters the recorded pass advanced are put back, and this signature stays on eager launches
                    rec.abort()
                    tr._sched = EagerSchedule()
                    for (o, n), v in zip(self._counters(), before):
                        setattr(o, n, v)
                    for seg in tr.segmentators:      # weight packs "built" by recorded-only launches do not exist: rebuild next step
                        if hasattr(seg.torchnet, "mark_weights_updated"):
                            seg.torchnet.mark_weights_updated()
                    if not _is_refused_capture(e):
                        raise                         # an argument / kernel error is not a refused capture: do not hide it
                    self._seen[sig] = -(1 << 30)
                    import warnings
                    warnings.warn(f"dct_amd: capturing the step as a program of HIP graphs failed ({e}); this step shape runs eagerly")
                    return None
                except BaseException:
                    rec.abort()
                    raise
                finally:
                    tr._sched = EagerSchedule()
                graph = None
            else:
                # ONE graph: only the model streams fork inside it (the layout captured since round 1; the route for this mode has no
                # pass streams and no multi-queue layout: step_route.plan_step)
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    cap.out = tr._run_step_fused(cap.lab, cap.unl, train_jsd, train_adv, adv_choice, route, lam_dev=lam_dev)
                if execution == "ddp_two_graphs":
                    # no collective inside a capture: graph 1 ended after the backward passes (route.defer_optimizer), graph 2 holds the
                    # optimizer steps -- S small launches on the capture stream; the exchange between them leaves a SUM, the update folds its 1/world in
                    cap.graph_opt = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cap.graph_opt, capture_error_mode="thread_local"):
                        tr._optimizer_graph_phase(route)
        finally:
            if gc_was_on:
                gc.enable()
            for seg, s in zip(tr.segmentators, side):
                if s is not None:
                    seg.torchnet.wgrad_side_stream = s
        cap.graph = graph
        cap.counters = [getattr(o, n) - b for (o, n), b in zip(self._counters(), before)]
        for (o, n), d in zip(self._counters(), cap.counters):
            if n == "_drop_calls" and d % 2:       # the device counter's two words are used in turn (dct_dropout_fwd_dev): replays must stay in turn
                raise RuntimeError("dct_amd: a captured step must hold an even number of dropout launches per network")
        # a re-allocation during the capture (first gradient buffer, moments) would have changed the signature
        if self._signature(lab, unl, train_jsd, train_adv, adv_choice, self._lam_host, execution, route) != sig:
            raise RuntimeError("dct_amd: weights / gradients / Adam moments were (re)allocated while the step was being "
                               "captured; they would live in the graph's private pool")
        self._graphs[sig] = cap
        self.captures += 1
        return cap
