"""trainer/stream_sched.py: the fused step captured as a PROGRAM of per-stream HIP graphs, the early backward passes beside the
adversarial block, and the hardware-queue probe.

The bar is bit-equality: whatever way the launches are scheduled -- eagerly, as one captured graph with forked streams, as one
graph per stream segment, with the labeled / unlabeled backward passes queued before or after the adversarial block -- the same
kernels run on the same operands in the same per-stream order, and gradient buffers are summed in pass order, so seven steps
must leave identical weights, Adam moments, BatchNorm running statistics and losses (cotraining_totalloss.py:203-248)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402

DEV = "cuda:0"


WIDE = ("wide", "wide_grouped")


def _run(tmp_path, arch, adv, n=7, S=2, flip=None, **attrs):
    """``flip`` = (k, switches): set before step k, after the step has been captured."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B, H = 3, 2, (176 if arch == "unet" else 64)
    segs = []
    for seed in range(11, 11 + S):
        torch.manual_seed(seed)
        segs.append(Segmentator({"name": arch, "num_classes": C, "compute_dtype": torch.bfloat16},
                                {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(S)]
    unl = FakeLoader(batches(91, n, 2 * B, H, C), 2 * B)
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                   adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
    for k, v in attrs.items():
        assert hasattr(tr, k), k
        setattr(tr, k, v)
    for s in segs:
        s.train()
    sups, kind_before_flip = [], None
    for k in range(n):
        if flip is not None and k == flip[0]:
            kind_before_flip = tr.last_route.kind
            for name, v in flip[1].items():
                assert hasattr(tr, name), name
                setattr(tr, name, v)
        lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(S)]
        out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, adv, (0, S - 1) if adv else None)
        sups.append([float(v) for v in out["sup"]] + [float(out["jsd"]), float(out["adv"]) if adv else 0.0])
    torch.cuda.synchronize()
    state = []
    for s in segs:
        state.append(torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).cpu())
        state.append(s.optimizer._m.cpu())
        state += [b.detach().clone().cpu() for b in s.torchnet.buffers()]
    return tr, sups, state, kind_before_flip


@pytest.fixture
def four_queues(monkeypatch):
    """The four-queue layouts need four stream groups.  A device that exposes fewer hardware queues (a shared box may limit them)
    gets four groups dealt round-robin through DCT_HW_QUEUES=4 instead: the layout is still exercised and still has to be bit-equal,
    only its passes share queues.  The forced groups are dropped again afterwards so that later tests probe afresh."""
    from dct_amd.trainer import stream_sched as ss
    if len(ss.queue_groups(DEV)) >= 4:
        yield
        return
    idx = torch.device(DEV).index
    monkeypatch.setenv("DCT_HW_QUEUES", "4")
    yield
    ss._QUEUE_GROUPS.pop(idx, None)
    ss._QUEUE_PROBE.pop(idx, None)


def _same(a, b):
    assert a[1] == b[1]
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("arch,adv,S", [("enet", True, 2), ("enet", False, 2), ("enet", True, 3), ("unet", True, 2)])
def test_program_of_graphs_equals_one_graph_equals_eager(tmp_path, arch, adv, S):
    eager = _run(tmp_path, arch, adv, S=S, use_hip_graph=False)
    one = _run(tmp_path, arch, adv, S=S, segmented_graphs=False)
    prog = _run(tmp_path, arch, adv, S=S, segmented_graphs=True)
    assert eager[0]._step_graphs is None
    cap1 = list(one[0]._step_graphs._graphs.values())
    capp = list(prog[0]._step_graphs._graphs.values())
    assert cap1 and all(c.program is None and c.graph is not None for c in cap1)
    assert capp and all(c.program is not None for c in capp)
    p = capp[0].program
    assert p.n_graphs >= 2 * S + 1 and p.n_nodes > 100
    # every hand-over between streams is an explicit op of the program, and a mark is recorded before it is waited for
    seen = set()
    for op in p.ops:
        if op[0] == 'record':
            seen.add(id(op[2]))
        elif op[0] == 'wait_event':
            assert id(op[2]) in seen
    assert one[0]._step_graphs.replays == prog[0]._step_graphs.replays >= 4
    # one graph holds the sequential layout; the program and the eager step the multi-queue one where the device shows four queues
    multi = (WIDE if arch == "enet" else ("adv_chain",)) if prog[0]._queue_streams() is not None else ("sequential",)
    assert one[0].last_route.kind == "sequential" and not any(one[0].last_route.pass_streams)
    assert prog[0].last_route.kind in multi and eager[0].last_route.kind in multi
    _same(eager, one)
    _same(eager, prog)


def test_default_mode_follows_the_network(tmp_path):
    """Enet (hundreds of short launches per pass) asks for the program of graphs, UNet (kernels that fill the chip) for one graph."""
    e = _run(tmp_path, "enet", False, n=4)
    u = _run(tmp_path, "unet", False, n=4)
    assert e[0]._use_segments() and all(c.program is not None for c in e[0]._step_graphs._graphs.values())
    assert not u[0]._use_segments() and all(c.program is None for c in u[0]._step_graphs._graphs.values())


@pytest.mark.parametrize("graph", [False, True])
def test_early_backward_changes_nothing(tmp_path, graph):
    """The labeled / unlabeled backward passes queued right after the FGSM chain (beside the adversarial forward) or after it:
    same pass buffers, same ((lab + unl) + adv) sum."""
    a = _run(tmp_path, "enet", True, use_hip_graph=graph, early_backward=True)
    b = _run(tmp_path, "enet", True, use_hip_graph=graph, early_backward=False)
    c = _run(tmp_path, "enet", True, use_hip_graph=graph, pass_streams=False)          # sequential in-place accumulation
    _same(a, b)
    _same(a, c)


@pytest.mark.parametrize("adv,S", [(True, 2), (False, 2), (True, 3)])
def test_four_queue_layout_changes_nothing(tmp_path, four_queues, adv, S):
    """CoTrainer._run_step_wide (forward passes with deferred running statistics, every pass on one of four hardware queues, the
    adversarial chain issued first) against the sequential layout: same weights, moments, running statistics, losses."""
    wide = _run(tmp_path, "enet", adv, S=S, wide_forward=True)
    seq = _run(tmp_path, "enet", adv, S=S, wide_forward=False)
    eager_wide = _run(tmp_path, "enet", adv, S=S, wide_forward=True, use_hip_graph=False)
    assert wide[0]._queue_streams() is not None, "fewer than four hardware queues found: the layout was not exercised"
    assert wide[0].last_route.kind in WIDE and eager_wide[0].last_route.kind in WIDE and seq[0].last_route.kind == "sequential"
    _same(wide, seq)
    _same(wide, eager_wide)


def test_unet_adversarial_chain_layout_changes_nothing(tmp_path, four_queues):
    """CoTrainer._run_step_adv_chain (2 x UNet + FGSM: the adversarial chain queued behind model b's forward, JSD and model b's
    backward on a third queue) against the sequential layout, dropout on: same weights, moments, losses."""
    new = _run(tmp_path, "unet", True, adv_chain_layout=True)
    old = _run(tmp_path, "unet", True, adv_chain_layout=False)
    new_eager = _run(tmp_path, "unet", True, adv_chain_layout=True, use_hip_graph=False)
    assert new[0]._queue_streams() is not None, "fewer than four hardware queues found: the layout was not exercised"
    assert all(c.program is not None for c in new[0]._step_graphs._graphs.values())      # adversarial steps replay as a program
    assert all(c.program is None for c in old[0]._step_graphs._graphs.values())
    assert new[0].last_route.kind == "adv_chain" and new_eager[0].last_route.kind == "adv_chain" and old[0].last_route.kind == "sequential"
    _same(new, old)
    _same(new, new_eager)


@pytest.mark.parametrize("switch", ["group_passes", "leaf_offload"])
def test_switch_flipped_after_a_capture_is_captured_again(tmp_path, four_queues, switch):
    """The captured step's signature holds the whole route: a layout switch flipped after the capture (these two were once missing
    from a hand-written list, and the old layout went on being replayed) leads to a second capture, and the run ends where a run
    with the switch off from the start ends."""
    off = _run(tmp_path, "enet", True, **{switch: False})
    flipped = _run(tmp_path, "enet", True, flip=(4, {switch: False}))          # steps 0-1 eager, 2 captured, 3 replayed | 4-5 eager, 6 captured
    assert flipped[3] == "wide_grouped" and flipped[0].last_route == off[0].last_route
    assert flipped[0].last_route.kind == ("wide" if switch == "group_passes" else "wide_grouped") and not flipped[0].last_route.leaf_offload
    assert off[0]._step_graphs.captures == 1 and flipped[0]._step_graphs.captures == 2
    _same(off, flipped)


def test_queue_groups_partition_the_candidates(monkeypatch):
    from dct_amd.trainer import stream_sched
    from dct_amd.trainer.stream_sched import StreamDealer, queue_groups, queue_probe_report
    groups = queue_groups(DEV)
    flat = [s for g in groups for s in g]
    assert 1 <= len(groups) <= len(flat) and len({s.cuda_stream for s in flat}) == len(flat) == 8
    probe = queue_probe_report(DEV)
    if probe.get("ok", probe.get("source") == "DCT_HW_QUEUES"):
        assert queue_groups(DEV) is groups              # probed once per device
    else:                                               # fewer than four queues found: reported, not cached, probed again
        assert len(groups) != 4 or max(len(g) for g in groups) > 3
        assert queue_groups(DEV) is not groups
        monkeypatch.setattr(stream_sched, "queue_groups", lambda device: groups)     # the dealer below deals these groups
    d = StreamDealer(DEV)
    first = [d.take() for _ in range(len(groups))]
    # the first len(groups) streams dealt come from different groups
    where = [next(i for i, g in enumerate(groups) if any(s.cuda_stream == t.cuda_stream for s in g)) for t in first]
    assert sorted(where) == list(range(len(groups)))
    more = [d.take() for _ in range(12)]                # more than the candidates: still streams
    assert all(isinstance(s, torch.cuda.Stream) for s in more)


def test_recorder_drops_empty_segments_and_replays_in_order():
    """A hand-made schedule: two streams, a hand-over by record / wait_event, a host callback, stream switches with nothing in
    between.  Replaying twice applies the captured work twice, in order."""
    from dct_amd.trainer.stream_sched import EagerSchedule, SegmentRecorder
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    x = torch.zeros(1 << 16, device=DEV)
    y = torch.zeros(1 << 16, device=DEV)
    calls = []

    def body(sched, main):
        sched.wait([(s1, main), (s2, main)])
        with sched.on(s1):
            x.add_(1.0)
            x.mul_(2.0)
        mark = sched.record(s1)
        with sched.on(s2):
            pass                                    # nothing launched: no graph for it
        sched.wait_event(s2, mark)
        with sched.on(s2):
            y.copy_(x)
            y.add_(0.5)
        sched.call(lambda: calls.append(len(calls)))
        sched.wait([(main, s1), (main, s2)])
        y.mul_(1.0)

    body(EagerSchedule(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert float(x[0]) == 2.0 and float(y[0]) == 2.5 and calls == [0]
    rec = SegmentRecorder(torch.device(DEV))
    rec.start()
    try:
        body(rec, rec.main)
        prog = rec.finish()
    except BaseException:
        rec.abort()
        raise
    torch.cuda.synchronize()
    assert float(x[0]) == 2.0 and calls == [0]      # recording launches nothing and calls nothing
    kinds = [op[0] for op in prog.ops]
    assert kinds.count('graph') == 3 and kinds.count('call') == 1 and kinds.index('record') < kinds.index('wait_event')
    assert [op[3] for op in prog.ops if op[0] == 'graph'] == [2, 2, 1]
    prog.replay()
    prog.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 14.0 and float(y[0]) == 14.5 and calls == [0, 1, 2]       # ((2 + 1) * 2 + 1) * 2


@pytest.mark.parametrize("message", ["capture refused (test)", "HIP error: operation not permitted when stream is capturing",
                                     "capturing stream has unjoined work"])
def test_refused_capture_falls_back_to_eager(tmp_path, monkeypatch, message):
    """A program capture the runtime refuses (RuntimeError while recording -- the messages HIP / torch really use among them) must
    leave the training on eager launches with the host counters intact: same results as a run that never captured."""
    from dct_amd.trainer import stream_sched
    eager = _run(tmp_path, "enet", True, n=6, use_hip_graph=False)

    def boom(self):
        raise RuntimeError(message)
    monkeypatch.setattr(stream_sched.SegmentRecorder, "finish", boom)
    with pytest.warns(UserWarning, match="runs eagerly"):
        fell = _run(tmp_path, "enet", True, n=6)
    g = fell[0]._step_graphs
    assert g is not None and g.captures == 0 and g.replays == 0
    assert [s.optimizer._steps for s in fell[0].segmentators] == [6, 6]
    _same(eager, fell)
