"""The guard in front of the fused Adam (include/dct.h: dct_grad_sumsq, dct_adam_flat_dev_guarded; optim.FusedAdam max_grad_norm /
skip_nonfinite): the norm against float64, non-finite detection, the guarded update against the unguarded kernel bit for bit, and the
guarded training step (eager, captured, replayed) of 2 x UNet in bf16.

The grid rule of grad_sumsq_kernel (csrc/loss.hip): blocks = clamp(ceil(floor(n / 4) / 256), 1, 2048) of 256 threads, one 16-byte vector
per thread and round, rounds taken two at a time; so STRIDE = 2048 * 256 vectors is one full round of the largest grid, every thread
makes at least two rounds from 2 * STRIDE vectors on, and vector STRIDE (element 4 * STRIDE) is the first one a second round reads."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402

DEV = "cuda:0"
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
STRIDE = 2048 * 256
N_TWO_ROUNDS = 4 * (2 * STRIDE) + 3          # every thread of every block: two rounds; three tail elements
SUMSQ_SIZES = [1, 3, 4, 5, 1023, 4 * 256 + 1, N_TWO_ROUNDS - 4, N_TWO_ROUNDS, 4 * (3 * STRIDE + 5) + 3]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _blocks(n):
    return min(max((n // 4 + 255) // 256, 1), 2048)


def _sum64(g):
    x = g.detach().cpu().numpy().astype(np.float64)
    return float(np.sum(x * x))


def _dev_state(t, lr, base, length):
    table = torch.tensor([(1.0 - B1 ** k, math.sqrt(1.0 - B2 ** k)) for k in range(base + 1, base + 1 + length)], dtype=torch.float64)
    state = torch.tensor([float(t), lr, float(base), float(length)], dtype=torch.float64)
    return state.to(DEV), table.to(DEV)


class _Bufs:
    """p, m, v (+ shadow) and the device state of one Adam run, all from one seed."""

    def __init__(self, n, shadow, p0=None, seed=17):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.p = torch.randn(n, device=DEV, generator=g) if p0 is None else p0.clone()
        self.m, self.v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.s = torch.zeros(n + 8, dtype=torch.bfloat16, device=DEV)[:n] if shadow else None
        self.state, self.table = _dev_state(0, 1e-3, 0, 8)

    def clone(self):
        c = _Bufs.__new__(_Bufs)
        c.p, c.m, c.v = self.p.clone(), self.m.clone(), self.v.clone()
        c.s = self.s.clone() if self.s is not None else None
        c.state, c.table = self.state.clone(), self.table
        return c

    def same(self, o):
        return (torch.equal(self.p, o.p) and torch.equal(self.m, o.m) and torch.equal(self.v, o.v) and torch.equal(self.state, o.state)
                and (self.s is None or torch.equal(self.s, o.s)))

    def plain(self, ops, gr, wd, gs):
        ops.adam_flat_dev(self.p, gr, self.m, self.v, self.state, self.table, B1, B2, ADAM_EPS, wd, bf16_shadow=self.s, grad_scale=gs)

    def guarded(self, ops, gr, wd, gs, rec, ws, skip, clip):
        ops.adam_flat_dev_guarded(self.p, gr, self.m, self.v, self.state, self.table, B1, B2, ADAM_EPS, wd, ws, rec, bf16_shadow=self.s,
                                  grad_scale=gs, skip_nonfinite=skip, clip=clip)


def _record(ops, rec):
    f = {k: v.cpu() for k, v in ops.guard_fields(rec).items()}
    return dict(norm=float(f["norm"][0]), max_norm=float(f["max_norm"][0]), coef=f["coef"].numpy()[0], skip=int(f["skip"][0]),
                skipped=int(f["skipped"][0]), clipped=int(f["clipped"][0]))


# ------------------------------------------------------------------------------------------------------------------- 1. sum of squares
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_vs_float64(ops, n):
    """Squares are exact in double and the folds are in double: the only error is that of the double additions, <= n 2^-53 relative
    (7e-10 at the largest n here), inside 1e-9; two runs give the same bits, and there is one partial per block of the grid rule."""
    g = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n % 1000 + 3))
    a = ops.grad_sumsq(g).clone()
    b = ops.grad_sumsq(g)
    torch.cuda.synchronize()
    assert a.numel() == _blocks(n) and a.dtype == torch.float64
    assert torch.equal(a, b)
    want = _sum64(g)
    got = float(a.sum())
    print(f"n {n}: sum {got!r} ref {want!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-9 * want


# ------------------------------------------------------------------------------------------------------------------- 2. non-finite
def test_sumsq_sees_every_nonfinite_and_no_overflow(ops):
    n = 4 * (STRIDE + 10) + 3
    n4 = n // 4
    g0 = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    ws = ops.grad_sumsq_workspace(n, DEV)
    places = [0, 4 * (n4 - 1), 4 * (n4 - 1) + 3, 4 * n4, 4 * n4 + 1, 4 * n4 + 2, 4 * STRIDE]
    for pos in places:
        for val in (float("inf"), float("-inf"), float("nan")):
            g = g0.clone()
            g[pos] = val
            assert not math.isfinite(float(ops.grad_sumsq(g, ws).sum())), (pos, val)
    g = g0.clone()
    g[1], g[4 * STRIDE + 1] = float("inf"), float("-inf")      # same lane's accumulator in two rounds: must not cancel
    s = float(ops.grad_sumsq(g, ws).sum())
    assert math.isinf(s) and s > 0
    g[4 * STRIDE + 1] = 7.0
    g[2] = float("-inf")                                        # and in one vector
    s = float(ops.grad_sumsq(g, ws).sum())
    assert math.isinf(s) and s > 0
    assert math.isfinite(float(ops.grad_sumsq(g0, ws).sum()))
    # 1e30 squared overflows fp32 but is a finite gradient: finite norm, no skip
    big = torch.full((n,), 1e30, device=DEV)
    b = _Bufs(n, False)
    rec = ops.adam_guard_record(DEV)
    b.guarded(ops, big, 0.0, 1.0, rec, ws, True, False)
    r = _record(ops, rec)
    want = math.sqrt(_sum64(big))
    assert math.isfinite(r["norm"]) and abs(r["norm"] - want) <= 1e-9 * want
    assert r["skip"] == 0 and r["skipped"] == 0 and b.state[0].item() == 1.0


# ------------------------------------------------------------------------------------------------------------------- 3. guard off
@pytest.mark.parametrize("n,shadow,gs,wd", [
    (1, False, 1.0, 0.0), (3, True, 1.0, 1e-4), (5, False, 2.0 ** -13, 1e-4), (5, True, 2.0 ** -13, 0.0),
    (100003, True, 1.0, 1e-4), (100003, False, 2.0 ** -13, 0.0), (100003, True, 2.0 ** -13, 1e-4), (100003, False, 1.0, 0.0),
])
def test_guard_off_is_the_unguarded_kernel(ops, n, shadow, gs, wd):
    """Clipping and skipping off, and clipping at a max_norm of 1e30 (coef == 1): three steps leave the bits of dct_adam_flat_dev."""
    ref = _Bufs(n, shadow)
    off, never = ref.clone(), ref.clone()
    rec_off, rec_never = ops.adam_guard_record(DEV), ops.adam_guard_record(DEV, 1e30)
    ws = ops.grad_sumsq_workspace(n, DEV)
    gen = torch.Generator(device=DEV).manual_seed(23)
    for t in range(3):
        gr = torch.randn(n, device=DEV, generator=gen) * 0.1 / gs
        ref.plain(ops, gr, wd, gs)
        off.guarded(ops, gr, wd, gs, rec_off, ws, False, False)
        never.guarded(ops, gr, wd, gs, rec_never, ws, True, True)
        torch.cuda.synchronize()
        assert ref.same(off) and ref.same(never), f"step {t}"
    assert ref.state[0].item() == 3.0
    for rec in (rec_off, rec_never):
        r = _record(ops, rec)
        assert r["coef"] == np.float32(1.0) and r["skipped"] == 0 and r["clipped"] == 0 and r["skip"] == 0


# ------------------------------------------------------------------------------------------------------------------- 4. clipping
@pytest.mark.parametrize("n,shadow,gs,wd", [(100003, True, 1.0, 1e-4), (100003, False, 2.0 ** -13, 0.0), (5, True, 2.0 ** -13, 1e-4)])
def test_clipping(ops, n, shadow, gs, wd):
    gr = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(29)) * 0.1 / gs
    norm64 = gs * math.sqrt(_sum64(gr))
    ws = ops.grad_sumsq_workspace(n, DEV)
    # a gradient of ten times max_norm
    max_norm = norm64 / 10.0
    ref = _Bufs(n, shadow)
    got = ref.clone()
    rec = ops.adam_guard_record(DEV, max_norm)
    got.guarded(ops, gr, wd, gs, rec, ws, False, True)
    r = _record(ops, rec)
    assert abs(r["norm"] - norm64) <= 1e-9 * norm64
    c64 = np.float32(min(1.0, max_norm / (norm64 + 1e-6)))
    assert r["coef"] in (c64, np.nextafter(c64, np.float32(0)), np.nextafter(c64, np.float32(1))), (r["coef"], c64)
    ref.plain(ops, gr, wd, float(np.float32(gs) * r["coef"]))
    torch.cuda.synchronize()
    assert ref.same(got)
    assert r["clipped"] == 1 and r["skipped"] == 0
    # half of max_norm: coef is exactly 1 and the count stays
    ops.guard_fields(rec)["max_norm"].fill_(2.0 * norm64)
    got.guarded(ops, gr, wd, gs, rec, ws, False, True)
    ref.plain(ops, gr, wd, gs)
    r = _record(ops, rec)
    assert r["coef"] == np.float32(1.0) and r["clipped"] == 1
    assert ref.same(got)


# ------------------------------------------------------------------------------------------------------------------- 5. skip
@pytest.mark.parametrize("n,shadow", [(100003, True), (100003, False), (6, True)])
def test_skip(ops, n, shadow):
    gen = torch.Generator(device=DEV).manual_seed(31)
    ws = ops.grad_sumsq_workspace(n, DEV)
    got = _Bufs(n, shadow)
    rec = ops.adam_guard_record(DEV)
    got.guarded(ops, torch.randn(n, device=DEV, generator=gen) * 0.1, 1e-4, 1.0, rec, ws, True, False)    # one good step: m, v, shadow live
    before = got.clone()
    bad = torch.randn(n, device=DEV, generator=gen) * 0.1
    bad[n - 2] = float("nan")
    got.guarded(ops, bad, 1e-4, 1.0, rec, ws, True, False)
    torch.cuda.synchronize()
    assert got.same(before) and got.state[0].item() == 1.0
    r = _record(ops, rec)
    assert r["skip"] == 1 and r["skipped"] == 1 and r["coef"] == np.float32(1.0) and math.isnan(r["norm"])
    # the next clean step is the unguarded kernel's from the same state (the step count that did not move included)
    clean = torch.randn(n, device=DEV, generator=gen) * 0.1
    got.guarded(ops, clean, 1e-4, 1.0, rec, ws, True, False)
    before.plain(ops, clean, 1e-4, 1.0)
    torch.cuda.synchronize()
    assert got.same(before) and got.state[0].item() == 2.0
    assert _record(ops, rec)["skip"] == 0 and _record(ops, rec)["skipped"] == 1
    # skip_nonfinite off under a clip: the NaN reaches p, as it does today
    rec2 = ops.adam_guard_record(DEV, 1.0)
    got.guarded(ops, bad, 1e-4, 1.0, rec2, ws, False, True)
    torch.cuda.synchronize()
    assert torch.isnan(got.p).any() and got.state[0].item() == 3.0 and _record(ops, rec2)["skipped"] == 0


# ------------------------------------------------------------------------------------------------------------------- 6. error codes
def test_error_codes(ops):
    from dct_amd import _lib
    lib = _lib.load()
    n = 4099
    b = _Bufs(n, True)
    g = torch.zeros(n + 4, device=DEV)
    ws = ops.grad_sumsq_workspace(n, DEV)
    rec = ops.adam_guard_record(DEV)
    nb = ws.numel() * 8
    assert nb == lib.dct_grad_sumsq_workspace_bytes(n) == 8 * _blocks(n) and lib.dct_grad_sumsq_workspace_bytes(0) == 0
    P = _lib.ptr
    BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
    assert b"workspace" in lib.dct_status_string(WORKSPACE)
    assert lib.dct_grad_sumsq(0, n, P(ws), nb, 0) == BAD_ARG
    assert lib.dct_grad_sumsq(P(g), n, 0, nb, 0) == BAD_ARG
    assert lib.dct_grad_sumsq(P(g), 0, P(ws), nb, 0) == BAD_ARG
    assert lib.dct_grad_sumsq(P(g) + 4, n, P(ws), nb, 0) == UNSUPPORTED
    assert lib.dct_grad_sumsq(P(g), n, P(ws), nb - 1, 0) == WORKSPACE
    assert lib.dct_grad_sumsq(P(g), n, P(ws), nb, 0) == 0

    def guarded(**kw):
        a = dict(p=P(b.p), g=P(g), m=P(b.m), v=P(b.v), state=P(b.state), ws=P(ws), nb=nb, rec=P(rec), shadow=P(b.s))
        a.update(kw)
        return lib.dct_adam_flat_dev_guarded(a["p"], a["g"], a["m"], a["v"], n, a["state"], P(b.table), B1, B2, ADAM_EPS, 0.0, 1.0,
                                             a["shadow"], a["ws"], a["nb"], a["rec"], 1, 0, 0)
    for k in ("p", "g", "m", "v", "state", "ws", "rec"):
        assert guarded(**{k: 0}) == BAD_ARG, k
    assert guarded(g=P(g) + 4) == UNSUPPORTED
    assert guarded(rec=P(rec) + 4) == UNSUPPORTED
    assert guarded(nb=nb - 1) == WORKSPACE
    p0 = b.p.clone()
    torch.cuda.synchronize()
    assert torch.equal(b.p, p0) and b.state[0].item() == 0.0       # a refused call launches nothing
    assert guarded() == 0 and guarded(shadow=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- optimizer
def test_table_rebuild_after_a_skip(ops):
    """TABLE_STEPS = 4, six steps, the third skipped: the host count runs ahead of the device's, the table is rebuilt from the device's
    count, and the result is the unguarded kernel stepped five times (always inside its table) on the same gradients."""
    from dct_amd.arch.flat import FlatParams
    from dct_amd.optim import FusedAdam
    torch.manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(37, device=DEV)), torch.nn.Parameter(torch.randn(5, 3, device=DEV))]
    flat = FlatParams(params)
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-4, flat=flat, skip_nonfinite=True)
    opt.TABLE_STEPS = 4
    flat.ensure()
    ref = _Bufs(flat.total, False, p0=flat.flat)
    gen = torch.Generator(device=DEV).manual_seed(37)
    for k in range(6):
        flat.ensure_grads()
        gr = torch.randn(flat.total, device=DEV, generator=gen) * 0.1
        if k == 2:
            gr[40] = float("inf")
        else:
            ref.plain(ops, gr, 1e-4, 1.0)
        flat.gflat.copy_(gr)
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(flat.flat, ref.p) and torch.equal(opt._m, ref.m) and torch.equal(opt._v, ref.v)
    assert opt._dev_state[0].item() == 5.0 and opt._table_base == 4
    assert opt.guard_counts() == {"skipped": 1, "clipped": 0}
    sd = opt.state_dict()
    assert {int(float(st["step"])) for st in sd["state"].values()} == {5} and opt._steps == 5


# ------------------------------------------------------------------------------------------------------------------- trainer
C, B_L, B_U, H = 3, 1, 2, 176        # the smallest UNet step of the suite (tests/test_step_gpu.py)


def _trainer(tmp_path, n, extra=None, use_graph=True, poison=None):
    """2 x UNet (no BatchNorm: a NaN batch leaves no running statistics behind) in bf16, built as tests/test_fp16_gpu.py::_trainer;
    ``extra``: more optim_dict keys; ``poison``: the step whose labeled images get one NaN pixel."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    segs = []
    for seed in (11, 12):
        torch.manual_seed(seed)
        segs.append(Segmentator({"name": "unet", "num_classes": C, "compute_dtype": torch.bfloat16, "dropout_p": 0.0},
                                dict({"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, **(extra or {})),
                                {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    lab = [FakeLoader(batches(81 + i, n, B_L, H, C), B_L) for i in range(2)]
    unl = FakeLoader(batches(91, n, B_U, H, C), B_U)
    if poison is not None:
        for i in range(2):
            lab[i][poison][0][0][0, 0, H // 2, H // 3] = float("nan")
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=list(range(1, C)),
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                   adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
    tr.use_hip_graph = use_graph
    for s in segs:
        s.train()
    return tr, lab, unl


def _step(tr, lab, unl, k):
    lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
    out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, True, (0, 1))
    return [float(v) for v in out["sup"]] + [float(out["jsd"]), float(out["adv"])]


def _weights(tr):
    torch.cuda.synchronize()
    return [(s.torchnet.flat_params.flat.clone(), s.optimizer._m.clone(), s.optimizer._v.clone()) for s in tr.segmentators]


def _same(a, b):
    return all(torch.equal(x, y) for wa, wb in zip(a, b) for x, y in zip(wa, wb))


def test_step_with_a_guard_that_never_triggers(tmp_path):
    n = 5
    res = []
    for extra in (None, {"max_grad_norm": 1e30, "skip_nonfinite": True}):
        tr, lab, unl = _trainer(tmp_path, n, extra)
        log = [_step(tr, lab, unl, k) for k in range(n)]
        res.append((log, _weights(tr)))
        assert tr._step_graphs is not None and tr._step_graphs.replays >= 2
        for s in tr.segmentators:
            assert s.optimizer.guarded == (extra is not None)
            assert s.optimizer.guard_counts() == {"skipped": 0, "clipped": 0}
            assert s.optimizer._dev_state[0].item() == float(n)
    (la, wa), (lb, wb) = res
    assert np.isfinite(np.array(la)).all() and la == lb
    assert _same(wa, wb)


def test_poisoned_batch_is_skipped(tmp_path):
    """One NaN pixel in the labeled images of a REPLAYED step: with skip_nonfinite the step leaves weights, moments and step count alone
    and training goes on; without the guard the same run ends with non-finite weights."""
    n, k = 6, 4
    tr, lab, unl = _trainer(tmp_path, n, {"skip_nonfinite": True}, poison=k)
    snaps = []
    for j in range(n):
        replays = tr._step_graphs.replays if tr._step_graphs is not None else 0
        log = _step(tr, lab, unl, j)
        snaps.append(_weights(tr))
        if j == k:
            assert tr._step_graphs.replays == replays + 1 and tr._step_graphs.replays >= 2       # k was a replay, not the capture
        if j == k + 1:
            assert np.isfinite(np.array(log)).all()
    assert _same(snaps[k], snaps[k - 1])
    assert not _same(snaps[k + 1], snaps[k])
    for s, w in zip(tr.segmentators, snaps[-1]):
        assert all(torch.isfinite(x).all() for x in w)
        assert s.optimizer.guard_counts() == {"skipped": 1, "clipped": 0}
        assert {int(float(st["step"])) for st in s.optimizer.state_dict()["state"].values()} == {n - 1}
        assert s.optimizer._steps == n - 1
    # what the guard prevents
    tr, lab, unl = _trainer(tmp_path, n, None, poison=k)
    for j in range(n):
        _step(tr, lab, unl, j)
    for w in _weights(tr):
        assert not torch.isfinite(w[0]).all()


def test_clipping_in_the_step(tmp_path):
    n = 6
    tr, lab, unl = _trainer(tmp_path, n, {"max_grad_norm": 1e30})
    _step(tr, lab, unl, 0)
    norms = [float(s.optimizer.last_grad_norm) for s in tr.segmentators]
    assert all(math.isfinite(x) and x > 0 for x in norms)
    max_norm = min(norms) / 50.0            # well under the first step's norm (and the next ones': asserted through the counts)
    res = []
    for use_graph in (False, True):
        tr, lab, unl = _trainer(tmp_path, n, {"max_grad_norm": max_norm}, use_graph=use_graph)
        log = [_step(tr, lab, unl, j) for j in range(n - 1)]
        res.append((log, _weights(tr)))
        for s in tr.segmentators:
            assert s.optimizer.guard_counts() == {"skipped": 0, "clipped": n - 1}
    assert res[0][0] == res[1][0] and _same(res[0][1], res[1][1])
    # (tr is the replayed run) another threshold between two replays: the next step differs, without a new capture
    sg = tr._step_graphs
    assert sg.replays >= 2
    captures, replays = sg.captures, sg.replays
    for s in tr.segmentators:
        s.optimizer.set_max_grad_norm(1e30)
    _step(tr, lab, unl, n - 1)
    assert sg.captures == captures and sg.replays == replays + 1
    for s in tr.segmentators:
        assert s.optimizer.guard_counts()["clipped"] == n - 1           # this one was not clipped
        assert float(ops_coef(s.optimizer)) == 1.0
    # the guard switched off: a new capture (after the eager warm-up of the new signature)
    for s in tr.segmentators:
        s.optimizer.set_max_grad_norm(None)
        assert not s.optimizer.guarded
    for j in range(sg.WARMUP + 1):
        _step(tr, lab, unl, j)
    assert sg.captures == captures + 1


def ops_coef(opt):
    from dct_amd import hip_ops
    return hip_ops.guard_fields(opt._guard)["coef"][0]
