"""The pseudo-label consistency kernels (dct_pl_map_fwd / dct_pl_map_bwd / dct_pl_logits_step) against tests/pseudo_label_ref.py.

Teachers (argmax, confidence, mask) are derived on the CPU in fp32 by the rule of include/dct.h and must match bit for bit: the kept
map is compared with ``torch.equal``, and where the reference has no teacher term the kernel's loss and gradient must be 0 exactly.
Given the teachers, values and gradients are compared with float64 within the bounds that pseudo_label_ref derives from the kernels'
arithmetic (``p + eps`` formed in fp32 as the kernel forms it; logf 3 ulp; one unit roundoff per further operation).

Shapes: P in {1, 255, 257} (partial blocks) for every S in {2, 3, 5, 8} (both SMAX instantiations of the map kernels, all three of the
step kernel) and C in {2, 4, 8}; for the step kernel 262,144 and 262,145 pixels as well (the 1024-block cap and one past it, where a
thread first walks a second pixel).  Inputs: random logits x 3; sentinel pixels where every student is sure of another class than its
teacher, so p underflows to 0 and eps carries the log (test_kl_at_scale's sentinels); exact-tie pixels.  Thresholds: 0 (all kept),
one teacher confidence taken from the data so that the reference keeps between 20 % and 80 % of the terms (asserted; it needs more
than one pixel, so not at P = 1, where a single ensemble term is kept or not), and 2 (above every confidence: nothing kept)."""
import ctypes

import numpy as np
import pytest
import torch

import pseudo_label_ref as R
from pseudo_label_ref import SUM_DEPTH, TINY, U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = float(np.float32(1e-10))       # eps as the kernels receive it
MARGIN_UFL = 120.0                   # the other probabilities underflow to 0 in fp32 (tests/test_loss_kernels_scale_gpu.py)
TAU_NONE = 2.0
SMALL = [(P, S, C) for P in (1, 255, 257) for S in (2, 3, 5, 8) for C in (2, 4, 8)]
LARGE = [(262144, 2, 4), (262145, 2, 4), (262145, 3, 8), (262144, 5, 2), (262145, 8, 2)]
TEACHERS = ["cross", "ensemble"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _special(P):
    """(sentinel pixels, tie pixels): the corners of the blocks and of the 1024-block grid stride."""
    s1 = min(max(1, (P + 255) // 256), 1024) * 256
    sen = sorted({i for i in (0, 255, 256, s1 - 1, s1, P - 1) if 0 <= i < P})
    tie = sorted({i for i in (1, 2, 3, 254, s1 + 1, s1 + 2, P - 2) if 0 <= i < P} - set(sen))
    return sen, tie


def _logits(P, S, C):
    """S logit maps [P, C], fp32: random x 3; sentinels: view s is sure (by 120) of class s % C... against its neighbour's (s + 1) % C, so
    every student's probability of every teacher's class underflows to 0 (C >= 2: neighbours always differ; with S > C some views
    agree, which the counts n > 1 then cover); ties: equal logits everywhere (every class ties: the first wins), mirrored pairs in
    the first two views (their sums tie exactly)."""
    g = torch.Generator().manual_seed(1000 * P + 10 * S + C)
    xs = [torch.randn(P, C, generator=g) * 3 for _ in range(S)]
    sen, tie = _special(P)
    for s in range(S):
        xs[s][sen] = 0.0
        xs[s][sen, s % C] = MARGIN_UFL
        xs[s][tie] = 0.0
    for n_, i in enumerate(tie):
        if n_ % 2 and S > 1:               # (a single view has no partner to mirror)
            xs[0][i, 0], xs[0][i, 1] = 1.5, -0.5
            xs[1][i, 0], xs[1][i, 1] = -0.5, 1.5
    return xs


def _collapsing_pair(S):
    inv = np.float32(1.0) / np.float32(S)
    a = np.float32(1.75)
    for _ in range(64):
        b = np.nextafter(a, np.float32(2.0))
        if np.float32(a * inv) == np.float32(b * inv):
            return a, b
        a = b
    raise AssertionError("no collapsing pair found")


def _probs(P, S, C):
    """S probability maps for the map kernels: the fp32 softmax of ``_logits`` with hand-built pixels on top -- sentinels exactly one-hot,
    and for S in (3, 5) one pixel whose class sums (1 + a', 1 + b') differ by one ulp but scale to the same fp32: the argmax must be
    taken before scaling."""
    ps = [torch.softmax(x, 1).contiguous() for x in _logits(P, S, C)]
    sen, tie = _special(P)
    for s in range(S):
        ps[s][sen] = 0.0
        ps[s][sen, s % C] = 1.0
    if S in (3, 5) and tie:
        a, b = _collapsing_pair(S)
        i = tie[0]
        for s in range(S):
            ps[s][i] = 0.0
        ps[0][i, :2] = 0.5
        ps[1][i, :2] = 0.5
        ps[2][i, 0], ps[2][i, 1] = float(a - np.float32(1.0)), float(b - np.float32(1.0))
    return ps


def _taus(q, P):
    """0, a confidence out of the data that keeps between 20 % and 80 % of the teacher terms (more than one pixel), 2."""
    if P == 1:
        return [0.0, TAU_NONE]
    flat = np.sort(q.reshape(-1))
    tau = float(flat[int(0.55 * (flat.size - 1))])
    frac = float((q >= np.float32(tau)).mean())
    assert 0.2 <= frac <= 0.8, (tau, frac)
    return [0.0, tau, TAU_NONE]


def _check(got, ref, bound, what):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    bad = ~((got - ref).abs() <= bound)
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} out of bound; first at flat {i}: got {got.reshape(-1)[i].item()!r} "
                             f"ref {ref.reshape(-1)[i].item()!r} bound {bound.reshape(-1)[i].item()!r}")


@pytest.mark.parametrize("teacher", TEACHERS)
@pytest.mark.parametrize("P,S,C", SMALL)
def test_map_kernels(ops, P, S, C, teacher):
    ps = _probs(P, S, C)
    pn = [p.numpy() for p in ps]
    pg = [p.to(DEV) for p in ps]
    sen, tie = _special(P)
    mode = ops.PL_TEACHERS[teacher]
    g = torch.Generator().manual_seed(P + S + C)
    dmap = torch.randn(P, generator=g)
    for tau in _taus(R.teachers_fp32(pn, teacher, 0.0)[2], P):
        k, m, q = R.teachers_fp32(pn, teacher, tau)
        n = R.term_counts(k, m, teacher, S, C)
        v, vb, d, drel = R.map_and_grad(pn, n, teacher, EPS)
        out, kept = ops.pl_map_fwd(pg, C, mode, tau, EPS)
        out_nokept, none = ops.pl_map_fwd(pg, C, mode, tau, EPS, want_kept=False)
        dps = ops.pl_map_bwd(pg, dmap.to(DEV), C, mode, tau, EPS)
        torch.cuda.synchronize()
        what = f"{teacher} P={P} S={S} C={C} tau={tau}"
        # teachers, bit for bit
        assert torch.equal(kept.cpu(), torch.from_numpy(R.kept_map(m, teacher, S))), what
        assert none is None and torch.equal(out, out_nokept)
        nopix = n.sum((0, 2)) == 0
        assert (out.cpu()[nopix] == 0).all(), what
        for s in range(S):
            assert (dps[s].cpu()[n[s] == 0] == 0).all(), what
        if tau == 0.0:
            assert m.all() and (kept == 1).all()
        if tau == TAU_NONE:
            assert not m.any() and (out == 0).all() and all((dp == 0).all() for dp in dps)
        # values and gradients
        _check(out, v, vb + TINY, what + " map")
        for s in range(S):
            ref = dmap.double()[:, None] * d[s]
            _check(dps[s], ref, (drel + U) * ref.abs() + TINY, what + f" dprobs {s}")
        if tau == 0.0 and 1 < S <= C:
            # the sentinels (one-hot views of distinct classes): every term of a student on another view's class is log(0 + eps) = -23.03;
            # the ensemble votes class 0 (all sums tie), which view 0 itself holds with p = 1: S - 1 such terms
            w = R.weight(teacher, S)
            terms = S * (S - 1) if teacher == "cross" else S - 1
            np.testing.assert_allclose(v[sen].numpy(), w * terms * -np.log(EPS), rtol=1e-12)
            assert (v[sen] > 1e4 * vb[sen]).all()


def _step_reference(ops, xs, C, teacher, tau, gg):
    """The step kernel's reference from hip_ops.softmax_fwd's probabilities (softmax_px's bits): teachers in fp32, the rest float64."""
    S = len(xs)
    sm = [ops.softmax_fwd(x, C) for x in xs]
    pn = [p.cpu().numpy() for p in sm]
    k, m, q = R.teachers_fp32(pn, teacher, tau)
    n = R.term_counts(k, m, teacher, S, C)
    v, vb, d, _ = R.map_and_grad(pn, n, teacher, EPS)
    grads = [R.logit_grad(pn[s], d[s], gg, C) for s in range(S)]
    return sm, m, q, n, v, vb, grads


@pytest.mark.parametrize("teacher", TEACHERS)
@pytest.mark.parametrize("P,S,C", SMALL + LARGE)
def test_step_kernel(ops, P, S, C, teacher):
    xs = [x.to(DEV) for x in _logits(P, S, C)]
    mode = ops.PL_TEACHERS[teacher]
    gscale, gmul = 0.5, 2.0
    gg = float(np.float32(gscale)) * gmul / P
    gs = torch.tensor([gscale], device=DEV)
    kden = S if teacher == "cross" else 1
    g = torch.Generator().manual_seed(3 * P + S + C)
    olds = [torch.randn(P, C, generator=g).to(DEV) for _ in range(S)]
    q0 = R.teachers_fp32([p.cpu().numpy() for p in (ops.softmax_fwd(x, C) for x in xs)], teacher, 0.0)[2]
    for tau in _taus(q0, P):
        what = f"{teacher} P={P} S={S} C={C} tau={tau}"
        dls = [_nan(P, C) for _ in range(S)]
        out2, probs = ops.pl_logits_step(xs, C, dls, True, gscale=gs, gmul=gmul, teacher=mode, tau=tau, eps=EPS)
        acc = [o.clone() for o in olds]
        out2a, none = ops.pl_logits_step(xs, C, acc, False, gscale=gs, gmul=gmul, accumulate=True, teacher=mode, tau=tau, eps=EPS)
        out2n, probs_n = ops.pl_logits_step(xs, C, None, True, gscale=gs, gmul=gmul, teacher=mode, tau=tau, eps=EPS)
        torch.cuda.synchronize()
        # accumulate: the rounded gradient added to what was there, bit for bit; no gradients asked: the same values and maps
        assert none is None and torch.equal(out2, out2a) and torch.equal(out2, out2n), what
        for s in range(S):
            assert torch.equal(acc[s], dls[s] + olds[s]), what
            assert torch.equal(probs[s], probs_n[s]), what
        if tau == TAU_NONE:
            # nothing kept: no float64 needed -- everything is exactly 0 and finite
            assert out2.tolist() == [0.0, 0.0] and all((dl == 0).all() for dl in dls), what
            continue
        sm, m, q, n, v, vb, grads = _step_reference(ops, xs, C, teacher, tau, gg)
        for s in range(S):
            assert torch.equal(probs[s], sm[s]), what                                   # softmax_fwd's bits
        # the kept fraction: whole numbers summed in fp32 (exact below 2^24), one fp32 division
        frac = np.float32(m.sum()) / np.float32(np.float32(P) * np.float32(kden))
        assert out2[1].item() == float(frac), (what, out2[1].item(), float(frac))
        if tau == 0.0:
            assert out2[1].item() == 1.0
        ref = v.mean().item()
        tol = (vb.sum().item() + SUM_DEPTH * U * v.abs().sum().item()) / P + 2 * U * abs(ref) + TINY
        assert abs(out2[0].item() - ref) <= tol, (what, out2[0].item(), ref, tol)
        for s in range(S):
            gref, gb = grads[s]
            _check(dls[s], gref, gb, what + f" dlogits {s}")
            assert (dls[s].cpu()[(n[s] == 0).all(1)] == 0).all(), what                  # a student without a teacher term: exactly 0


CLASS_SWEEP = [(S, C, teacher) for C in range(2, 9) for S in (1, 2, 3, 5) for teacher in TEACHERS if S > 1 or teacher == "ensemble"]


@pytest.mark.parametrize("S,C,teacher", CLASS_SWEEP)
def test_every_class_count_of_the_dispatch(ops, S, C, teacher):
    """The dispatch instantiates C = 2..8 and the grids above use 2, 4 and 8: the map kernels and the step kernel at every C, at 257
    pixels (one full block and a grid-stride tail of one pixel), S = 2, 3, 5 (every SMAX instantiation) and the ensemble's single
    view; the references, thresholds and bounds are the tests' above, which this runs as they are."""
    test_map_kernels(ops, 257, S, C, teacher)
    test_step_kernel(ops, 257, S, C, teacher)


def test_status_codes(ops):
    from dct_amd import _lib
    lib = _lib.load()
    P, C, S = 64, 4, 3
    xs = [torch.randn(P, C, device=DEV) for _ in range(S)]
    outs = [torch.empty(P, C, device=DEV) for _ in range(S)]
    mp, out2 = torch.empty(P, device=DEV), torch.empty(2, device=DEV)
    ws = ops._loss_ws(xs[0].device)
    arr, oarr = ops._ptr_array(xs), ops._ptr_array(outs)
    nullarr = (ctypes.c_void_p * S)(xs[0].data_ptr(), None, xs[2].data_ptr())
    st = ops.stream()
    BAD, UNS, WSP = -1, -2, -4

    def fwd(S_=S, t=0, tau=0.5, eps=1e-10, a=arr, m_=mp.data_ptr(), P_=P, C_=C):
        return lib.dct_pl_map_fwd(a, S_, t, tau, eps, m_, None, P_, C_, st)

    def bwd(S_=S, t=0, tau=0.5, eps=1e-10, a=arr, dm=mp.data_ptr(), o=oarr, P_=P, C_=C):
        return lib.dct_pl_map_bwd(a, S_, t, tau, eps, dm, o, P_, C_, st)

    def step(S_=S, t=0, tau=0.5, eps=1e-10, a=arr, P_=P, C_=C, o2=out2.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        return lib.dct_pl_logits_step(a, S_, t, tau, eps, P_, C_, o2, None, None, 1.0, None, 0, w, wb, st)

    for f in (fwd, bwd, step):
        assert f() == 0 and f(t=1) == 0 and f(S_=1, t=1) == 0 and f(tau=float("inf")) == 0
        assert f(S_=1, t=0) == BAD and f(S_=0, t=1) == BAD and f(S_=9) == BAD and f(S_=9, t=1) == BAD     # S outside the mode's range
        assert f(t=2) == BAD and f(t=-1) == BAD                                                          # an unknown mode
        assert f(tau=-0.1) == BAD and f(tau=float("nan")) == BAD
        assert f(eps=0.0) == BAD and f(eps=-1e-10) == BAD and f(eps=float("nan")) == BAD
        assert f(a=None) == BAD and f(a=nullarr) == BAD and f(P_=0) == BAD
        assert f(C_=1) == UNS and f(C_=9) == UNS
    assert fwd(m_=None) == BAD and bwd(dm=None) == BAD and bwd(o=None) == BAD and bwd(o=nullarr) == BAD and step(o2=None) == BAD
    assert step(w=None) == WSP and step(wb=16) == WSP
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,teacher", [("cps", "cross"), ("pseudo_label", "ensemble")])
def test_module_through_autograd_equals_the_raw_ops(ops, name, teacher):
    from dct_amd.loss import get_loss_fn
    B, C, H, W, S = 2, 4, 9, 13, 3
    g = torch.Generator().manual_seed(5)
    logits = [(torch.randn(B, C, H, W, generator=g) * 3).to(DEV) for _ in range(S)]
    leaves = [torch.softmax(x, 1).requires_grad_(True) for x in logits]
    q = R.teachers_fp32([p.detach().permute(0, 2, 3, 1).reshape(-1, C).cpu().numpy() for p in leaves], teacher, 0.0)[2]
    tau = _taus(q, B * H * W)[1]
    crit = get_loss_fn(name, threshold=tau)
    out = crit(leaves)
    assert out.shape == (B, H, W) and torch.is_tensor(crit.last_kept) and crit.last_kept.is_cuda and crit.last_kept.dim() == 0
    seed = torch.randn(B, H, W, generator=g).to(DEV)
    (out * seed).sum().backward()
    pcs = [p.detach().permute(0, 2, 3, 1).contiguous() for p in leaves]
    mp, kept = ops.pl_map_fwd(pcs, C, **crit.launch_args())
    dps = ops.pl_map_bwd(pcs, seed.reshape(-1).contiguous(), C, **crit.launch_args())
    torch.cuda.synchronize()
    assert torch.equal(out.detach().reshape(-1), mp)
    assert torch.equal(crit.last_kept, kept.mean()) and 0.2 <= crit.last_kept.item() <= 0.8
    for p, dp in zip(leaves, dps):
        assert torch.equal(p.grad.permute(0, 2, 3, 1).reshape(-1, C), dp.reshape(-1, C))
    # the mean over ALL pixels is what the trainer's generic step takes; fewer than two views are refused by cross at call time
    assert torch.isfinite(out.mean())
    if teacher == "cross":
        with pytest.raises(ValueError, match="at least 2 views"):
            crit(leaves[:1])
    else:
        assert crit(leaves[:1]).shape == (B, H, W)
