"""The softmax-MSE consistency kernels (dct_mse_map_fwd / dct_mse_map_bwd / dct_mse_logits_step) against tests/mse_consistency_ref.py.

The first maximum, the confidence and the mask are pseudo_label_ref's, derived on the CPU in fp32, and must match bit for bit: the kept
map is compared with ``torch.equal``, and where the reference has no kept teacher term the kernel's value and gradient must be 0
exactly, whatever ``dmap`` holds.  Given those, values and gradients are compared with float64 within the bounds mse_consistency_ref
derives from the kernels' operation count.

Shapes, inputs and thresholds are tests/test_pseudo_label_gpu.py's (rebuilt here): P in {1, 255, 257} for every S in {2, 3, 5, 8} and
C in {2, 4, 8}, for the step kernel 262,144 and 262,145 pixels as well; random logits x 3, the one-hot sentinels, the tie pixels
including the collapsing pair; thresholds 0, one confidence from the data that keeps between 20 % and 80 % of the terms (asserted on
the reference; not at P = 1), and 2.  Every output is pre-filled with NaN, so an element no kernel wrote shows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mse_consistency_ref as R
import pseudo_label_ref as PR
from mse_consistency_ref import SUM_DEPTH, TINY, U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN_UFL = 120.0                   # the other probabilities underflow to 0 in fp32 (tests/test_loss_kernels_scale_gpu.py)
TAU_NONE = 2.0
HUGE = 3.0e38                        # a finite dmap that turns anything but an exact 0 into something enormous
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


@functools.lru_cache(maxsize=2)
def _logits(P, S, C):
    """test_pseudo_label_gpu._logits: S logit maps [P, C], fp32: random x 3; sentinels: view s is sure (by 120) of class s % C, so its
    softmax is exactly one-hot; ties: equal logits everywhere, mirrored pairs in the first two views (their sums tie exactly).
    (Shared by the teachers of a shape: never written to.)"""
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
    return tuple(xs)


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
    """test_pseudo_label_gpu._probs: the fp32 softmax of ``_logits`` with hand-built pixels on top -- sentinels exactly one-hot, and for
    S in (3, 5) one pixel whose class sums differ by one ulp but scale to the same fp32: the argmax must be taken before scaling."""
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


def _sentinel_value(S, C):
    """Cross teacher, one-hot views of classes s % C, everything kept: every ordered pair of views of different classes is 2 apart."""
    pairs = sum(1 for i in range(S) for j in range(S) if j != i and i % C != j % C)
    return 2.0 * pairs * R.weight("cross", S, C)


def _no_term(m, teacher, S):
    """[S, P] bool: student i meets no kept teacher term."""
    if teacher == "cross":
        return np.stack([~np.stack([m[j] for j in range(S) if j != i]).any(0) for i in range(S)])
    return np.broadcast_to(~m[0], (S, m.shape[1]))


@pytest.mark.parametrize("teacher", TEACHERS)
@pytest.mark.parametrize("P,S,C", SMALL)
def test_map_kernels(ops, P, S, C, teacher):
    ps = _probs(P, S, C)
    pn = [p.numpy() for p in ps]
    pg = [p.to(DEV) for p in ps]
    sen, tie = _special(P)
    mode = ops.PL_TEACHERS[teacher]
    g = torch.Generator().manual_seed(P + S + C)
    dmap0 = torch.randn(P, generator=g)
    for tau in _taus(PR.teachers_fp32(pn, teacher, 0.0)[2], P):
        m, v, vb, d, db = R.rule(pn, teacher, tau)
        none_kept = torch.from_numpy(~m.any(0))
        noterm = torch.from_numpy(np.ascontiguousarray(_no_term(m, teacher, S)))
        dmap = torch.where(none_kept, torch.full_like(dmap0, HUGE), dmap0)          # huge where the reference keeps nothing
        what = f"{teacher} P={P} S={S} C={C} tau={tau}"
        # straight through the library, into NaN
        out, kept, dps = _nan(P), _nan(P), [_nan(P, C) for _ in range(S)]
        ops.call("dct_mse_map_fwd", ops._ptr_array(pg), S, mode, tau, ops.ptr(out), ops.ptr(kept), P, C, ops.stream())
        dmg = dmap.to(DEV)
        ops.call("dct_mse_map_bwd", ops._ptr_array(pg), S, mode, tau, ops.ptr(dmg), ops._ptr_array(dps), P, C, ops.stream())
        # and through the wrappers
        out_w, kept_w = ops.mse_map_fwd(pg, C, teacher=mode, tau=tau)
        out_nokept, none = ops.mse_map_fwd(pg, C, teacher=mode, tau=tau, want_kept=False)
        dps_w = ops.mse_map_bwd(pg, dmg, C, teacher=mode, tau=tau)
        torch.cuda.synchronize()
        assert none is None and torch.equal(out, out_w) and torch.equal(out, out_nokept) and torch.equal(kept, kept_w), what
        assert all(torch.equal(a, b) for a, b in zip(dps, dps_w)), what
        # the masks, bit for bit
        assert torch.equal(kept.cpu(), torch.from_numpy(PR.kept_map(m, teacher, S))), what
        assert (out.cpu()[noterm.all(0)] == 0).all(), what
        for s in range(S):
            assert (dps[s].cpu()[noterm[s]] == 0).all(), what
        if tau == 0.0:
            assert m.all() and (kept == 1).all()
        if tau == TAU_NONE:
            assert not m.any() and (out == 0).all() and all((dp == 0).all() for dp in dps)
        # values and gradients
        _check(out, v, vb + TINY, what + " map")
        # [0, 2 / C]: every fp32 probability vector sums to 1 within C U, so a squared distance is at most 2 (1 + C U)^2; on top the
        # value's own bound of (C + 2 S + 4) U
        assert (out.cpu().double() <= 2.0 / C * (1 + (3 * C + 2 * S + 6) * U)).all() and (out >= 0).all(), what
        for s in range(S):
            ref = dmap.double()[:, None] * d[s]
            _check(dps[s], ref, dmap.double().abs()[:, None] * db[s] + U * ref.abs() + TINY, what + f" dprobs {s}")
        if tau == 0.0 and teacher == "cross":
            # the sentinels (one-hot views of classes s % C): the closed form, which the fp32 arithmetic gives bit for bit
            want = _sentinel_value(S, C)
            np.testing.assert_allclose(v[sen].numpy(), want, rtol=1e-15)
            assert (out.cpu()[sen].double() - want).abs().max().item() <= 2 * U * want, what
            if S == 2:
                assert (out.cpu()[sen] == np.float32(2.0) / np.float32(C)).all(), what


@functools.lru_cache(maxsize=2)
def _softmax_and_conf(P, S, C, teacher):
    """hip_ops.softmax_fwd's probabilities of ``_logits`` (softmax_px's bits) as numpy, and the raw confidences at threshold 0."""
    from dct_amd import hip_ops
    sm = [hip_ops.softmax_fwd(x.to(DEV), C) for x in _logits(P, S, C)]
    pn = tuple(p.cpu().numpy() for p in sm)
    return tuple(sm), pn, PR.teachers_fp32(pn, teacher, 0.0)[2]


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
    sm, pn, q0 = _softmax_and_conf(P, S, C, teacher)
    sen, tie = _special(P)
    ws = ops._loss_ws(xs[0].device)
    for tau in _taus(q0, P):
        what = f"{teacher} P={P} S={S} C={C} tau={tau}"
        kw = dict(gscale=gs, gmul=gmul, teacher=mode, tau=tau)
        # straight through the library, every output NaN before
        out2, dls, probs = _nan(2), [_nan(P, C) for _ in range(S)], [_nan(P, C) for _ in range(S)]
        ops.call("dct_mse_logits_step", ops._ptr_array(xs), S, mode, tau, P, C, ops.ptr(out2), ops._ptr_array(probs), ops.ptr(gs), gmul,
                 ops._ptr_array(dls), 0, ops.ptr(ws), ws.numel(), ops.stream())
        out2w, probs_w = ops.mse_logits_step(xs, C, [_nan(P, C) for _ in range(S)], True, **kw)
        acc = [o.clone() for o in olds]
        out2a, none = ops.mse_logits_step(xs, C, acc, False, accumulate=True, **kw)
        out2n, probs_n = ops.mse_logits_step(xs, C, None, True, **kw)                 # dlogits=None
        out2p, none_p = ops.mse_logits_step(xs, C, None, False, **kw)                 # dlogits=None and probs=None
        torch.cuda.synchronize()
        # accumulate: the rounded gradient added to what was there, bit for bit; no gradients asked: the same values and maps
        assert none is None and none_p is None, what
        for o in (out2w, out2a, out2n, out2p):
            assert torch.equal(out2, o), what
        for s in range(S):
            assert torch.equal(acc[s], dls[s] + olds[s]), what
            assert torch.equal(probs[s], probs_n[s]) and torch.equal(probs[s], probs_w[s]), what
            assert torch.equal(probs[s], sm[s]), what                                   # softmax_fwd's bits
        if tau == TAU_NONE:
            # nothing kept: no float64 needed -- everything is exactly 0 and finite
            assert out2.tolist() == [0.0, 0.0] and all((dl == 0).all() for dl in dls), what
            continue
        m, v, vb, d, db = R.rule(pn, teacher, tau)
        # the kept fraction: whole numbers summed in fp32 (exact below 2^24), one fp32 division
        frac = np.float32(m.sum()) / np.float32(np.float32(P) * np.float32(kden))
        assert out2[1].item() == float(frac), (what, out2[1].item(), float(frac))
        if tau == 0.0:
            assert out2[1].item() == 1.0
        ref = v.mean().item()
        tol = (vb.sum().item() + SUM_DEPTH * U * v.abs().sum().item()) / P + 2 * U * abs(ref) + TINY
        assert abs(out2[0].item() - ref) <= tol, (what, out2[0].item(), ref, tol)
        noterm = torch.from_numpy(np.ascontiguousarray(_no_term(m, teacher, S)))
        for s in range(S):
            gref, gb = R.logit_grad(pn[s], d[s], db[s], gg, C)
            _check(dls[s], gref, gb, what + f" dlogits {s}")
            assert (dls[s].cpu()[noterm[s]] == 0).all(), what                           # a student without a teacher term: exactly 0
        if tau == 0.0 and teacher == "cross":
            # the sentinels are exactly one-hot after softmax_px, so the float64 value there is the closed form
            np.testing.assert_allclose(v[sen].numpy(), _sentinel_value(S, C), rtol=1e-15)


CLASS_SWEEP = [(S, C, teacher) for C in range(2, 9) for S in (1, 2, 3, 5) for teacher in TEACHERS if S > 1 or teacher == "ensemble"]


@pytest.mark.parametrize("S,C,teacher", CLASS_SWEEP)
def test_every_class_count_of_the_dispatch(ops, S, C, teacher):
    """The dispatch instantiates C = 2..8 and the grids above use 2, 4 and 8: the map kernels and the step kernel at every C, at 257
    pixels (one full block and a grid-stride tail of one pixel), S = 2, 3, 5 (every SMAX instantiation) and the ensemble's single
    view; the references, thresholds and bounds are the tests' above, which this runs as they are."""
    test_map_kernels(ops, 257, S, C, teacher)
    test_step_kernel(ops, 257, S, C, teacher)


@pytest.mark.parametrize("teacher,S", [("cross", 2), ("cross", 3), ("cross", 5), ("cross", 8), ("ensemble", 1), ("ensemble", 2)])
@pytest.mark.parametrize("C", [2, 4, 8])
def test_bitwise_equal_views_give_exactly_zero(ops, teacher, S, C):
    """Differences of two probabilities, never a total minus a share: views that agree bit for bit give exactly 0 everywhere (the cross
    teacher at any S; the ensemble at S = 1 and 2, where its fp32 mean is exact)."""
    P = 257
    g = torch.Generator().manual_seed(S + C)
    x = (torch.randn(P, C, generator=g) * 3).to(DEV)
    xs = [x.clone() for _ in range(S)]
    mode = ops.PL_TEACHERS[teacher]
    for tau in (0.0, 0.5):
        dls = [_nan(P, C) for _ in range(S)]
        out2, probs = ops.mse_logits_step(xs, C, dls, True, gmul=1e6, teacher=mode, tau=tau)
        old = torch.randn(P, C, generator=g).to(DEV)
        acc = [old.clone() for _ in range(S)]
        ops.mse_logits_step(xs, C, acc, False, gmul=1e6, accumulate=True, teacher=mode, tau=tau)
        mp, kept = ops.mse_map_fwd(probs, C, teacher=mode, tau=tau)
        dps = ops.mse_map_bwd(probs, torch.full((P,), HUGE, device=DEV), C, teacher=mode, tau=tau)
        torch.cuda.synchronize()
        assert out2[0].item() == 0.0 and 0.0 <= out2[1].item() <= 1.0 and (tau or out2[1].item() == 1.0)
        assert all((dl == 0).all() for dl in dls) and all(torch.equal(a, old) for a in acc)
        assert (mp == 0).all() and all((dp == 0).all() for dp in dps)


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

    def fwd(S_=S, t=0, tau=0.5, a=arr, m_=mp.data_ptr(), P_=P, C_=C):
        return lib.dct_mse_map_fwd(a, S_, t, tau, m_, None, P_, C_, st)

    def bwd(S_=S, t=0, tau=0.5, a=arr, dm=mp.data_ptr(), o=oarr, P_=P, C_=C):
        return lib.dct_mse_map_bwd(a, S_, t, tau, dm, o, P_, C_, st)

    def step(S_=S, t=0, tau=0.5, a=arr, P_=P, C_=C, o2=out2.data_ptr(), w=ws.data_ptr(), wb=ws.numel(), dl=None):
        return lib.dct_mse_logits_step(a, S_, t, tau, P_, C_, o2, None, None, 1.0, dl, 0, w, wb, st)

    for f in (fwd, bwd, step):
        assert f() == 0 and f(t=1) == 0 and f(S_=1, t=1) == 0 and f(tau=float("inf")) == 0 and f(tau=0.0) == 0
        assert f(S_=1, t=0) == BAD and f(S_=0, t=1) == BAD and f(S_=9) == BAD and f(S_=9, t=1) == BAD     # S outside the mode's range
        assert f(t=2) == BAD and f(t=-1) == BAD                                                          # an unknown mode
        assert f(tau=-0.1) == BAD and f(tau=float("nan")) == BAD
        assert f(a=None) == BAD and f(a=nullarr) == BAD and f(P_=0) == BAD and f(P_=-5) == BAD
        assert f(C_=1) == UNS and f(C_=9) == UNS and f(C_=0) == UNS
    assert fwd(m_=None) == BAD and bwd(dm=None) == BAD and bwd(o=None) == BAD and bwd(o=nullarr) == BAD and step(o2=None) == BAD
    assert step(dl=oarr) == 0 and step(dl=nullarr) == BAD
    assert step(w=None) == WSP and step(wb=16) == WSP and step(wb=ws.numel() - 1) == WSP
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,teacher", [("cross_mse", "cross"), ("mean_mse", "ensemble")])
def test_module_through_autograd_equals_the_raw_ops(ops, name, teacher):
    from dct_amd.loss import get_loss_fn
    B, C, H, W, S = 2, 4, 9, 13, 3
    g = torch.Generator().manual_seed(5)
    logits = [(torch.randn(B, C, H, W, generator=g) * 3).to(DEV) for _ in range(S)]
    leaves = [torch.softmax(x, 1).requires_grad_(True) for x in logits]
    q = PR.teachers_fp32([p.detach().permute(0, 2, 3, 1).reshape(-1, C).cpu().numpy() for p in leaves], teacher, 0.0)[2]
    tau = _taus(q, B * H * W)[1]
    crit = get_loss_fn(name, threshold=tau)
    out = crit(leaves)
    assert out.shape == (B, H, W) and torch.is_tensor(crit.last_kept) and crit.last_kept.is_cuda and crit.last_kept.dim() == 0
    seed = torch.randn(B, H, W, generator=g).to(DEV)
    (out * seed).sum().backward()
    pcs = [p.detach().permute(0, 2, 3, 1).contiguous() for p in leaves]
    assert crit.launch_args() == dict(teacher=ops.PL_TEACHERS[teacher], tau=tau)
    mp, kept = ops.mse_map_fwd(pcs, C, **crit.launch_args())
    dps = ops.mse_map_bwd(pcs, seed.reshape(-1).contiguous(), C, **crit.launch_args())
    other, _ = ops.mse_map_fwd(pcs, C, **dict(crit.launch_args(), tau=0.0))
    torch.cuda.synchronize()
    assert torch.equal(out.detach().reshape(-1), mp) and not torch.equal(mp, other)       # (the threshold reaches the kernel)
    assert torch.equal(crit.last_kept, kept.mean()) and 0.2 <= crit.last_kept.item() <= 0.8
    for p, dp in zip(leaves, dps):
        assert torch.equal(p.grad.permute(0, 2, 3, 1).reshape(-1, C), dp.reshape(-1, C))
    assert torch.isfinite(out.mean()) and (out >= 0).all() and (out <= 2.0 / C).all()
    if teacher == "cross":
        with pytest.raises(ValueError, match="at least 2 views"):
            crit(leaves[:1])
    else:
        alone = crit(leaves[:1])
        assert alone.shape == (B, H, W) and (alone == 0).all()                              # S = 1 ensemble is exactly 0
