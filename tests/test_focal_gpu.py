"""The focal loss kernels (``dct_focal_*``, include/dct.h) and ``FocalLoss2d`` on top of them, against the float64 reference of
tests/focal_ref.py (plain torch, autograd for the gradients) computed from exactly the fp32 logits and fp32 weights the kernels see.

The method is tests/test_weighted_ce_gpu.py's: sentinel pixels at the seams of both grids (target logit -D: q = 1, so a sentinel is
worth w (D + log(C - 1)) under every gamma), each worth more than four times the value bound and on a class of non-zero weight;
per-pixel outputs pre-filled with NaN; every tolerance derived.  With U the fp32 unit roundoff, SUM_DEPTH the levels of the kernels'
reduction and e_i the per-pixel bound -- here ``Ref.ef``: f_i (eps_m + eps_l + 2 U) + TINY max(1, w_i) in place of
``test_ce_at_scale``'s absolute e_i, which at a confident pixel (l ~ 1e-9) would let any l pass --:
  * numerator N = sum f_i:    sum e_i + SUM_DEPTH U N;
  * denominator D = sum w_i:  SUM_DEPTH U D;
  * mean N / D:               the numerator's bound / D + (SUM_DEPTH + 2) U |ref|;
  * map f_i:                  e_i;
  * gradient (g w_i k_i) v_c: |g w_i k_i v_c| (eps_k + eps_v + eps_g + 3 U) + TINY max(1, |g w_i|); the accumulate adds U |old + d|.
The factors' terms -- eps_q (the relative error of q, summed off the target), eps_l, eps_m = gamma eps_q + 7 U gamma |ln q| + T (the
error of q^gamma), eps_k, eps_v, eps_g -- are derived line by line in the docstring of tests/focal_ref.py, which evaluates them, and
tests/test_focal_cpu.py holds a float32 evaluation on the CPU to them on the inputs below.

Pixel counts: 1, 255, 257 (partial blocks), 262,145 (one past ``grid_for``'s 1024 blocks: a thread takes a second trip) and, in two
cases, 2,097,153 (one past ``wide_grid``'s 8192, the backward kernels' grid); 262,401 at every C from 2 to 8.  C otherwise: 2, 3, 4, 8; gamma: 0, 0.5, 1, 2, 5, spread over the
cases.  A quarter of the targets are 255, some cases carry stray targets (C, -1).  Every case plants confident pixels and checks them
by name: the target logit 20 and 40 above the rest (q ~ 1e-9, ~ 1e-17), 120 above (q = 0 in fp32: value and gradient exactly 0 under
gamma > 0, the cross entropy's under gamma = 0, everything finite), and 150 below (p_t = 0 in fp32, q = 1).

Measured max error / bound on an MI355X (the printed ratios: profiles/focal_loss.txt)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_loss_kernels_scale_gpu import DEV, IGN, SUM_DEPTH, U, _check, _nan, _sentinels  # noqa: E402

import focal_ref as R  # noqa: E402

MEAN, SUM = R.MEAN, R.SUM
assert (R.U, R.SUM_DEPTH, R.IGN) == (U, SUM_DEPTH, IGN)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _ratio(got, ref, bound):
    return ((got.detach().cpu().double() - ref).abs() / bound.clamp(min=1e-300)).max().item()


# every C from 2 to 8 at 1024 * 256 + 257 pixels (the forward grid's second trip ends in a ragged block): the kernels are one template per
# role over the pixel rule, and "the step is fwd followed by bwd, bit for bit" below is held at every C it is instantiated for
STEP_CASES = [
    (262401, 2, 2.0, MEAN, True, False, True), (262401, 3, 0.5, SUM, False, False, True), (262401, 4, 0.0, MEAN, False, True, False),
    (262401, 5, 2.0, SUM, True, False, True), (262401, 6, 0.5, MEAN, False, False, False), (262401, 7, 1.0, MEAN, True, True, True),
    (262401, 8, 2.0, MEAN, False, False, True),
]


@pytest.mark.parametrize("P,C,gamma,reduction,accumulate,stray,weighted", R.CASES + STEP_CASES)
def test_focal_at_scale(ops, P, C, gamma, reduction, accumulate, stray, weighted):
    w = R.weights(C, alt=reduction == SUM) if weighted else torch.ones(C)
    g, x, t, t_ref, sen, plants = R.inputs(P, C, w, stray, seed=P + 7 * C + reduction)
    assert torch.equal(sen, _sentinels(P))
    r = R.Ref(x, t_ref, w, C, gamma)
    loss, tol = r.value(reduction)
    ref = loss.item()
    assert (r.wi[sen] > 0).all()
    lost = r.f[sen].min().item() / (r.D if reduction == MEAN else 1.0)
    assert lost > 4 * tol, (lost, tol)                                  # one lost sentinel is far outside the bound

    gscale, gmul = 0.61, 8.0
    gg = float(np.float32(gscale)) * gmul
    old = torch.randn(P, C, generator=g) if accumulate else None
    dref, dbound = r.grad(loss * gg, gg / r.D if reduction == MEAN else gg, mean=reduction == MEAN, old=old)
    dmap = torch.randn(P, generator=g)
    mref, mbound = r.grad(r.fmap, gmul * dmap.double(), per_pixel=True, old=old, grad_outputs=gmul * dmap.double())

    xg, tg = x.to(DEV), t.to(DEV)
    wg = w.to(DEV) if weighted else None
    gs = torch.tensor([gscale], device=DEV)

    def fresh():
        return old.to(DEV) if accumulate else _nan(P, C)
    out = ops.focal_fwd(xg, tg, C, wg, gamma, reduction, IGN)
    d1 = ops.focal_bwd(xg, tg, C, out[1:2], fresh(), weight=wg, gamma=gamma, reduction=reduction, gscale=gs, gmul=gmul, ignore_index=IGN,
                       accumulate=accumulate)
    d2 = fresh()
    out2 = ops.focal_step(xg, tg, C, d2, weight=wg, gamma=gamma, reduction=reduction, gscale=gs, gmul=gmul, ignore_index=IGN,
                          accumulate=accumulate)
    m = _nan(P)
    ops.call("dct_focal_map_fwd", ops.ptr(xg), ops.ptr(tg), P, C, IGN, ops.ptr(wg), float(gamma), ops.ptr(m), ops.stream())
    d3 = ops.focal_map_bwd(xg, tg, C, dmap.to(DEV), fresh(), weight=wg, gamma=gamma, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    torch.cuda.synchronize()
    print(f"focal P={P} C={C} gamma={gamma} {R.RED[reduction]} {'weighted' if weighted else 'NULL'}: ref {ref!r} tol {tol:.3e}; value err / tol "
          f"{abs(out[0].item() - ref) / tol:.3f}; denominator err {abs(out[1].item() - r.D):.3e} of {SUM_DEPTH * U * r.D:.3e}; max err / "
          f"bound: map {_ratio(m, r.f, r.ef):.3f}, gradient {_ratio(d1, dref, dbound):.3f}, map gradient {_ratio(d3, mref, mbound):.3f}")
    for o, what in ((out, "focal_fwd"), (out2, "focal_step")):
        assert abs(o[1].item() - r.D) <= SUM_DEPTH * U * r.D, (what, o[1].item(), r.D)
        assert abs(o[0].item() - ref) <= tol, (what, o[0].item(), ref, tol)
    assert torch.equal(out, out2) and torch.equal(d1, d2)               # the step is fwd followed by bwd, bit for bit
    _check(d1, dref, dbound, "focal_bwd")
    _check(d2, dref, dbound, "focal_step gradient")
    _check(m, r.f, r.ef, "focal_map_fwd")
    _check(d3, mref, mbound, "focal_map_bwd")
    # ignored and stray pixels: nothing in the map, exactly nothing (exactly the old value) in the gradients
    gone = ~r.keep
    mc, d1c, d3c = m.cpu(), d1.cpu(), d3.cpu()
    if gone.any():
        want = old[gone] if accumulate else torch.zeros(int(gone.sum()), C)
        assert torch.equal(mc[gone], torch.zeros(int(gone.sum())))
        for d in (d1c, d3c):
            assert torch.equal(d[gone], want)
    # the planted pixels, by name
    for name, lo, hi in (("c20", 1e-10, 1e-7), ("c40", 1e-19, 1e-15)):
        i = plants[name]
        if len(i):
            assert bool(((r.q[i] > lo) & (r.q[i] < hi)).all()) and bool((r.wi[i] > 0).all()) and bool((r.f[i] > 0).all())
            rel = ((mc[i].double() - r.f[i]).abs() / r.f[i]).max().item()
            allowed = (r.ef[i] / r.f[i]).max().item()
            assert rel <= allowed, (name, rel, allowed)          # (relative: f_i eps_f, plus the TINY floor where f_i is below the fp32 range)
    i = plants["c120"]
    if len(i):
        zero = torch.zeros(len(i), C)
        if gamma > 0:
            assert torch.equal(mc[i], torch.zeros(len(i)))
            for d in (d1c, d3c):
                assert torch.equal(d[i], old[i] if accumulate else zero)
        else:
            assert bool((r.f[i] < R.TINY).all())                       # the cross entropy of such a pixel: below the fp32 range
    i = plants["low"]
    if len(i):
        assert bool((r.q[i] > 1 - 1e-12).all()) and bool((r.l[i] > 149).all())
    for what, v in (("map", mc), ("gradient", d1c), ("map gradient", d3c), ("value", out.cpu())):
        assert bool(torch.isfinite(v).all()), what


@pytest.mark.parametrize("P,C,weighted", [(257, 4, True), (262145, 3, True), (262145, 2, False)])
def test_gamma_zero_agrees_with_the_weighted_cross_entropy(ops, P, C, weighted):
    """gamma = 0 is the class-weighted cross entropy computed another way (l by -log1p(-q) or from two non-negative terms, the target's
    gradient entry as -q): the two agree within the sum of the two derived bounds, value, map and gradients, under both reductions."""
    w = R.weights(C) if weighted else torch.ones(C)
    g, x, t, t_ref, sen, _ = R.inputs(P, C, w, False, seed=5 * P + C)
    r = R.Ref(x, t_ref, w, C, 0.0)
    ce_num_tol, ce_map_bound, ce_grad_bound = R.ce_bounds(r)
    xg, tg = x.to(DEV), t.to(DEV)
    wg = w.to(DEV) if weighted else None
    gs = torch.tensor([0.61], device=DEV)
    gg = float(np.float32(0.61)) * 8.0
    for reduction in (MEAN, SUM):
        loss, tol = r.value(reduction)
        ce_tol = ce_num_tol / r.D + (SUM_DEPTH + 2) * U * abs(loss.item()) if reduction == MEAN else ce_num_tol
        a = ops.focal_fwd(xg, tg, C, wg, 0.0, reduction, IGN)
        b = ops.ce_weighted_fwd(xg, tg, C, wg, reduction, IGN)
        assert abs(a[0].item() - b[0].item()) <= tol + ce_tol, (a[0].item(), b[0].item(), tol, ce_tol)
        assert abs(a[1].item() - b[1].item()) <= 2 * SUM_DEPTH * U * r.D
        da = ops.focal_bwd(xg, tg, C, a[1:2], _nan(P, C), weight=wg, gamma=0.0, reduction=reduction, gscale=gs, gmul=8.0, ignore_index=IGN)
        db = ops.ce_weighted_bwd(xg, tg, C, b[1:2], _nan(P, C), weight=wg, reduction=reduction, gscale=gs, gmul=8.0, ignore_index=IGN)
        gfac = gg / r.D if reduction == MEAN else gg
        _, fb = r.grad(loss, gfac, mean=reduction == MEAN)
        _check(da, db.cpu().double(), fb + ce_grad_bound(gfac, 6 if reduction == MEAN else 5), f"gradient, reduction {reduction}")
    ma, mb = ops.focal_map_fwd(xg, tg, C, wg, 0.0, IGN), ops.ce_map_fwd(xg, tg, C, wg, IGN)
    _check(ma, mb.cpu().double(), r.ef + ce_map_bound, "map")
    torch.cuda.synchronize()


@pytest.mark.parametrize("P,C,gamma", [(257, 4, 2.0), (262145, 3, 0.0)])
def test_focal_mean_without_weight_is_nan(ops, P, C, gamma):
    """Every target ignored, or every weight zero, under the mean: 0 / 0 = NaN as the weighted cross entropy gives, and a denominator
    of exactly 0; the sum is exactly 0.  Two runs are bit-identical."""
    g = torch.Generator().manual_seed(3 + P)
    x = torch.randn(P, C, generator=g)
    t = torch.randint(0, C, (P,), generator=g)
    zeros = torch.zeros(C)
    xg = x.to(DEV)
    for tt, w in ((t, zeros), (torch.full_like(t, IGN), R.weights(C))):
        ce = ops.ce_weighted_fwd(xg, tt.to(DEV), C, w.to(DEV), MEAN, IGN)
        assert math.isnan(ce[0].item())
        for o in (ops.focal_fwd(xg, tt.to(DEV), C, w.to(DEV), gamma, MEAN, IGN),
                  ops.focal_step(xg, tt.to(DEV), C, _nan(P, C), weight=w.to(DEV), gamma=gamma, reduction=MEAN, ignore_index=IGN)):
            assert math.isnan(o[0].item()) and o[1].item() == 0.0
        o = ops.focal_fwd(xg, tt.to(DEV), C, w.to(DEV), gamma, SUM, IGN)
        assert o[0].item() == 0.0 and o[1].item() == 0.0
    w = R.weights(C).to(DEV)
    tg = t.to(DEV)
    runs = []
    for _ in range(2):
        d = _nan(P, C)
        o = ops.focal_step(xg, tg, C, d, weight=w, gamma=gamma, gmul=8.0, ignore_index=IGN)
        runs.append((o, d, ops.focal_map_fwd(xg, tg, C, w, gamma, IGN)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_focal_status_codes(ops):
    P, C = 64, 3
    x = torch.zeros(P, C, device=DEV)
    t = torch.zeros(P, dtype=torch.int64, device=DEV)
    w = torch.ones(8, device=DEV)
    out, dl, m = torch.zeros(2, device=DEV), torch.zeros(P, 9, device=DEV), torch.zeros(P, device=DEV)
    ws = ops._loss_ws(DEV)
    p, st = ops.ptr, ops.stream

    def fwd(**k):
        return ["dct_focal_fwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("gamma", 2.0),
                k.get("red", 0), k.get("out", p(out)), p(ws), k.get("wsb", ws.numel()), st()]

    def bwd(**k):
        return ["dct_focal_bwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("gamma", 2.0),
                k.get("red", 0), k.get("den", p(out[1:2])), None, 1.0, k.get("dl", p(dl)), 0, st()]

    def step(**k):
        return ["dct_focal_step", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("gamma", 2.0),
                k.get("red", 0), k.get("out", p(out)), None, 1.0, k.get("dl", p(dl)), 0, p(ws), k.get("wsb", ws.numel()), st()]

    def mfwd(**k):
        return ["dct_focal_map_fwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("gamma", 2.0),
                k.get("out", p(m)), st()]

    def mbwd(**k):
        return ["dct_focal_map_bwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("gamma", 2.0),
                k.get("dm", p(m)), 1.0, k.get("dl", p(dl)), 0, st()]
    for f in (fwd, bwd, step, mfwd, mbwd):
        ops.call(*f())
        ops.call(*f(gamma=0.0))
        bad = [dict(x=None), dict(t=None), dict(P=0), dict(gamma=-1.0), dict(gamma=-1e-30), dict(gamma=float("nan")), dict(gamma=float("inf"))]
        bad += [dict(red=2), dict(red=-1)] if f in (fwd, bwd, step) else []
        bad += [dict(out=None)] if f in (fwd, step, mfwd) else []
        bad += [dict(dl=None)] if f in (bwd, step, mbwd) else []
        bad += [dict(dm=None)] if f is mbwd else []
        bad += [dict(den=None)] if f is bwd else []
        for b in bad:
            with pytest.raises(RuntimeError, match=r"status -1"):
                ops.call(*f(**b))
        for b in (dict(C=1), dict(C=9)):
            with pytest.raises(RuntimeError, match=r"status -2"):
                ops.call(*f(**b))
        if f in (fwd, step):
            with pytest.raises(RuntimeError, match=r"status -4"):
                ops.call(*f(wsb=ws.numel() - 4))
    ops.call(*bwd(red=1, den=None))          # the sum's denominator is 1: none is read
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("C,gamma", [(2, 2.0), (4, 0.5)])
@pytest.mark.parametrize("kw,strided", [(dict(), False), (dict(size_average=False), False), (dict(reduce=False), False),
                                        (dict(), True), (dict(reduce=False, size_average=False), True)])
def test_module_against_the_reference(ops, C, gamma, kw, strided):
    """FocalLoss2d(gamma, weight, reduce, size_average) and its backward at [2, C, 16, 24] with an upstream gradient that is not 1
    ((3 loss).backward(); a random dmap for the map), once through a non-contiguous NCHW input; bounds as for the kernels.  Then the
    same module again after an in-place change of its device weights."""
    from dct_amd.loss import FocalLoss2d
    B, H, W = 2, 16, 24
    g = torch.Generator().manual_seed(17 + C + len(kw))
    w = R.weights(C)
    crit = FocalLoss2d(gamma=gamma, weight=w.tolist(), **kw)
    red = crit.reduction
    x = torch.randn(B, C, H, 2 * W if strided else W, generator=g) * 2
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.25] = IGN
    leaf = x.to(DEV).requires_grad_(True)
    inp = leaf[..., ::2] if strided else leaf
    assert inp.is_contiguous() != strided
    xs = x[..., ::2] if strided else x
    flat = xs.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    r = R.Ref(flat, t.reshape(-1), w, C, gamma)
    got = crit(inp, t.to(DEV))
    if red == "none":
        assert got.shape == (B, H, W)
        dmap = torch.randn(B, H, W, generator=g)
        got.backward(dmap.to(DEV))
        _check(got.reshape(-1), r.f, r.ef, "map")
        dref, bound = r.grad(r.fmap, dmap.double().reshape(-1), per_pixel=True, grad_outputs=dmap.double().reshape(-1))
    else:
        reduction = MEAN if red == "mean" else SUM
        (3 * got).backward()
        loss, tol = r.value(reduction)
        assert got.dim() == 0 and abs(got.item() - loss.item()) <= tol, (got.item(), loss.item(), tol)
        dref, bound = r.grad(3 * loss, 3.0 / r.D if reduction == MEAN else 3.0, mean=reduction == MEAN)
    torch.cuda.synchronize()
    gx = leaf.grad[..., ::2] if strided else leaf.grad
    _check(gx.permute(0, 2, 3, 1).reshape(-1, C), dref, bound, f"{red} gradient")
    if strided:
        assert torch.equal(leaf.grad[..., 1::2], torch.zeros_like(leaf.grad[..., 1::2]))
    # the device copy of the weights is made once and is what the kernels read: an in-place change of it changes the next call
    buf = crit.device_weight(DEV, C)
    assert buf is crit.device_weight(DEV) and buf.dtype == torch.float32 and torch.equal(buf.cpu(), w)
    buf.mul_(2.0)
    again = crit(inp.detach(), t.to(DEV))
    scale = 1.0 if red == "mean" else 2.0           # the mean is invariant to the weights' scale, up to rounding
    np.testing.assert_allclose(again.cpu().numpy(), scale * got.detach().cpu().numpy(), rtol=1e-5)


def test_module_runs_the_focal_kernels_at_gamma_zero(ops, monkeypatch):
    """No hand-over to the cross-entropy kernels: gamma = 0 and unit weights still call dct_focal_*."""
    from dct_amd.loss import CrossEntropyLoss2d, FocalLoss2d
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 16, 24, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(0, 3, (2, 16, 24), generator=g).to(DEV)
    seen = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    for kw in (dict(), dict(size_average=False), dict(reduce=False)):
        out = FocalLoss2d(gamma=0, weight=[1, 1, 1], **kw)(x, t)
        out.sum().backward()
        want = CrossEntropyLoss2d(**kw)(x.detach(), t)
        np.testing.assert_allclose(out.detach().cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    names = [n for n in seen if "focal" in n]
    assert names == ["dct_focal_fwd", "dct_focal_bwd"] * 2 + ["dct_focal_map_fwd", "dct_focal_map_bwd"], seen
    with pytest.raises(ValueError, match="FocalLoss2d: 4 class weights for logits of 3 classes"):
        FocalLoss2d(weight=[0.1, 1, 2.5, 0])(x, t)
