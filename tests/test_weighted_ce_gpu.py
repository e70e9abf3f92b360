"""Class-weighted cross entropy, its sum reduction and its per-pixel map (``dct_ce_weighted_*`` / ``dct_ce_map_*``, include/dct.h) and
``CrossEntropyLoss2d(weight, reduce, size_average)`` on top of them, against ``F.cross_entropy(x.double(), t, weight=w.double(),
ignore_index=255, reduction=...)`` and its autograd gradient on the CPU, from exactly the fp32 logits and fp32 weights the kernels see.

The method is tests/test_loss_kernels_scale_gpu.py's: sentinel pixels at the seams of both grids, each worth more than four times the
bound; per-pixel outputs pre-filled with NaN; every tolerance derived (U: fp32 unit roundoff, SUM_DEPTH: the levels of the kernels'
reduction, e_i: the per-pixel bound of ``test_ce_at_scale``):
  * numerator N = sum w_i l_i:   sum w_i e_i + (SUM_DEPTH + 1) U N    (one U more than the unweighted sum: the product w_i l_i);
  * denominator D = sum w_i:     SUM_DEPTH U D                          (the weights are exact, their fp32 sum is not);
  * mean N / D:                  the numerator's bound / D + (SUM_DEPTH + 2) U |ref|   (the fp32 sum of the weights and the division);
  * map w_i l_i:                 w_i e_i + U w_i l_i;
  * gradient (g w_i)(p_c - [t_i == c]):   ``test_ce_at_scale``'s |g| ((C + 6 + |x_c - m|) U p_c + 4 U |p_c - 1_t|) with |g w_i| for |g| and
    5 U for 4 U (the product g w_i), 6 U under the mean (its denominator is an fp32 sum); the accumulate adds U |old + d|.
Pixel counts: 1, 255, 257 (partial blocks), 262,145 (one past ``grid_for``'s 1024 blocks: a thread takes a second trip) and 2,097,153
(one past ``wide_grid``'s 8192).  Weights: a non-dyadic value, a one, a zero and one above 1, cycled to C (C = 2 has room for two of
them: 0.1 and 1 under the mean, 2.5 and 0 under the sum); a quarter of the targets are 255."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_loss_kernels_scale_gpu import DEV, IGN, SUM_DEPTH, U, _check, _nan, _sentinels, _sm64  # noqa: E402

MEAN, SUM = 0, 1
RED = {MEAN: "mean", SUM: "sum"}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _weights(C, alt=False):
    if C == 2:
        return torch.tensor([2.5, 0.0] if alt else [0.1, 1.0], dtype=torch.float32)
    return torch.tensor([(0.1, 1.0, 0.0, 2.5)[c % 4] for c in range(C)], dtype=torch.float32)


def _inputs(P, C, w, stray, seed):
    """fp32 logits [P, C], targets (a quarter ignored; ``stray``: a few are C and -1), the targets the reference may see (the stray ones
    ignored: torch raises on them) and the sentinels: target logit -D, the others 0 -> l = D + log(C - 1), on classes of non-zero weight."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g) * 2
    t = torch.randint(0, C, (P,), generator=g)
    t[torch.rand(P, generator=g) < 0.25] = IGN
    if stray:
        idx = (torch.arange(6) * P // 7 + 1) % P
        t[idx[:3]] = C
        t[idx[3:]] = -1
    sen = _sentinels(P)
    nz = torch.nonzero(w)[:, 0]
    D = max(1e4, 0.1 * P)
    t[sen] = nz[sen % len(nz)]
    x[sen] = 0.0
    x[sen, t[sen]] = -D
    t_ref = torch.where((t < 0) | (t >= C), torch.full_like(t, IGN), t)
    if stray:
        assert int(((t != IGN) & (t_ref == IGN)).sum()) >= 3
    return g, x, t, t_ref, sen


class _Ref:
    """float64 reference of one (x, t, w): F.cross_entropy and autograd, plus the per-pixel pieces the bounds are made of."""

    def __init__(self, x, t_ref, w, C):
        self.C, self.wd = C, w.double()
        self.xd = x.double().requires_grad_(True)
        self.t = t_ref
        self.keep = t_ref != IGN
        tc = t_ref.clamp(max=C - 1)
        with torch.no_grad():
            xd = self.xd
            self.wi = torch.where(self.keep, self.wd[tc], torch.zeros((), dtype=torch.float64))
            l = torch.where(self.keep, torch.logsumexp(xd, 1) - xd.gather(1, tc[:, None])[:, 0], torch.zeros((), dtype=torch.float64))
            amax = xd.abs().max(1).values
            # per pixel (test_ce_at_scale): |e_i| <= (C + 8) U (3 max|x| + log C + l_i + 1)
            self.e = torch.where(self.keep, (C + 8) * U * (3 * amax + math.log(C) + l + 1), torch.zeros((), dtype=torch.float64))
            self.wl = self.wi * l
            self.N, self.D = self.wl.sum().item(), self.wi.sum().item()
            self.num_tol = (self.wi * self.e).sum().item() + (SUM_DEPTH + 1) * U * self.N
            self.p, self.spread = _sm64(x)
            self.onehot = F.one_hot(tc, C).double()

    def value(self, reduction):
        """(loss as a float64 tensor with a graph, tolerance)"""
        loss = F.cross_entropy(self.xd, self.t, weight=self.wd, ignore_index=IGN, reduction=RED[reduction])
        if reduction == MEAN:
            return loss, self.num_tol / self.D + (SUM_DEPTH + 2) * U * abs(loss.item())
        return loss, self.num_tol

    def grad(self, loss, gfac, k, old=None, grad_outputs=None):
        """gfac * dloss/dx (+ old) and its bound; ``gfac``: per pixel [P] or scalar, the factor g of (g w_i)(p - onehot)."""
        (d,) = torch.autograd.grad(loss, self.xd, grad_outputs=grad_outputs)
        gw = (torch.as_tensor(gfac, dtype=torch.float64) * self.wi).abs().reshape(-1, 1)
        bound = torch.where(self.keep[:, None], gw * ((self.C + 6 + self.spread) * U * self.p + k * U * (self.p - self.onehot).abs()) + 1e-30,
                            torch.zeros((), dtype=torch.float64))
        if old is not None:
            d = d + old.double()
            bound = bound + U * d.abs()
        return d, bound


CASES = [  # P, C, reduction, accumulate, stray targets
    (1, 2, MEAN, False, False), (1, 3, SUM, True, False), (255, 3, SUM, False, False), (255, 8, MEAN, True, False),
    (257, 4, MEAN, True, True), (257, 2, SUM, False, False), (262145, 2, SUM, True, False), (262145, 4, MEAN, False, False),
    (262145, 8, SUM, False, True), (262145, 3, MEAN, True, False), (2097153, 3, MEAN, False, False), (2097153, 4, SUM, True, False),
    (2097153, 2, MEAN, True, False), (2097153, 8, SUM, False, False),
]


@pytest.mark.parametrize("P,C,reduction,accumulate,stray", CASES)
def test_weighted_ce_at_scale(ops, P, C, reduction, accumulate, stray):
    w = _weights(C, alt=reduction == SUM)
    g, x, t, t_ref, sen = _inputs(P, C, w, stray, seed=P + 7 * C + reduction)
    r = _Ref(x, t_ref, w, C)
    loss, tol = r.value(reduction)
    ref = loss.item()
    np.testing.assert_allclose(ref, r.N / r.D if reduction == MEAN else r.N, rtol=1e-12)       # torch's rule is include/dct.h's
    assert (r.wi[sen] > 0).all()
    lost = r.wl[sen].min().item() / (r.D if reduction == MEAN else 1.0)
    assert lost > 4 * tol, (lost, tol)                                  # one lost sentinel is far outside the bound

    gscale, gmul = 0.61, 8.0
    gg = float(np.float32(gscale)) * gmul
    old = torch.randn(P, C, generator=g) if accumulate else None
    # g = gscale gmul / D: the factor of the reference's own gradient is gscale gmul (autograd divides by D under the mean)
    dref, dbound = r.grad(loss * gg, gg / r.D if reduction == MEAN else gg, 6 if reduction == MEAN else 5, old)
    dmap = torch.randn(P, generator=g)
    lmap = F.cross_entropy(r.xd, r.t, weight=r.wd, ignore_index=IGN, reduction="none")
    # (torch's map is the reference; the pieces the bounds are made of agree with it to float64's rounding of logsumexp(x) - x_t)
    np.testing.assert_allclose(r.wl.numpy(), lmap.detach().numpy(), rtol=1e-9, atol=1e-12)
    mref, mbound = r.grad(lmap, gmul * dmap.double(), 5, old, grad_outputs=gmul * dmap.double())

    xg, tg, wg = x.to(DEV), t.to(DEV), w.to(DEV)
    gs = torch.tensor([gscale], device=DEV)

    def fresh():
        return old.to(DEV) if accumulate else _nan(P, C)
    out = ops.ce_weighted_fwd(xg, tg, C, wg, reduction, IGN)
    d1 = ops.ce_weighted_bwd(xg, tg, C, out[1:2], fresh(), weight=wg, reduction=reduction, gscale=gs, gmul=gmul, ignore_index=IGN,
                             accumulate=accumulate)
    d2 = fresh()
    out2 = ops.ce_weighted_step(xg, tg, C, d2, weight=wg, reduction=reduction, gscale=gs, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    m = _nan(P)
    ops.call("dct_ce_map_fwd", ops.ptr(xg), ops.ptr(tg), P, C, IGN, ops.ptr(wg), ops.ptr(m), ops.stream())
    d3 = ops.ce_map_bwd(xg, tg, C, dmap.to(DEV), fresh(), weight=wg, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    torch.cuda.synchronize()
    print(f"P={P} C={C} {RED[reduction]}: ref {ref!r} tol {tol:.3e}; fwd err {abs(out[0].item() - ref):.3e}, denominator err "
          f"{abs(out[1].item() - r.D):.3e} of {SUM_DEPTH * U * r.D:.3e}; max gradient err / bound "
          f"{((d1.cpu().double() - dref).abs() / dbound.clamp(min=1e-300)).max().item():.3f}")
    for o, what in ((out, "ce_weighted_fwd"), (out2, "ce_weighted_step")):
        assert abs(o[1].item() - r.D) <= SUM_DEPTH * U * r.D, (what, o[1].item(), r.D)
        assert abs(o[0].item() - ref) <= tol, (what, o[0].item(), ref, tol)
    assert torch.equal(out, out2) and torch.equal(d1, d2)               # the step is fwd followed by bwd, bit for bit
    _check(d1, dref, dbound, "ce_weighted_bwd")
    _check(d2, dref, dbound, "ce_weighted_step gradient")
    _check(m, lmap.detach(), r.wi * r.e + U * r.wl, "ce_map_fwd")
    _check(d3, mref, mbound, "ce_map_bwd")
    # ignored and stray pixels: nothing in the map, exactly nothing (exactly the old value) in the gradients
    gone = ~r.keep
    if gone.any():
        want = old[gone] if accumulate else torch.zeros(int(gone.sum()), C)
        assert torch.equal(m.cpu()[gone], torch.zeros(int(gone.sum())))
        for d in (d1, d3):
            assert torch.equal(d.cpu()[gone], want)


# (262401 = 1024 * 256 + 257: the forward grid's second trip ends in a ragged block; there every C the kernel templates are instantiated for)
@pytest.mark.parametrize("P,C", [(1, 2), (255, 3), (257, 8), (262145, 4), (2097153, 2), (2097153, 3)] + [(262401, C) for C in range(2, 9)])
def test_weighted_ce_identities(ops, P, C):
    """All-ones weights under the mean are dct_ce_step bit for bit (out2 and dlogits, both accumulate values, gscale set, gmul = 8);
    weight = NULL is all ones; dct_ce_weighted_step is fwd followed by bwd under both reductions; two runs are bit-identical."""
    g = torch.Generator().manual_seed(41 * P + C)
    x = (torch.randn(P, C, generator=g) * 2).to(DEV)
    t = torch.randint(0, C, (P,), generator=g)
    t[torch.rand(P, generator=g) < 0.25] = IGN
    t[0] = 0
    t = t.to(DEV)
    ones = torch.ones(C, device=DEV)
    w = _weights(C).to(DEV)
    gs = torch.tensor([0.61], device=DEV)
    for acc in (False, True):
        old = torch.randn(P, C, generator=g).to(DEV)

        def fresh():
            return old.clone() if acc else _nan(P, C)
        kw = dict(gscale=gs, gmul=8.0, ignore_index=IGN, accumulate=acc)
        d0 = fresh()
        o0 = ops.ce_step(x, t, C, d0, **kw)
        for weight in (ones, None):
            d = fresh()
            o = ops.ce_weighted_step(x, t, C, d, weight=weight, reduction=MEAN, **kw)
            assert torch.equal(o, o0) and torch.equal(d, d0), ("all ones" if weight is not None else "NULL", acc)
            assert torch.equal(ops.ce_weighted_fwd(x, t, C, weight, MEAN, IGN), o0)
        assert not torch.isnan(d0).any()
        for reduction in (MEAN, SUM):
            for weight in (w, None):
                da, db, dc = fresh(), fresh(), fresh()
                oa = ops.ce_weighted_fwd(x, t, C, weight, reduction, IGN)
                ops.ce_weighted_bwd(x, t, C, oa[1:2], da, weight=weight, reduction=reduction, **kw)
                ob = ops.ce_weighted_step(x, t, C, db, weight=weight, reduction=reduction, **kw)
                oc = ops.ce_weighted_step(x, t, C, dc, weight=weight, reduction=reduction, **kw)
                assert torch.equal(oa, ob) and torch.equal(da, db), (reduction, acc)
                assert torch.equal(ob, oc) and torch.equal(db, dc), (reduction, acc)
                assert not torch.isnan(ob).any() and not torch.isnan(db).any()
        ma, mb = ops.ce_map_fwd(x, t, C, w, IGN), ops.ce_map_fwd(x, t, C, w, IGN)
        dm = torch.randn(P, generator=g).to(DEV)
        da = ops.ce_map_bwd(x, t, C, dm, fresh(), weight=w, gmul=8.0, ignore_index=IGN, accumulate=acc)
        db = ops.ce_map_bwd(x, t, C, dm, fresh(), weight=w, gmul=8.0, ignore_index=IGN, accumulate=acc)
        assert torch.equal(ma, mb) and torch.equal(da, db)
    torch.cuda.synchronize()


@pytest.mark.parametrize("P,C", [(257, 4), (262145, 3)])
def test_weighted_mean_without_weight_is_nan(ops, P, C):
    """Every target ignored, or every weight zero, under the mean: 0 / 0 = NaN as in torch, and a denominator of exactly 0 (the
    gradients are unspecified there)."""
    g = torch.Generator().manual_seed(3 + P)
    x = torch.randn(P, C, generator=g)
    t = torch.randint(0, C, (P,), generator=g)
    zeros = torch.zeros(C)
    ref = F.cross_entropy(x.double(), t, weight=zeros.double(), ignore_index=IGN, reduction="mean")
    assert math.isnan(ref.item())
    xg = x.to(DEV)
    for tt, w in ((t, zeros), (torch.full_like(t, IGN), _weights(C))):
        for o in (ops.ce_weighted_fwd(xg, tt.to(DEV), C, w.to(DEV), MEAN, IGN),
                  ops.ce_weighted_step(xg, tt.to(DEV), C, _nan(P, C), weight=w.to(DEV), reduction=MEAN, ignore_index=IGN)):
            assert math.isnan(o[0].item()) and o[1].item() == 0.0
        o = ops.ce_weighted_fwd(xg, tt.to(DEV), C, w.to(DEV), SUM, IGN)
        assert o[0].item() == 0.0 and o[1].item() == 0.0


def test_weighted_ce_status_codes(ops):
    P, C = 64, 3
    x = torch.zeros(P, C, device=DEV)
    t = torch.zeros(P, dtype=torch.int64, device=DEV)
    w = torch.ones(8, device=DEV)
    out, dl, m = torch.zeros(2, device=DEV), torch.zeros(P, 9, device=DEV), torch.zeros(P, device=DEV)
    ws = ops._loss_ws(DEV)
    p, st = ops.ptr, ops.stream

    def fwd(**k):
        return ["dct_ce_weighted_fwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("red", 0),
                k.get("out", p(out)), p(ws), k.get("wsb", ws.numel()), st()]

    def bwd(**k):
        return ["dct_ce_weighted_bwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("red", 0),
                k.get("den", p(out[1:2])), None, 1.0, k.get("dl", p(dl)), 0, st()]

    def step(**k):
        return ["dct_ce_weighted_step", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("red", 0),
                k.get("out", p(out)), None, 1.0, k.get("dl", p(dl)), 0, p(ws), k.get("wsb", ws.numel()), st()]

    def mfwd(**k):
        return ["dct_ce_map_fwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("out", p(m)), st()]

    def mbwd(**k):
        return ["dct_ce_map_bwd", k.get("x", p(x)), k.get("t", p(t)), k.get("P", P), k.get("C", C), IGN, p(w), k.get("dm", p(m)), 1.0,
                k.get("dl", p(dl)), 0, st()]
    for f in (fwd, bwd, step, mfwd, mbwd):
        ops.call(*f())
        bad = [dict(x=None), dict(t=None), dict(P=0)]
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
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("kw,strided", [(dict(), False), (dict(size_average=False), False), (dict(reduce=False), False),
                                        (dict(), True), (dict(reduce=False, size_average=False), True)])
def test_module_against_torch(ops, C, kw, strided):
    """CrossEntropyLoss2d(weight, reduce, size_average) and its backward at [2, C, 16, 24] with an upstream gradient that is not 1
    ((3 loss).backward(); a random dmap for the map), once through a non-contiguous NCHW input; bounds as for the kernels."""
    from dct_amd.loss import CrossEntropyLoss2d
    B, H, W = 2, 16, 24
    g = torch.Generator().manual_seed(17 + C + len(kw))
    w = _weights(C)
    crit = CrossEntropyLoss2d(weight=w.tolist(), **kw)
    red = crit.reduction
    x = torch.randn(B, C, H, 2 * W if strided else W, generator=g) * 2
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.25] = IGN
    leaf = x.to(DEV).requires_grad_(True)
    inp = leaf[..., ::2] if strided else leaf
    assert inp.is_contiguous() != strided
    xs = x[..., ::2] if strided else x
    flat = xs.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    r = _Ref(flat, t.reshape(-1), w, C)
    got = crit(inp, t.to(DEV))
    if red == "none":
        assert got.shape == (B, H, W)
        dmap = torch.randn(B, H, W, generator=g)
        got.backward(dmap.to(DEV))
        lmap = F.cross_entropy(r.xd, r.t, weight=r.wd, ignore_index=IGN, reduction="none")
        _check(got.reshape(-1), lmap.detach(), r.wi * r.e + U * r.wl, "map")
        dref, bound = r.grad(lmap, dmap.double().reshape(-1), 5, grad_outputs=dmap.double().reshape(-1))
    else:
        reduction = MEAN if red == "mean" else SUM
        (3 * got).backward()
        loss, tol = r.value(reduction)
        assert got.dim() == 0 and abs(got.item() - loss.item()) <= tol, (got.item(), loss.item(), tol)
        dref, bound = r.grad(3 * loss, 3.0 / r.D if reduction == MEAN else 3.0, 6 if reduction == MEAN else 5)
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


def test_module_checks_weight_length_and_unit_weights_take_the_unweighted_kernels(ops):
    from dct_amd.loss import CrossEntropyLoss2d
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 16, 24, generator=g).to(DEV)
    t = torch.randint(0, 3, (2, 16, 24), generator=g).to(DEV)
    with pytest.raises(ValueError, match="4 class weights for logits of 3 classes"):
        CrossEntropyLoss2d(weight=[0.1, 1, 2.5, 0])(x, t)
    a, b, c = CrossEntropyLoss2d()(x, t), CrossEntropyLoss2d(weight=[1, 1, 1])(x, t), CrossEntropyLoss2d(weight=torch.ones(3))(x, t)
    assert torch.equal(a, b) and torch.equal(a, c)
    # the sum and the map of an unweighted criterion: the mean times the count, and a map that sums to it
    s, m = CrossEntropyLoss2d(size_average=False)(x, t), CrossEntropyLoss2d(reduce=False)(x, t)
    np.testing.assert_allclose(s.item(), a.item() * t.numel(), rtol=1e-5)
    np.testing.assert_allclose(m.double().sum().item(), s.item(), rtol=1e-5)
