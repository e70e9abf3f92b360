"""Tversky and focal Tversky on the device (``dct_ce_tversky_fwd`` / ``_bwd`` / ``_step``, include/dct.h) and ``TverskyLoss`` /
``FocalTverskyLoss`` / ``CrossEntropyTverskyLoss2d`` on top of them, against tests/tversky_ref.py's float64 reference computed on the CPU
from exactly the fp32 logits and fp32 weights the kernels read, within the bounds derived in that module's docstring (no tolerance is put
in by hand).  Method, input generator and sentinel class are tests/test_dice_loss_gpu.py's: the last class sits only at the seam pixels
of both grids, and the test asserts from the reference that dropping any one of them moves T of that class by more than four times eT.
Before comparing, every case asserts from the reference what keeps a bound from hiding a failure (``TverskyBounds.conditions``: u >= 0.1
for the classes of the mask under gamma != 1 -- at C = 2 class 0 is predicted almost perfectly, so those cases take the sentinel class
alone, and PPI = 1 runs with gamma = 1 only --, Den - eDen > 0).  Per-pixel outputs are pre-filled with NaN.
Shapes: PPI 1, 255, 257 (partial blocks); one pixel past one trip of the forward grid (512 // B blocks of 256 pixels per image: 131,073
at B = 1, 65,537 at B = 2, 43,521 at B = 3) and of the backward grid (1024 // B blocks: 262,145, 131,073, 87,297)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_loss_kernels_scale_gpu import DEV, IGN, SUM_DEPTH, U, _check, _nan  # noqa: E402
from test_dice_loss_cpu import DiceRef  # noqa: E402
from test_dice_loss_gpu import _Bounds as DiceBounds, _classes, _inputs, _same, _weights  # noqa: E402
import tversky_ref  # noqa: E402
from tversky_ref import TverskyBounds, TverskyRef  # noqa: E402

assert (U, SUM_DEPTH, IGN) == (tversky_ref.U, tversky_ref.SUM_DEPTH, tversky_ref.IGN)

P1, P2, P3, P4 = (0.3, 0.7, 1.0), (0.3, 0.7, 4.0 / 3.0), (1.0, 1.0, 2.0), (0.7, 0.3, 0.75)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _hold(ops, g, x, t, w, classes, smooth, abg, per_image, coefs, accumulate, sen=None, what=""):
    """fwd, bwd and step of one input against the reference, within the derived bounds; returns (reference, bounds, out4, tversky_gc,
    gradient)."""
    B, PPI, C = x.shape
    cc, tc = coefs
    r = TverskyRef(x, t, w, classes, smooth, *abg, per_image, cc, tc)
    bd = TverskyBounds(r, x)                                                # (asserts Den - eDen > 0 for every non-empty (g, c))
    bd.conditions()
    margin = move = None
    if sen is not None:
        margin, move = bd.sentinel_margin(sen)
        assert margin > 4, margin                                          # one lost sentinel is far outside the bound
    gscale, gmul = 0.61, 8.0
    gg = float(np.float32(gscale)) * gmul
    old = torch.randn(B, PPI, C, generator=g) if accumulate else None
    dref, dbound = bd.grad(gg, old)
    mask = None if classes is None else sum(1 << c for c in set(classes))
    xg, tg, wg = x.to(DEV), t.to(DEV), None if w is None else w.to(DEV)
    gs = torch.tensor([gscale], device=DEV)
    kw = dict(weight=wg, class_mask=mask, smooth=smooth, alpha=abg[0], beta=abg[1], gamma=abg[2], per_image=per_image, ce_coef=cc,
              tversky_coef=tc, ignore_index=IGN)

    def fresh():
        return old.to(DEV) if accumulate else _nan(B, PPI, C)
    out4, tgc, sums = ops.ce_tversky_fwd(xg, tg, C, **kw)
    d1 = ops.ce_tversky_bwd(xg, tg, C, out4, sums, fresh(), gscale=gs, gmul=gmul, accumulate=accumulate, **kw)
    d2 = fresh()
    out4s, tgcs, sumss = ops.ce_tversky_step(xg, tg, C, d2, gscale=gs, gmul=gmul, accumulate=accumulate, **kw)
    d3 = fresh()
    out4t, tgct, sumst = ops.ce_tversky_step(xg, tg, C, d3, gscale=gs, gmul=gmul, accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    o = out4.cpu().double()
    live = r.mask[None, :] & ~r.empty
    print(f"{what} B={B} PPI={PPI} C={C} G={r.G} K={r.K} smooth={smooth} abg={abg} coefs={coefs}: total {r.total.item()!r} err "
          f"{abs(o[0].item() - r.total.item()):.3e} of {bd.e_total:.3e}; tversky {r.tversky.item()!r} err {abs(o[3].item() - r.tversky.item()):.3e} of "
          f"{bd.e_tversky:.3e}; max T err / bound {((tgc.cpu().double() - r.T.detach()).abs() / bd.eT.clamp(min=1e-300)).max().item():.3f}; max gradient "
          f"err / bound {((d1.cpu().double() - dref).abs() / dbound.clamp(min=1e-300)).max().item():.3f}; min masked u "
          f"{r.u.detach()[live].min().item() if live.any() else float('nan'):.3e}" + (f"; sentinel margin {margin:.1f}, move {move:.2e}" if sen is not None else ""))
    # the step is fwd followed by bwd, bit for bit, and two runs are bit-identical
    assert _same(out4, out4s) and _same(tgc, tgcs) and _same(sums, sumss) and _same(d1, d2), "step != fwd + bwd"
    assert _same(out4s, out4t) and _same(tgcs, tgct) and _same(sumss, sumst) and _same(d2, d3), "two runs differ"
    with torch.no_grad():
        s = sums.cpu().double()
        _check(s[..., 0], r.I.detach(), bd.eI, "I")
        _check(s[..., 1], r.S.detach(), bd.eS, "S")
        _check(s[..., 2], r.Y.detach(), bd.eY, "Y")
        _check(tgc, r.T.detach(), bd.eT, "T_gc")
        assert abs(o[2].item() - r.sumw.item()) <= bd.e_sumw, ("sum w", o[2].item(), r.sumw.item())
        if r.sumw.item() > 0:
            assert abs(o[1].item() - r.ce.item()) <= bd.e_ce, ("ce", o[1].item(), r.ce.item(), bd.e_ce)
        else:
            assert math.isnan(o[1].item())
        assert abs(o[3].item() - r.tversky.item()) <= bd.e_tversky, ("tversky", o[3].item(), r.tversky.item(), bd.e_tversky)
        assert abs(o[0].item() - r.total.item()) <= bd.e_total, ("total", o[0].item(), r.total.item(), bd.e_total)
        if r.empty.any():
            assert (tgc.cpu()[r.empty] == 1.0).all()
    _check(d1, dref, dbound, "ce_tversky_bwd")
    gone = ~r.keep
    if gone.any():
        want = old[gone] if accumulate else torch.zeros(int(gone.sum()), C)
        assert torch.equal(d1.cpu()[gone], want)                           # uncounted: exactly nothing (exactly the old value)
    return r, bd, out4, tgc, d1


CASES = [  # B, PPI, C, per_image, accumulate, stray, smooth, classes ("fg": range(1, C); "s": the sentinel class alone), (ce_coef, tversky_coef),
    #        class weights (with the CE term) or None, (alpha, beta, gamma)
    (1, 1, 2, False, False, False, 1e-5, None, (1.0, 1.0), True, P1),
    (2, 1, 4, True, True, False, 0.0, "fg", (0.5, 2.0), True, P1),          # (C = 4: the one pixel is a sentinel, and class 3 has a weight)
    (3, 255, 4, True, False, False, 1e-5, "fg", (1.0, 1.0), True, P2),
    (2, 255, 8, False, True, False, 1.0, None, (0.0, 1.0), False, P3),
    (3, 257, 3, False, True, True, 0.0, "fg", (1.0, 1.0), True, P4),
    (2, 257, 2, True, False, True, 1e-5, "s", (0.0, 1.0), False, P2),
    (1, 131073, 4, False, True, False, 1e-5, "fg", (0.0, 1.0), False, P1),
    (2, 65537, 3, True, False, True, 1.0, None, (1.0, 0.5), True, P3),
    (3, 43521, 8, False, False, False, 1e-5, "fg", (0.0, 1.0), False, P4),
    (1, 262145, 2, True, True, False, 0.0, "s", (2.0, 1.0), True, P1),      # (class 0's u is within 4 eu of 0 at this size: the sentinel class alone)
    (2, 131073, 4, False, False, True, 1e-5, "s", (1.0, 1.0), True, P2),
    (3, 87297, 4, True, False, False, 1e-5, None, (0.0, 1.0), False, P3),
    (2, 257, 4, True, True, True, 1e-5, "fg", (1.0, 1.0), True, P3),
    (3, 255, 3, True, False, False, 1e-5, None, (0.3, 0.7), True, P4),
    (1, 257, 8, False, True, True, 0.0, "fg", (0.0, 1.0), False, P4),
    (2, 65537, 4, False, True, False, 1e-5, "fg", (1.0, 1.0), True, P2),
    (1, 255, 2, False, True, True, 1e-5, "s", (0.0, 1.0), False, P2),
    (3, 257, 4, False, False, True, 1e-5, None, (0.0, 1.0), False, P1),
]


def test_the_cases_cover_what_they_must():
    """Every parameter set runs with and without the CE term and class weights, with accumulate on and off and with stray targets; every
    shape, C and G is there; gamma != 1 never meets PPI = 1, and at C = 2 takes the sentinel class alone."""
    for abg in (P1, P2, P3, P4):
        mine = [c for c in CASES if c[10] == abg]
        assert {c[9] for c in mine} == {True, False} and {c[4] for c in mine} == {True, False} and any(c[5] for c in mine)
        assert all((c[8][0] != 0.0) == c[9] for c in mine)
    assert {(c[0], c[1]) for c in CASES} >= {(1, 1), (2, 1), (3, 255), (2, 255), (3, 257), (2, 257), (1, 131073), (2, 65537), (3, 43521),
                                             (3, 87297), (1, 262145)}
    assert {c[2] for c in CASES} == {2, 3, 4, 8} and {c[3] for c in CASES} == {True, False}
    for c in CASES:
        if c[10][2] != 1.0:
            assert c[1] > 1 and (c[2] > 2 or c[7] == "s")


@pytest.mark.parametrize("B,PPI,C,per_image,accumulate,stray,smooth,which,coefs,weighted,abg", CASES)
def test_ce_tversky_at_scale(ops, B, PPI, C, per_image, accumulate, stray, smooth, which, coefs, weighted, abg):
    g, x, t, sen = _inputs(B, PPI, C, stray, seed=PPI + 7 * C + B)
    if stray and PPI > 6:
        assert int(((t != IGN) & ((t < 0) | (t >= C))).sum()) >= 3 * B
    _hold(ops, g, x, t, _weights(C) if weighted else None, _classes(C, which), smooth, abg, per_image, coefs, accumulate, sen, "at scale")


@pytest.mark.parametrize("B,PPI,C,abg", [(3, 257, 4, P2), (2, 65537, 3, P1)])
def test_image_permutation_and_removed_terms(ops, B, PPI, C, abg):
    """Under per_image a permutation of the images permutes the rows of tversky_gc and sums, bit for bit.  tversky_coef = 0: total is
    fl(ce_coef) ce exactly and the gradient does not depend on alpha, beta, gamma, mask, smooth or per_image; ce_coef = 0: total is
    fl(tversky_coef) tversky exactly, the gradient does not depend on the weights, and the NaN ce of all-zero weights reaches neither."""
    g, x, t, _ = _inputs(B, PPI, C, True, seed=3 * PPI + C)
    xg, tg, wg = x.to(DEV), t.to(DEV), _weights(C).to(DEV)
    kw = dict(weight=wg, class_mask=(1 << C) - 2, smooth=1e-5, alpha=abg[0], beta=abg[1], gamma=abg[2], per_image=True, ce_coef=1.0,
              tversky_coef=1.0, ignore_index=IGN)
    out4, tgc, sums = ops.ce_tversky_fwd(xg, tg, C, **kw)
    perm = torch.tensor([(b + 1) % B for b in range(B)], device=DEV)
    out4p, tgcp, sumsp = ops.ce_tversky_fwd(xg[perm].contiguous(), tg[perm].contiguous(), C, **kw)
    assert _same(tgcp, tgc[perm]) and _same(sumsp, sums[perm])
    assert not torch.isnan(tgc).any() and len({tuple(row) for row in tgc.cpu().tolist()}) == B     # (the rows differ)

    gs = torch.tensor([0.61], device=DEV)

    def step(**over):
        d = _nan(B, PPI, C)
        o, tg_, _ = ops.ce_tversky_step(xg, tg, C, d, gscale=gs, gmul=8.0, **{**kw, **over})
        return o, tg_, d
    # tversky_coef = 0
    oa, _, da = step(ce_coef=0.75, tversky_coef=0.0)
    ob, tgb, db = step(ce_coef=0.75, tversky_coef=0.0, class_mask=1 << (C - 1), smooth=1.0, per_image=False, alpha=1.0, beta=0.25, gamma=2.0)
    assert _same(da, db) and not torch.isnan(da).any()
    assert oa[0].item() == (torch.tensor(0.75) * oa[1].cpu()).item() == ob[0].item()
    assert not torch.isnan(tgb).any() and not math.isnan(ob[3].item())                   # (tversky is still reported)
    # ce_coef = 0
    zeros = torch.zeros(C, device=DEV)
    oc, _, dc = step(ce_coef=0.0, tversky_coef=0.6)
    od, _, dd = step(ce_coef=0.0, tversky_coef=0.6, weight=zeros)
    oe, _, de = step(ce_coef=0.0, tversky_coef=0.6, weight=None)
    assert _same(dc, dd) and _same(dc, de) and not torch.isnan(dc).any()
    assert math.isnan(od[1].item()) and od[2].item() == 0.0 and not math.isnan(oc[1].item())
    want = (torch.tensor(0.6) * oc[3].cpu()).item()
    assert oc[0].item() == want and od[0].item() == want and oe[0].item() == want
    # with its coefficient, the NaN does reach total (the rule is torch's mean)
    of, _, _ = step(ce_coef=1.0, tversky_coef=0.6, weight=zeros)
    assert math.isnan(of[0].item()) and of[3].item() == oc[3].item()
    torch.cuda.synchronize()


def _degenerate(seed=91):
    B, PPI, C = 3, 300, 4
    g, x, t, _ = _inputs(B, PPI, C, False, seed=seed)
    return g, x, t


@pytest.mark.parametrize("gamma", [1.0, 4.0 / 3.0])
def test_an_ignored_image_is_an_empty_denominator(ops, gamma):
    """smooth = 0 under per_image with image 1 fully ignored: T of that image is exactly 1 for every class, it adds exactly 0 to the value
    (nothing of that image reaches any output: other logits there give the same bits) and its gradient is exactly 0."""
    g, x, t = _degenerate()
    t[1] = IGN
    B, PPI, C = x.shape
    for classes in (None, [1, 3]):
        r, bd, out4, tgc, d = _hold(ops, g, x, t, _weights(C), classes, 0.0, (0.3, 0.7, gamma), True, (1.0, 1.0), False, None, "ignored image")
        assert r.empty[1].all() and not r.empty[0].any() and not r.empty[2].any() and (r.term.detach()[1] == 0).all()
        assert (tgc.cpu()[1] == 1.0).all() and torch.equal(d.cpu()[1], torch.zeros(PPI, C))
    x2 = x.clone()
    x2[1] = torch.randn(PPI, C, generator=g) * 3
    kw = dict(weight=None, class_mask=None, smooth=0.0, alpha=0.3, beta=0.7, gamma=gamma, per_image=True, ce_coef=1.0, tversky_coef=1.0, ignore_index=IGN)
    da, db = _nan(B, PPI, C), _nan(B, PPI, C)
    oa, ta, _ = ops.ce_tversky_step(x.to(DEV), t.to(DEV), C, da, **kw)
    ob, tb, _ = ops.ce_tversky_step(x2.to(DEV), t.to(DEV), C, db, **kw)
    assert _same(oa, ob) and _same(ta, tb) and _same(da, db) and not torch.isnan(da).any()


@pytest.mark.parametrize("gamma", [1.0, 4.0 / 3.0])
@pytest.mark.parametrize("how", ["absent", "perfect"])
def test_zero_terms_are_exact_zeros(ops, gamma, how):
    """alpha = 0, beta = 1 and a class of the mask that gives no term: ``absent`` -- smooth = 0 and class 1 absent from the targets, so
    Den = beta Y = 0 although S > 0 (T = 1 by the empty-denominator rule); ``perfect`` -- every target pixel of class 1 predicted with
    probability exactly 1 (its logit 200 above the rest: exactly 1 in fp32 and in float64), so I = Y, N = Den and u = 0 with a non-zero
    denominator.  Either way class 1 adds exactly 0 to the value and to the gradient: with the mask {1, 2} the value and the gradient
    are exactly half of those with the mask {2} (1 / (G K) is 1/2 against 1, a power of two, and nothing else differs)."""
    g, x, t = _degenerate(seed=92)
    B, PPI, C = x.shape
    if how == "absent":
        t[t == 1] = 2
        smooth = 0.0
    else:
        x[t == 1] = torch.tensor([0.0, 200.0, 0.0, 0.0])
        smooth = 1e-5
    r, bd, out4, tgc, d = _hold(ops, g, x, t, None, [1, 2], smooth, (0.0, 1.0, gamma), False, (0.0, 1.0), False, None, how)
    assert bool(r.empty[0, 1]) == (how == "absent") and r.u[0, 1].item() == 0.0 and r.term[0, 1].item() == 0.0 and r.u[0, 2].item() >= 0.1
    if how == "perfect":
        assert r.I[0, 1].item() == r.Y[0, 1].item() > 0
    assert tgc[0, 1].item() == 1.0
    r1, _, out41, _, d1 = _hold(ops, g, x, t, None, [2], smooth, (0.0, 1.0, gamma), False, (0.0, 1.0), False, None, how + " (class 2 alone)")
    assert out4[3].item() * 2 == out41[3].item() and out4[0].item() * 2 == out41[0].item()
    assert torch.equal(d.cpu() * 2, d1.cpu()) and d.abs().max().item() > 1e-6


@pytest.mark.parametrize("B,PPI,C,per_image,s", [(3, 257, 4, True, 1e-5), (2, 65537, 3, False, 1.0), (2, 255, 2, True, 0.0)])
def test_half_half_agrees_with_dice_at_twice_the_smooth(ops, B, PPI, C, per_image, s):
    """alpha = beta = 0.5, gamma = 1, smooth = s against dct_ce_dice_fwd at smooth = 2 s, device against device, within the sum of the two
    derived bounds (each side is within its own bound of the same float64 number)."""
    g, x, t, _ = _inputs(B, PPI, C, True, seed=5 * PPI + C)
    w = _weights(C)
    r = TverskyRef(x, t, w, None, s, 0.5, 0.5, 1.0, per_image, 0.5, 2.0)
    bt = TverskyBounds(r, x)
    rd = DiceRef(x, t, w, None, 2 * s, per_image, 0.5, 2.0)
    bdc = DiceBounds(rd, x)
    assert (r.T.detach() - rd.D.detach()).abs().max().item() <= 1e-12
    xg, tg, wg = x.to(DEV), t.to(DEV), w.to(DEV)
    o, tgc, sums = ops.ce_tversky_fwd(xg, tg, C, weight=wg, smooth=s, alpha=0.5, beta=0.5, gamma=1.0, per_image=per_image, ce_coef=0.5, tversky_coef=2.0)
    od, dgc, dsums = ops.ce_dice_fwd(xg, tg, C, weight=wg, smooth=2 * s, per_image=per_image, ce_coef=0.5, dice_coef=2.0)
    torch.cuda.synchronize()
    assert _same(sums, dsums) and _same(o[1:3], od[1:3])                    # (the same forward kernel and fold)
    _check(tgc, dgc.cpu().double(), bt.eT + bdc.eD, "T against D")
    assert abs(o[3].item() - od[3].item()) <= bt.e_tversky + bdc.e_dice, (o[3].item(), od[3].item())
    assert abs(o[0].item() - od[0].item()) <= bt.e_total + bdc.e_total, (o[0].item(), od[0].item())
    print(f"B={B} PPI={PPI} C={C} s={s}: max |T - D| {(tgc - dgc).abs().max().item():.3e}, |tversky - dice| {abs(o[3].item() - od[3].item()):.3e} "
          f"of {bt.e_tversky + bdc.e_dice:.3e}")


def test_ce_tversky_status_codes(ops):
    B, PPI, C = 2, 64, 3
    g, x, t, _ = _inputs(B, PPI, C, False, seed=2)
    xg, tg = x.to(DEV), t.to(DEV)
    w = torch.ones(8, device=DEV)
    out4, tgc, sums, dl = torch.zeros(4, device=DEV), torch.zeros(B, 8, device=DEV), torch.zeros(B, 8, 3, device=DEV), torch.zeros(B, PPI, 8, device=DEV)
    lib = ops._lib.load()
    need = lib.dct_ce_tversky_workspace_bytes(B, C, 1)
    assert need == lib.dct_ce_dice_workspace_bytes(B, C, 1) == lib.dct_ce_tversky_workspace_bytes(B, C, 0)
    assert lib.dct_ce_tversky_workspace_bytes(B, 8, 1) > need
    ws = torch.empty(lib.dct_ce_tversky_workspace_bytes(B, 8, 1), dtype=torch.uint8, device=DEV)
    p, st = ops.ptr, ops.stream
    nan, inf = float("nan"), float("inf")

    def rule(k):
        return [k.get("B", B), k.get("PPI", PPI), k.get("C", C), IGN, p(w), k.get("mask", 0b110), k.get("smooth", 1e-5), k.get("alpha", 0.3),
                k.get("beta", 0.7), k.get("gamma", 4.0 / 3.0), k.get("per_image", 1), 1.0, 1.0]

    def fwd(**k):
        return ["dct_ce_tversky_fwd", k.get("x", p(xg)), k.get("t", p(tg))] + rule(k) + [k.get("out", p(out4)), k.get("tgc", p(tgc)), k.get("sums", p(sums)),
                                                                                        k.get("ws", p(ws)), k.get("wsb", need), st()]

    def bwd(**k):
        return ["dct_ce_tversky_bwd", k.get("x", p(xg)), k.get("t", p(tg))] + rule(k) + [k.get("out", p(out4)), k.get("sums", p(sums)), None, 1.0,
                                                                                        k.get("dl", p(dl)), 0, st()]

    def step(**k):
        return ["dct_ce_tversky_step", k.get("x", p(xg)), k.get("t", p(tg))] + rule(k) + [k.get("out", p(out4)), k.get("tgc", p(tgc)), k.get("sums", p(sums)),
                                                                                         None, 1.0, k.get("dl", p(dl)), 0, k.get("ws", p(ws)), k.get("wsb", need), st()]
    for f in (fwd, bwd, step):
        ops.call(*f())
        ops.call(*f(alpha=0.0, beta=1.0))
        ops.call(*f(alpha=1.0, beta=0.0, gamma=1.0))
        # everything Dice refuses
        bad = [dict(x=None), dict(t=None), dict(out=None), dict(sums=None), dict(PPI=0), dict(B=0), dict(smooth=-1e-5), dict(smooth=nan),
               dict(smooth=inf), dict(mask=0), dict(mask=0b1000), dict(per_image=2), dict(per_image=-1)]
        bad += [dict(tgc=None)] if f in (fwd, step) else []
        bad += [dict(dl=None)] if f in (bwd, step) else []
        # and the Tversky parameters
        bad += [dict(alpha=-0.1), dict(alpha=nan), dict(alpha=inf), dict(beta=-0.1), dict(beta=nan), dict(beta=inf), dict(alpha=0.0, beta=0.0),
                dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=nan), dict(gamma=inf)]
        for b in bad:
            with pytest.raises(RuntimeError, match=r"status -1"):
                ops.call(*f(**b))
        for b in (dict(C=1), dict(C=9)):
            with pytest.raises(RuntimeError, match=r"status -2"):
                ops.call(*f(**b))
        if f in (fwd, step):
            for b in (dict(wsb=need - 4), dict(ws=None)):
                with pytest.raises(RuntimeError, match=r"status -4"):
                    ops.call(*f(**b))
    torch.cuda.synchronize()
    # after the refused calls a good call still gives the right answer
    _hold(ops, g, x, t, _weights(C), [1, 2], 1e-5, P1, True, (1.0, 1.0), False, None, "after the refused calls")


# ---------------------------------------------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("which,per_image", [("tversky", True), ("focal_tversky", False), ("ce_tversky", True), ("ce_tversky", False)])
def test_modules_against_the_reference(ops, C, which, per_image):
    """TverskyLoss(foreground, per image), FocalTverskyLoss (the paper's defaults; at C = 2 the foreground class alone, whose u is large)
    and CrossEntropyTverskyLoss2d(weight, ce_coef = 0.5, tversky_coef = 2, (0.7, 0.3, 0.75)) through (3 loss).backward() at [2, C, 16, 24],
    from a non-contiguous NCHW input and int32 targets; ``last_tversky`` is the [G, C] table of T_gc."""
    from dct_amd.loss import get_loss_fn
    B, H, W = 2, 16, 24
    g = torch.Generator().manual_seed(23 + C + per_image)
    w = _weights(C)
    fg = list(range(1, C))
    if which == "tversky":
        crit, rule = get_loss_fn("tversky", classes=range(1, C), per_image=per_image), (None, fg, 1e-5, 0.3, 0.7, 1.0, per_image, 0.0, 1.0)
    elif which == "focal_tversky":
        crit, rule = get_loss_fn("focal_tversky", classes=fg, per_image=per_image), (None, fg, 1e-5, 0.3, 0.7, 4.0 / 3.0, per_image, 0.0, 1.0)
    else:
        crit = get_loss_fn("ce_tversky", weight=w.tolist(), ce_coef=0.5, tversky_coef=2.0, alpha=0.7, beta=0.3, gamma=0.75, smooth=1.0,
                           per_image=per_image)
        rule = (w, None, 1.0, 0.7, 0.3, 0.75, per_image, 0.5, 2.0)
    x = torch.randn(B, C, H, 2 * W, generator=g) * 2
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.25] = IGN
    leaf = x.to(DEV).requires_grad_(True)
    inp = leaf[..., ::2]
    assert not inp.is_contiguous()
    flat = x[..., ::2].permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()
    r = TverskyRef(flat, t.reshape(B, -1), *rule)
    bd = TverskyBounds(r, flat)
    bd.conditions()
    got = crit(inp, t.to(DEV).to(torch.int32))
    (3 * got).backward()
    torch.cuda.synchronize()
    assert got.dim() == 0 and abs(got.item() - r.total.item()) <= bd.e_total, (got.item(), r.total.item(), bd.e_total)
    assert crit.last_tversky.shape == (r.G, C) and crit.last_tversky.is_cuda and not crit.last_tversky.requires_grad
    _check(crit.last_tversky, r.T.detach(), bd.eT, "last_tversky")
    dref, dbound = bd.grad(3.0)
    _check(leaf.grad[..., ::2].permute(0, 2, 3, 1).reshape(B, H * W, C), dref, dbound, f"{which} gradient")
    assert torch.equal(leaf.grad[..., 1::2], torch.zeros_like(leaf.grad[..., 1::2]))
    with pytest.raises(ValueError, match="outside"):
        get_loss_fn("tversky", classes=[C])(inp, t.to(DEV))
    if which == "ce_tversky":
        with pytest.raises(ValueError, match="class weights for logits"):
            get_loss_fn("ce_tversky", weight=[0.5] * (C + 1))(inp, t.to(DEV))
        buf = crit.device_weight(DEV, C)
        assert buf is crit.device_weight(DEV) and torch.equal(buf.cpu(), w)
