"""Soft Dice and CE + Dice on the device (``dct_ce_dice_fwd`` / ``_bwd`` / ``_step``, include/dct.h) and ``DiceLoss`` /
``CrossEntropyDiceLoss2d`` on top of them, against tests/test_dice_loss_cpu.py's float64 reference (``DiceRef``) computed on the CPU from
exactly the fp32 logits and fp32 weights the kernels read.  The method is tests/test_weighted_ce_gpu.py's.

Tolerances (first order; U: fp32 unit roundoff; SUM_DEPTH: the levels of an fp32 reduction, here <= 3 grid trips of a thread + 6 shuffle
levels + 3 adds of the wave sums in the forward kernel, then the fold of the block rows: 2 rows per thread + 6 + 3 by a block, or up to 8
rows per lane + 6 by one wave (a group under per_image), 26 at the most <= SUM_DEPTH; a probability carries
ep_c = (C + 6 + |x_c - m|) U p_c, the per-pixel softmax bound of ``test_ce_at_scale``):
  * S = sum p_c: eS = sum ep_c + SUM_DEPTH U S;  I = sum_{t = c} p_c: eI = sum_{t = c} ep_c + SUM_DEPTH U I;  Y (a count; its partial sums
    are integers below 2^24): eY = SUM_DEPTH U Y;  sum w: SUM_DEPTH U sum w.
  * D = N / Den with N = 2 I + smooth (eN = 2 eI + U N + U smooth: one add, and smooth's conversion to fp32) and Den = S + Y + smooth
    (eDen = eS + eY + 2 U Den + U smooth: two adds and the conversion):
    |N'/Den' - N/Den| <= (eN + D eDen) / Den' with Den' >= Den - eDen, and the division rounds once:
    eD = (eN + D eDen) / (Den - eDen) + U D.  An empty denominator is exact (no term was added): D = 1 with eD = 0.
  * dice = 1 - (1 / (G K)) sum D: sum eD / (G K) + (G K + 2) U mean D + U |dice| (G K sequential adds, the rounded 1 / (G K), the product;
    the subtraction).
  * ce: test_weighted_ce_gpu's mean: (sum w_i e_i + (SUM_DEPTH + 1) U sum w_i l_i) / sum w + (SUM_DEPTH + 2) U |ce|.
  * total = cc ce + dc dice: |cc| e_ce + |dc| e_dice + 3 U (|cc ce| + |dc dice|) (a coefficient's conversion to fp32, its product, the sum).
  * gradient d = a + b per element:
      a = (g cc / sum w) w_t (p_c - y_c): test_weighted_ce_gpu's |g cc w_t / sum w| ((C + 6 + |x_c - m|) U p_c + k U |p_c - y_c|) with
        k = SUM_DEPTH + 7 (the fp32 sum of the weights, g = gscale gmul, cc's conversion and product, the division, w_t, p - y, the product);
      b = (g dc) p_c (q_c - dot), q_c = qb_c - y_c qa_c, qa = alpha / (G K), qb = beta / (G K), dot = sum_k p_k q_k:
        alpha = 2 / Den: e_alpha = alpha (eDen / (Den - eDen) + U);  beta = D / Den: e_beta = (eD + beta eDen) / (Den - eDen) + U beta;
        e_qa = (e_alpha + 2 U alpha) / (G K), e_qb likewise;  e_q = e_qb + y e_qa + U |q|;
        e_dot = sum_k (ep_k |q_k| + p_k e_q_k) + C U sum_k p_k |q_k|;  e_diff = e_q + e_dot + U |q - dot|;
        e_b = |g dc| (ep_c |q_c - dot| + p_c e_diff + 5 U p_c |q_c - dot|)   (the product p (q - dot), then g dc: three roundings and the product);
      e_d = e_a + e_b + U |d|, and U |old + d| more under accumulate.  Uncounted pixels: exactly 0 (exactly old).
Sentinels work through a *sentinel class* (the last class, always in the mask): its targets sit only at the seam pixels of both grids
(0, 255, 256, stride - 1, stride, 2 stride, PPI - 1 of every image), with logits of +5 and -2 in turn; everywhere else its logit is
about -20.  I and Y of that class are the seams alone, and the test asserts from the reference that dropping any one of them moves D of
that class by more than four times eD.  Per-pixel outputs are pre-filled with NaN.
Shapes: PPI 1, 255, 257 (partial blocks); one pixel past one trip of the forward grid (512 // B blocks of 256 pixels per image: 131,073
at B = 1, 65,537 at B = 2, 43,521 at B = 3) and of the backward grid (1024 // B blocks: 262,145, 131,073, 87,297)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_loss_kernels_scale_gpu import DEV, IGN, SUM_DEPTH, U, _check, _nan, _sm64  # noqa: E402
from test_dice_loss_cpu import DiceRef  # noqa: E402

FWD_BLOCKS, BWD_BLOCKS = 512, 1024        # csrc/loss.hip: kDiceFwdBlocks, kDiceBwdBlocks


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _grid_x(PPI, B, cap):
    return min((PPI + 255) // 256, max(1, cap // B))


def _seams(PPI, B):
    s = set()
    for cap in (FWD_BLOCKS, BWD_BLOCKS):
        st = _grid_x(PPI, B, cap) * 256
        s |= {0, 255, 256, st - 1, st, 2 * st, PPI - 1}
    return torch.tensor(sorted(i for i in s if 0 <= i < PPI))


def _weights(C):
    return torch.tensor([(0.1, 1.0, 0.0, 2.5)[c % 4] for c in range(C)], dtype=torch.float32)


def _inputs(B, PPI, C, stray, seed):
    """fp32 logits [B, PPI, C], targets [B, PPI] (a quarter ignored; ``stray``: a few are C and -1) and the seam pixels, which alone carry
    the sentinel class C - 1."""
    g = torch.Generator().manual_seed(seed)
    sc = C - 1
    x = torch.randn(B, PPI, C, generator=g) * 2
    x[..., sc] = -20 + 0.5 * torch.randn(B, PPI, generator=g)
    t = torch.randint(0, sc, (B, PPI), generator=g)
    t[torch.rand(B, PPI, generator=g) < 0.25] = IGN
    if stray:
        idx = (torch.arange(6) * PPI // 7 + 1) % PPI
        t[:, idx[:3]] = C
        t[:, idx[3:]] = -1
    sen = _seams(PPI, B)
    t[:, sen] = sc
    x[:, sen, :] = 0.0
    x[:, sen, sc] = torch.where(torch.arange(len(sen)) % 2 == 0, 5.0, -2.0)[None, :] + 0.25 * torch.arange(B)[:, None]
    return g, x, t, sen


class _Bounds:
    """The bounds of the module docstring for one reference ``r`` (DiceRef of the fp32 logits ``x``)."""

    def __init__(self, r, x):
        self.r = r
        B, PPI, C = x.shape
        fbx = _grid_x(PPI, B, FWD_BLOCKS)
        assert -(-PPI // (fbx * 256)) + 6 + 3 + max(-(-B * fbx // 256) + 6 + 3, -(-fbx // 64) + 6) <= SUM_DEPTH
        with torch.no_grad():
            p, spread = _sm64(x.reshape(-1, C))
            self.p, self.spread = p.reshape(B, PPI, C), spread.reshape(B, PPI, C)
            self.ep = (C + 6 + self.spread) * U * self.p
            k = r.keep[..., None].double()
            dims = (1,) if r.per_image else (0, 1)
            shape = (r.G, C)
            self.eS = (self.ep * k).sum(dims).reshape(shape) + SUM_DEPTH * U * r.S
            self.eI = (self.ep * r.y).sum(dims).reshape(shape) + SUM_DEPTH * U * r.I
            self.eY = SUM_DEPTH * U * r.Y
            self.eN = 2 * self.eI + U * r.num + U * r.smooth
            self.eDen = self.eS + self.eY + 2 * U * r.den + U * r.smooth
            zero, one = torch.zeros_like(r.den), torch.ones_like(r.den)
            self.den1 = torch.where(r.empty, one, r.den - self.eDen)            # Den - eDen (1 where the denominator is empty)
            assert (self.den1 > 0).all()
            self.eD = torch.where(r.empty, zero, (self.eN + r.D * self.eDen) / self.den1 + U * r.D)
            GK = r.G * r.K
            Dm = r.D[:, r.mask]
            self.e_dice = self.eD[:, r.mask].sum().item() / GK + (GK + 2) * U * Dm.sum().item() / GK + U * abs(r.dice.item())
            amax = x.double().abs().max(-1).values
            e = (C + 8) * U * (3 * amax + math.log(C) + r.l + 1) * r.keep
            N = (r.wi * r.l).sum().item()
            self.e_sumw = SUM_DEPTH * U * r.sumw.item()
            self.e_ce = ((r.wi * e).sum().item() + (SUM_DEPTH + 1) * U * N) / r.sumw.item() + (SUM_DEPTH + 2) * U * abs(r.ce.item()) \
                if r.sumw.item() > 0 else float("nan")
            self.e_total = 0.0
            if r.ce_coef != 0:
                self.e_total += abs(r.ce_coef) * self.e_ce + 3 * U * abs(r.ce_coef * r.ce.item())
            if r.dice_coef != 0:
                self.e_total += abs(r.dice_coef) * self.e_dice + 3 * U * abs(r.dice_coef * r.dice.item())

    def _px(self, v):
        return v[:, None, :] if self.r.per_image else v[None]

    def grad(self, gg, old=None):
        """(gg * dtotal/dx (+ old), its bound), both [B, PPI, C]"""
        r, C = self.r, self.r.C
        with torch.no_grad():
            d = r.closed_form(gg)
            k = r.keep[..., None]
            bound = torch.zeros_like(d)
            if r.ce_coef != 0:
                gw = (abs(gg * r.ce_coef) / r.sumw * r.wi)[..., None]
                bound = bound + gw * ((C + 6 + self.spread) * U * self.p + (SUM_DEPTH + 7) * U * (self.p - r.y).abs())
            if r.dice_coef != 0:
                q, alpha, beta = r.q()
                GK = r.G * r.K
                m = r.mask.double() / GK
                e_alpha = alpha * (self.eDen / self.den1 + U)
                e_beta = (self.eD + beta * self.eDen) / self.den1 + U * beta
                e_qa, e_qb = self._px(m * (e_alpha + 2 * U * alpha)), self._px(m * (e_beta + 2 * U * beta))
                e_q = e_qb + r.y * e_qa + U * q.abs()
                dot = (self.p * q).sum(-1, keepdim=True)
                e_dot = (self.ep * q.abs() + self.p * e_q).sum(-1, keepdim=True) + C * U * (self.p * q.abs()).sum(-1, keepdim=True)
                diff = q - dot
                e_diff = e_q + e_dot + U * diff.abs()
                bound = bound + abs(gg * r.dice_coef) * (self.ep * diff.abs() + self.p * e_diff + 5 * U * self.p * diff.abs())
            bound = bound + U * d.abs() + 1e-30
            bound = torch.where(k, bound, torch.zeros_like(bound))
            if old is not None:
                d = d + old.double()
                bound = bound + torch.where(k, U * d.abs(), torch.zeros_like(bound))
            return d, bound

    def sentinel_margin(self, sen):
        """min over the sentinels of |D without it - D| / eD for the sentinel class (must exceed 4)."""
        r, sc = self.r, self.r.C - 1
        worst = float("inf")
        with torch.no_grad():
            for b in range(r.B):
                g = b if r.per_image else 0
                pj = self.p[b, sen, sc]
                assert r.keep[b, sen].all() and (r.tc[b, sen] == sc).all()
                num, den = r.num[g, sc] - 2 * pj, r.den[g, sc] - pj - 1
                Dwo = torch.where(den.abs() < 1e-9, torch.ones_like(den), num / den.clamp(min=1e-300))
                worst = min(worst, ((Dwo - r.D[g, sc]).abs() / self.eD[g, sc]).min().item())
            assert int(r.Y[:, sc].sum().item()) == r.B * len(sen)          # the seams alone carry the class
        return worst


def _bits(a):
    return a.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hold(ops, g, x, t, w, classes, smooth, per_image, coefs, accumulate, sen=None, what=""):
    """fwd, bwd and step of one input against the reference, within the derived bounds; returns (reference, out4, dice_gc, gradient)."""
    B, PPI, C = x.shape
    cc, dc = coefs
    r = DiceRef(x, t, w, classes, smooth, per_image, cc, dc)
    bd = _Bounds(r, x)
    if sen is not None:
        margin = bd.sentinel_margin(sen)
        assert margin > 4, margin                                          # one lost sentinel is far outside the bound
    gscale, gmul = 0.61, 8.0
    gg = float(np.float32(gscale)) * gmul
    old = torch.randn(B, PPI, C, generator=g) if accumulate else None
    dref, dbound = bd.grad(gg, old)
    mask = None if classes is None else sum(1 << c for c in set(classes))
    xg, tg, wg = x.to(DEV), t.to(DEV), None if w is None else w.to(DEV)
    gs = torch.tensor([gscale], device=DEV)
    kw = dict(weight=wg, class_mask=mask, smooth=smooth, per_image=per_image, ce_coef=cc, dice_coef=dc, ignore_index=IGN)

    def fresh():
        return old.to(DEV) if accumulate else _nan(B, PPI, C)
    out4, dice_gc, sums = ops.ce_dice_fwd(xg, tg, C, **kw)
    d1 = ops.ce_dice_bwd(xg, tg, C, out4, sums, fresh(), gscale=gs, gmul=gmul, accumulate=accumulate, **kw)
    d2 = fresh()
    out4s, dice_gcs, sumss = ops.ce_dice_step(xg, tg, C, d2, gscale=gs, gmul=gmul, accumulate=accumulate, **kw)
    d3 = fresh()
    out4t, dice_gct, sumst = ops.ce_dice_step(xg, tg, C, d3, gscale=gs, gmul=gmul, accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    o = out4.cpu().double()
    print(f"{what} B={B} PPI={PPI} C={C} G={r.G} K={r.K} smooth={smooth} coefs={coefs}: total {r.total.item()!r} err {abs(o[0].item() - r.total.item()):.3e} "
          f"of {bd.e_total:.3e}; dice {r.dice.item()!r} err {abs(o[3].item() - r.dice.item()):.3e} of {bd.e_dice:.3e}; max D err / bound "
          f"{((dice_gc.cpu().double() - r.D).abs() / bd.eD.clamp(min=1e-300)).max().item():.3f}; max gradient err / bound "
          f"{((d1.cpu().double() - dref).abs() / dbound.clamp(min=1e-300)).max().item():.3f}" + (f"; sentinel margin {margin:.1f}" if sen is not None else ""))
    # the step is fwd followed by bwd, bit for bit, and two runs are bit-identical
    assert _same(out4, out4s) and _same(dice_gc, dice_gcs) and _same(sums, sumss) and _same(d1, d2), "step != fwd + bwd"
    assert _same(out4s, out4t) and _same(dice_gcs, dice_gct) and _same(sumss, sumst) and _same(d2, d3), "two runs differ"
    with torch.no_grad():
        s = sums.cpu().double()
        _check(s[..., 0], r.I, bd.eI, "I")
        _check(s[..., 1], r.S, bd.eS, "S")
        _check(s[..., 2], r.Y, bd.eY, "Y")
        _check(dice_gc, r.D, bd.eD, "D_gc")
        assert abs(o[2].item() - r.sumw.item()) <= bd.e_sumw, ("sum w", o[2].item(), r.sumw.item())
        if r.sumw.item() > 0:
            assert abs(o[1].item() - r.ce.item()) <= bd.e_ce, ("ce", o[1].item(), r.ce.item(), bd.e_ce)
        else:
            assert math.isnan(o[1].item())
        assert abs(o[3].item() - r.dice.item()) <= bd.e_dice, ("dice", o[3].item(), r.dice.item(), bd.e_dice)
        assert abs(o[0].item() - r.total.item()) <= bd.e_total, ("total", o[0].item(), r.total.item(), bd.e_total)
        if r.empty.any():
            assert (dice_gc.cpu()[r.empty] == 1.0).all()
    _check(d1, dref, dbound, "ce_dice_bwd")
    gone = ~r.keep
    if gone.any():
        want = old[gone] if accumulate else torch.zeros(int(gone.sum()), C)
        assert torch.equal(d1.cpu()[gone], want)                           # uncounted: exactly nothing (exactly the old value)
    return r, out4, dice_gc, d1


CASES = [  # B, PPI, C, per_image, accumulate, stray, smooth, classes ("fg": range(1, C); "s": the sentinel class alone, K = 1), (ce_coef, dice_coef)
    (1, 1, 2, False, False, False, 1e-5, None, (1.0, 1.0)),
    (2, 1, 4, True, True, False, 0.0, "fg", (0.5, 2.0)),         # (C = 4: the one pixel is a sentinel, and class 3 has a weight)
    (3, 255, 4, True, False, False, 1e-5, "fg", (1.0, 1.0)),
    (2, 255, 8, False, True, False, 1.0, None, (0.3, 0.7)),
    (3, 257, 3, False, True, True, 0.0, "fg", (1.0, 1.0)),
    (2, 257, 2, True, False, True, 1e-5, "s", (0.0, 1.0)),
    (1, 131073, 4, False, True, False, 1e-5, "fg", (1.0, 1.0)),
    (2, 65537, 3, True, False, True, 1.0, None, (1.0, 0.5)),
    (3, 43521, 8, False, False, False, 1e-5, "fg", (1.0, 1.0)),
    (1, 262145, 2, True, True, False, 0.0, None, (2.0, 1.0)),
    (2, 131073, 4, False, False, True, 1e-5, "s", (1.0, 1.0)),
    (3, 87297, 4, True, True, False, 1e-5, None, (0.0, 1.0)),
]


def _classes(C, which):
    return None if which is None else (list(range(1, C)) if which == "fg" else [C - 1])


@pytest.mark.parametrize("B,PPI,C,per_image,accumulate,stray,smooth,which,coefs", CASES)
def test_ce_dice_at_scale(ops, B, PPI, C, per_image, accumulate, stray, smooth, which, coefs):
    g, x, t, sen = _inputs(B, PPI, C, stray, seed=PPI + 7 * C + B)
    if stray and PPI > 6:
        assert int(((t != IGN) & ((t < 0) | (t >= C))).sum()) >= 3 * B
    _hold(ops, g, x, t, _weights(C), _classes(C, which), smooth, per_image, coefs, accumulate, sen, "at scale")


@pytest.mark.parametrize("B,PPI,C", [(3, 257, 4), (2, 65537, 3)])
def test_image_permutation_and_removed_terms(ops, B, PPI, C):
    """Under per_image a permutation of the images permutes the rows of dice_gc and sums, bit for bit.  dice_coef = 0: total is
    fl(ce_coef) ce exactly and the gradient does not depend on mask, smooth or per_image; ce_coef = 0: total is fl(dice_coef) dice exactly,
    the gradient does not depend on the weights, and the NaN ce of all-zero weights reaches neither."""
    g, x, t, _ = _inputs(B, PPI, C, True, seed=3 * PPI + C)
    xg, tg, wg = x.to(DEV), t.to(DEV), _weights(C).to(DEV)
    kw = dict(weight=wg, class_mask=(1 << C) - 2, smooth=1e-5, per_image=True, ce_coef=1.0, dice_coef=1.0, ignore_index=IGN)
    out4, dice_gc, sums = ops.ce_dice_fwd(xg, tg, C, **kw)
    perm = torch.tensor([(b + 1) % B for b in range(B)], device=DEV)
    out4p, dice_gcp, sumsp = ops.ce_dice_fwd(xg[perm].contiguous(), tg[perm].contiguous(), C, **kw)
    assert _same(dice_gcp, dice_gc[perm]) and _same(sumsp, sums[perm])
    assert not torch.isnan(dice_gc).any() and len({tuple(row) for row in dice_gc.cpu().tolist()}) == B     # (the rows differ)

    gs = torch.tensor([0.61], device=DEV)

    def step(**over):
        d = _nan(B, PPI, C)
        o, dg, _ = ops.ce_dice_step(xg, tg, C, d, gscale=gs, gmul=8.0, **{**kw, **over})
        return o, dg, d
    # dice_coef = 0
    oa, _, da = step(ce_coef=0.75, dice_coef=0.0)
    ob, dgb, db = step(ce_coef=0.75, dice_coef=0.0, class_mask=1 << (C - 1), smooth=1.0, per_image=False)
    assert _same(da, db) and not torch.isnan(da).any()
    assert oa[0].item() == (torch.tensor(0.75) * oa[1].cpu()).item() == ob[0].item()
    assert not torch.isnan(dgb).any() and not math.isnan(ob[3].item())                   # (dice is still reported)
    # ce_coef = 0
    zeros = torch.zeros(C, device=DEV)
    oc, _, dc = step(ce_coef=0.0, dice_coef=0.6)
    od, _, dd = step(ce_coef=0.0, dice_coef=0.6, weight=zeros)
    oe, _, de = step(ce_coef=0.0, dice_coef=0.6, weight=None)
    assert _same(dc, dd) and _same(dc, de) and not torch.isnan(dc).any()
    assert math.isnan(od[1].item()) and od[2].item() == 0.0 and not math.isnan(oc[1].item())
    want = (torch.tensor(0.6) * oc[3].cpu()).item()
    assert oc[0].item() == want and od[0].item() == want and oe[0].item() == want
    # with its coefficient, the NaN does reach total (the rule is torch's mean)
    of, _, _ = step(ce_coef=1.0, dice_coef=0.6, weight=zeros)
    assert math.isnan(of[0].item()) and of[3].item() == oc[3].item()
    torch.cuda.synchronize()


@pytest.mark.parametrize("smooth", [0.0, 1e-5])
@pytest.mark.parametrize("per_image", [False, True])
def test_degenerate_groups(ops, smooth, per_image):
    """A class absent from gt (class 1: D = smooth / (S + smooth)), an image with no counted pixel (image 1: under G = B its D is 1 in
    both cases -- by the empty-denominator rule under smooth = 0, as smooth / smooth otherwise -- and its gradient exactly 0) and K = 1."""
    B, PPI, C = 3, 300, 4
    g, x, t, _ = _inputs(B, PPI, C, False, seed=91)
    t[t == 1] = 2
    t[1] = IGN
    for classes in (None, [1]):
        r, out4, dice_gc, d = _hold(ops, g, x, t, _weights(C), classes, smooth, per_image, (1.0, 1.0), False, None, "degenerate")
        assert r.Y[:, 1].sum().item() == 0 and not r.keep[1].any()
        assert torch.equal(d.cpu()[1], torch.zeros(PPI, C))
        if per_image:
            assert (dice_gc.cpu()[1] == 1.0).all() and bool(r.empty[1].all()) == (smooth == 0.0)
        if smooth == 0.0:
            assert (dice_gc.cpu()[:, 1][r.S[:, 1] > 0] == 0.0).all()


def test_ce_dice_status_codes(ops):
    B, PPI, C = 2, 64, 3
    g, x, t, _ = _inputs(B, PPI, C, False, seed=2)
    xg, tg = x.to(DEV), t.to(DEV)
    w = torch.ones(8, device=DEV)
    out4, dgc, sums, dl = torch.zeros(4, device=DEV), torch.zeros(B, 8, device=DEV), torch.zeros(B, 8, 3, device=DEV), torch.zeros(B, PPI, 8, device=DEV)
    lib = ops._lib.load()
    need = lib.dct_ce_dice_workspace_bytes(B, C, 1)
    assert need > lib.dct_loss_workspace_bytes(0) and need == lib.dct_ce_dice_workspace_bytes(B, C, 0)
    assert lib.dct_ce_dice_workspace_bytes(B, 8, 1) > need
    ws = torch.empty(lib.dct_ce_dice_workspace_bytes(B, 8, 1), dtype=torch.uint8, device=DEV)
    p, st = ops.ptr, ops.stream

    def rule(k):
        return [k.get("B", B), k.get("PPI", PPI), k.get("C", C), IGN, p(w), k.get("mask", 0b110), k.get("smooth", 1e-5), k.get("per_image", 1), 1.0, 1.0]

    def fwd(**k):
        return ["dct_ce_dice_fwd", k.get("x", p(xg)), k.get("t", p(tg))] + rule(k) + [k.get("out", p(out4)), k.get("dgc", p(dgc)), k.get("sums", p(sums)),
                                                                                     k.get("ws", p(ws)), k.get("wsb", need), st()]

    def bwd(**k):
        return ["dct_ce_dice_bwd", k.get("x", p(xg)), k.get("t", p(tg))] + rule(k) + [k.get("out", p(out4)), k.get("sums", p(sums)), None, 1.0,
                                                                                     k.get("dl", p(dl)), 0, st()]

    def step(**k):
        return ["dct_ce_dice_step", k.get("x", p(xg)), k.get("t", p(tg))] + rule(k) + [k.get("out", p(out4)), k.get("dgc", p(dgc)), k.get("sums", p(sums)),
                                                                                      None, 1.0, k.get("dl", p(dl)), 0, k.get("ws", p(ws)), k.get("wsb", need), st()]
    for f in (fwd, bwd, step):
        ops.call(*f())
        bad = [dict(x=None), dict(t=None), dict(out=None), dict(sums=None), dict(PPI=0), dict(B=0), dict(smooth=-1e-5), dict(smooth=float("nan")),
               dict(smooth=float("inf")), dict(mask=0), dict(mask=0b1000), dict(per_image=2), dict(per_image=-1)]
        bad += [dict(dgc=None)] if f in (fwd, step) else []
        bad += [dict(dl=None)] if f in (bwd, step) else []
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
    _hold(ops, g, x, t, _weights(C), [1, 2], 1e-5, True, (1.0, 1.0), False, None, "after the refused calls")


# ---------------------------------------------------------------------------------------------------------------------- the modules
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("which,per_image", [("dice", True), ("dice", False), ("ce_dice", True), ("ce_dice", False)])
def test_modules_against_the_reference(ops, C, which, per_image):
    """DiceLoss(foreground, per image or not) and CrossEntropyDiceLoss2d(weight, ce_coef = 0.5, dice_coef = 2) through (3 loss).backward()
    at [2, C, 16, 24], from a non-contiguous NCHW input and int32 targets; ``last_dice`` is the [G, C] table of D_gc."""
    from dct_amd.loss import get_loss_fn
    B, H, W = 2, 16, 24
    g = torch.Generator().manual_seed(23 + C + per_image)
    w = _weights(C)
    fg = list(range(1, C))
    if which == "dice":
        crit, rule = get_loss_fn("dice", classes=range(1, C), per_image=per_image), (None, fg, 1e-5, per_image, 0.0, 1.0)
    else:
        crit = get_loss_fn("ce_dice", weight=w.tolist(), ce_coef=0.5, dice_coef=2.0, smooth=1.0, per_image=per_image)
        rule = (w, None, 1.0, per_image, 0.5, 2.0)
    x = torch.randn(B, C, H, 2 * W, generator=g) * 2
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.25] = IGN
    leaf = x.to(DEV).requires_grad_(True)
    inp = leaf[..., ::2]
    assert not inp.is_contiguous()
    flat = x[..., ::2].permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous()
    r = DiceRef(flat, t.reshape(B, -1), *rule)
    bd = _Bounds(r, flat)
    got = crit(inp, t.to(DEV).to(torch.int32))
    (3 * got).backward()
    torch.cuda.synchronize()
    assert got.dim() == 0 and abs(got.item() - r.total.item()) <= bd.e_total, (got.item(), r.total.item(), bd.e_total)
    assert crit.last_dice.shape == (r.G, C) and crit.last_dice.is_cuda and not crit.last_dice.requires_grad
    _check(crit.last_dice, r.D.detach(), bd.eD, "last_dice")
    dref, dbound = bd.grad(3.0)
    _check(leaf.grad[..., ::2].permute(0, 2, 3, 1).reshape(B, H * W, C), dref, dbound, f"{which} gradient")
    assert torch.equal(leaf.grad[..., 1::2], torch.zeros_like(leaf.grad[..., 1::2]))
    with pytest.raises(ValueError, match="outside"):
        get_loss_fn("dice", classes=[C])(inp, t.to(DEV))
    if which == "ce_dice":
        with pytest.raises(ValueError, match="class weights for logits"):
            get_loss_fn("ce_dice", weight=[0.5] * (C + 1))(inp, t.to(DEV))
        buf = crit.device_weight(DEV, C)
        assert buf is crit.device_weight(DEV) and torch.equal(buf.cpu(), w)
