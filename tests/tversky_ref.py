"""The Tversky / focal Tversky rule of include/dct.h (``dct_ce_tversky_*``) in float64, for tests/test_tversky_cpu.py and
tests/test_tversky_gpu.py: ``TverskyRef`` (shaped like tests/test_dice_loss_cpu.py's ``DiceRef``: the sums, ``Den``, ``T``, ``u``, the value,
``closed_form(g)`` and ``autograd(g)``) and ``TverskyBounds``, the first-order error bounds of an fp32 evaluation of that rule.

The reference takes alpha, beta, gamma and smooth as the fp32 numbers the entry points receive, and c0 = fl(1 - alpha - beta), e = fl(1 / gamma)
(each formed in double and rounded to fp32 once, as the host does): the parameters then carry no error of their own and every epsilon
below is the arithmetic's.  The exponent of the gradient's power is e - 1 exactly (the derivative of u^e); the kernels' fp32 subtraction
e - 1 is part of the arithmetic.

Bounds (the derivation of tests/test_dice_loss_gpu.py's docstring, continued; U: fp32 unit roundoff; SUM_DEPTH: the levels of an fp32
reduction, the forward kernel and the fold are Dice's, so the count there holds; T6 = 6 U: the three ulp a device transcendental is allowed
(tests/focal_ref.py); a probability carries ep_c = (C + 6 + |x_c - m|) U p_c):
  * S = sum p_c: eS = sum ep_c + SUM_DEPTH U S;  I = sum_{t = c} p_c: eI = sum_{t = c} ep_c + SUM_DEPTH U I;  Y (a count; partial sums are
    integers below 2^24): eY = SUM_DEPTH U Y;  sum w: SUM_DEPTH U sum w.
  * N = I + smooth: eN = eI + U N (one add).
  * Den = ((c0 I + alpha S) + beta Y) + smooth, three products and three adds, one rounding each (Dice's has no product and two adds); with
    M = |c0| I + alpha S + beta Y + smooth, which bounds every intermediate sum (c0 may be negative):
    eDen = |c0| eI + alpha eS + beta eY + U (|c0| I + alpha S + beta Y) + 3 U M.
  * T = N / Den: |N'/Den' - N/Den| <= (eN + T eDen) / Den' with Den' >= Den - eDen (asserted > 0), and the division rounds once:
    eT = (eN + T eDen) / (Den - eDen) + U T.  An empty denominator is exact (no term was added): T = 1 with eT = 0.
  * u = max(1 - T, 0): eu = eT + U u (the subtraction; the clamp is 1-Lipschitz).
  * term: gamma == 1: u itself, e_term = eu.  Otherwise term = exp2(e log2 u) with the relative error of focal_ref.py's m = q^gamma:
    eps = e eps_u + 7 U e |ln u| + T6 with eps_u = eu / u; e_term = term eps.  (eps_u is only small while u is not: the tests assert
    u >= 0.1 for every class of the mask under gamma != 1, and u > 4 eu under gamma == 1 so that fp32 and float64 agree on u > 0.)
  * tversky = (sum term) (1 / (G K)): sum e_term / (G K) + (G K + 2) U mean term (G K sequential adds, the rounded 1 / (G K), the product).
  * ce, total: tests/test_dice_loss_gpu.py's, with tversky in dice's place.
  * f = ((m / (G K)) e) u^(e - 1): the same power bound with |e - 1| in place of e, U |e - 1| |ln u| more for the fp32 subtraction e - 1
    (an exponent off by U |e - 1| moves the power by that times |ln u|), U for the rounded 1 / (G K) and two products:
    eps_f = |e - 1| eps_u + 8 U |e - 1| |ln u| + T6 + 3 U;  gamma == 1: f = m / (G K), eps_f = U.  ef = f eps_f.
  * qa = (f A) / Den with A = 1 - c0 T: eA = |c0| eT + U |c0| T + U |A| (the product, the subtraction); the numerator X = f A carries
    eX = ef |A| + f eA + U |X|, and by the quotient rule used for Dice's alpha and beta  e_qa = (eX + |qa| eDen) / (Den - eDen) + U |qa|.
  * qb = ((f alpha) T) / Den: X = f alpha T, eX = ef alpha T + f alpha eT + 2 U X;  e_qb = (eX + qb eDen) / (Den - eDen) + U qb.
    A class outside the mask, an empty denominator and u == 0 give qa = qb = 0 exactly.
  * gradient d = a + b per element: a is tests/test_dice_loss_gpu.py's cross-entropy part; b = (g tc) p_c (q_c - dot), q_c = qb_c - y_c qa_c,
    dot = sum_k p_k q_k:  e_q = e_qb + y e_qa + U |q|;  e_dot = sum_k (ep_k |q_k| + p_k e_q_k) + C U sum_k p_k |q_k|;
    e_diff = e_q + e_dot + U |q - dot|;  e_b = |g tc| (ep_c |q_c - dot| + p_c e_diff + 5 U p_c |q_c - dot|);
    e_d = e_a + e_b + U |d|, and U |old + d| more under accumulate.  Uncounted pixels: exactly 0 (exactly old)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
T6 = 6 * U
SUM_DEPTH = 32          # tests/test_loss_kernels_scale_gpu.py: the levels of the kernels' reduction
IGN = 255
FWD_BLOCKS, BWD_BLOCKS = 512, 1024        # csrc/loss.hip: kDiceFwdBlocks, kDiceBwdBlocks (the Tversky entry points launch Dice's grids)


def f32(v):
    """``v`` rounded to fp32, as a Python float."""
    return float(np.float32(v))


class TverskyRef:
    """The rule of include/dct.h in float64.  ``x``: logits [B, PPI, C] (any float dtype; taken to float64), ``t``: int64 [B, PPI],
    ``weight``: C values or None, ``classes``: the class indices of the mean or None (all).  Fields: ``total``, ``ce``, ``sumw``,
    ``tversky`` (0-d tensors; ``total`` carries the graph to ``xd``), ``T``, ``u``, ``term``, ``Den``, ``N``, ``I``, ``S``, ``Y`` ([G, C]),
    ``empty``, ``some`` ([G, C] bool: Den == 0; u > 0), ``keep`` [B, PPI], ``p``, ``y``."""

    def __init__(self, x, t, weight=None, classes=None, smooth=1e-5, alpha=0.3, beta=0.7, gamma=1.0, per_image=False, ce_coef=1.0,
                 tversky_coef=1.0, ignore_index=IGN):
        B, PPI, C = x.shape
        self.B, self.PPI, self.C = B, PPI, C
        self.G = B if per_image else 1
        self.mask = torch.zeros(C, dtype=torch.bool)
        self.mask[list(range(C)) if classes is None else sorted(set(classes))] = True
        self.K = int(self.mask.sum())
        self.smooth, self.alpha, self.beta, self.gamma = f32(smooth), f32(alpha), f32(beta), f32(gamma)
        self.c0 = f32(1.0 - self.alpha - self.beta)
        self.focal = self.gamma != 1.0
        self.e = f32(1.0 / self.gamma)
        self.em1 = self.e - 1.0
        self.per_image, self.ce_coef, self.tversky_coef = bool(per_image), float(ce_coef), float(tversky_coef)
        self.xd = x.detach().double().requires_grad_(True)
        self.keep = (t != ignore_index) & (t >= 0) & (t < C)
        self.tc = torch.where(self.keep, t, torch.zeros_like(t))
        k = self.keep[..., None].double()
        self.wd = torch.ones(C, dtype=torch.float64) if weight is None else torch.as_tensor(weight).double()
        self.wi = self.wd[self.tc] * self.keep
        self.p = torch.softmax(self.xd, -1)
        self.y = F.one_hot(self.tc, C).double() * k
        dims = (1,) if per_image else (0, 1)
        shape = (self.G, C)
        self.I = (self.p * self.y).sum(dims).reshape(shape)
        self.S = (self.p * k).sum(dims).reshape(shape)
        self.Y = self.y.sum(dims).reshape(shape)
        one, zero = torch.ones(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
        self.N = self.I + self.smooth
        self.Den = self.c0 * self.I + self.alpha * self.S + self.beta * self.Y + self.smooth
        self.empty = self.Den == 0
        self.T = torch.where(self.empty, one, self.N / torch.where(self.empty, one, self.Den))
        self.u = (1 - self.T).clamp(min=0)
        self.some = self.u > 0
        us = torch.where(self.some, 1 - self.T, one)                        # (u where it is > 0: the selects keep autograd off the rest)
        self.term = torch.where(self.some, torch.exp2(self.e * torch.log2(us)) if self.focal else us, zero)
        self.tversky = self.term[:, self.mask].sum() / (self.G * self.K)
        self.l = (torch.logsumexp(self.xd, -1) - self.xd.gather(-1, self.tc[..., None])[..., 0]) * self.keep
        self.sumw = self.wi.sum()
        self.ce = (self.wi * self.l).sum() / self.sumw
        self.total = torch.zeros((), dtype=torch.float64)
        if self.ce_coef != 0:
            self.total = self.total + self.ce_coef * self.ce
        if self.tversky_coef != 0:
            self.total = self.total + self.tversky_coef * self.tversky

    def autograd(self, g=1.0):
        """g * dtotal/dx by torch.autograd [B, PPI, C] (zeros when neither term depends on x)."""
        if not self.total.requires_grad:
            return torch.zeros_like(self.xd)
        return g * torch.autograd.grad(self.total, self.xd, retain_graph=True)[0]

    def coeffs(self):
        """(f, qa, qb) of the header, [G, C]: f = (m / (G K)) e u^(e - 1) (gamma == 1: m / (G K)), qa = f (1 - c0 T) / Den,
        qb = f alpha T / Den; 0 where the denominator is empty or u == 0."""
        with torch.no_grad():
            one, zero = torch.ones_like(self.Den), torch.zeros_like(self.Den)
            den = torch.where(self.empty, one, self.Den)
            us = torch.where(self.some, self.u, one)
            m = (self.mask.double() / (self.G * self.K)).expand_as(den)
            f = m * self.e * torch.exp2(self.em1 * torch.log2(us)) if self.focal else m
            f = torch.where(self.some, f, zero)
            return f, f * (1 - self.c0 * self.T) / den, f * self.alpha * self.T / den

    def _px(self, v):
        """A [G, C] table per pixel: [B, 1, C] under per_image, [1, 1, C] otherwise."""
        return v[:, None, :] if self.per_image else v[None]

    def q(self):
        """q_c = qb_gc - y_c qa_gc per pixel [B, PPI, C]."""
        _, qa, qb = self.coeffs()
        return self._px(qb) - self.y * self._px(qa)

    def closed_form(self, g=1.0):
        """The header's gradient: g (ce_coef (w_i / sum w)(p - y) + tversky_coef p (q - sum_k p_k q_k)); exactly 0 off the counted pixels."""
        with torch.no_grad():
            k = self.keep[..., None].double()
            d = torch.zeros_like(self.xd)
            if self.ce_coef != 0:
                d = d + self.ce_coef * (self.wi / self.sumw)[..., None] * (self.p - self.y)
            if self.tversky_coef != 0:
                q = self.q()
                d = d + self.tversky_coef * self.p * (q - (self.p * q).sum(-1, keepdim=True))
            return g * d * k


def grid_x(PPI, B, cap):
    return min((PPI + 255) // 256, max(1, cap // B))


class TverskyBounds:
    """The bounds of the module docstring for one reference ``r`` (TverskyRef of the fp32 logits ``x``)."""

    def __init__(self, r, x):
        self.r = r
        B, PPI, C = x.shape
        fbx = grid_x(PPI, B, FWD_BLOCKS)
        assert -(-PPI // (fbx * 256)) + 6 + 3 + max(-(-B * fbx // 256) + 6 + 3, -(-fbx // 64) + 6) <= SUM_DEPTH
        with torch.no_grad():
            xd = x.double()
            self.p = torch.softmax(xd, -1)
            self.spread = (xd - xd.max(-1, keepdim=True).values).abs()
            self.ep = (C + 6 + self.spread) * U * self.p
            k = r.keep[..., None].double()
            dims = (1,) if r.per_image else (0, 1)
            shape = (r.G, C)
            zero, one = torch.zeros(shape, dtype=torch.float64), torch.ones(shape, dtype=torch.float64)
            self.eS = (self.ep * k).sum(dims).reshape(shape) + SUM_DEPTH * U * r.S
            self.eI = (self.ep * r.y).sum(dims).reshape(shape) + SUM_DEPTH * U * r.I
            self.eY = SUM_DEPTH * U * r.Y
            I, S, Y, T, u = r.I.detach(), r.S.detach(), r.Y.detach(), r.T.detach(), r.u.detach()
            N, Den = r.N.detach(), r.Den.detach()
            c0a = abs(r.c0)
            self.eN = self.eI + U * N
            M = c0a * I + r.alpha * S + r.beta * Y + r.smooth
            self.eDen = c0a * self.eI + r.alpha * self.eS + r.beta * self.eY + U * (c0a * I + r.alpha * S + r.beta * Y) + 3 * U * M
            self.den1 = torch.where(r.empty, one, Den - self.eDen)          # Den - eDen (1 where the denominator is empty)
            assert (self.den1 > 0).all(), "Den - eDen <= 0 for a non-empty (g, c)"
            self.eT = torch.where(r.empty, zero, (self.eN + T * self.eDen) / self.den1 + U * T)
            self.eu = self.eT + U * u
            us = torch.where(r.some, u, one)
            eps_u = torch.where(r.some, self.eu / us, zero)
            lnu = us.log().abs()
            term = r.term.detach()
            if r.focal:
                self.e_term = torch.where(r.some, term * (r.e * eps_u + 7 * U * r.e * lnu + T6), zero)
                self.eps_f = abs(r.em1) * eps_u + 8 * U * abs(r.em1) * lnu + T6 + 3 * U
            else:
                self.e_term = self.eu
                self.eps_f = U * one
            GK = r.G * r.K
            self.e_tversky = self.e_term[:, r.mask].sum().item() / GK + (GK + 2) * U * term[:, r.mask].sum().item() / GK
            amax = xd.abs().max(-1).values
            e = (C + 8) * U * (3 * amax + math.log(C) + r.l.detach() + 1) * r.keep
            Nce = (r.wi * r.l.detach()).sum().item()
            self.e_sumw = SUM_DEPTH * U * r.sumw.item()
            self.e_ce = ((r.wi * e).sum().item() + (SUM_DEPTH + 1) * U * Nce) / r.sumw.item() + (SUM_DEPTH + 2) * U * abs(r.ce.item()) \
                if r.sumw.item() > 0 else float("nan")
            self.e_total = 0.0
            if r.ce_coef != 0:
                self.e_total += abs(r.ce_coef) * self.e_ce + 3 * U * abs(r.ce_coef * r.ce.item())
            if r.tversky_coef != 0:
                self.e_total += abs(r.tversky_coef) * self.e_tversky + 3 * U * abs(r.tversky_coef * r.tversky.item())
            # qa, qb
            f, qa, qb = r.coeffs()
            ef = f * self.eps_f
            A = 1 - r.c0 * T
            eA = c0a * self.eT + U * c0a * T + U * A.abs()
            eXa = ef * A.abs() + f * eA + U * (f * A).abs()
            self.e_qa = torch.where(r.some, (eXa + qa.abs() * self.eDen) / self.den1 + U * qa.abs(), zero)
            Xb = f * r.alpha * T
            eXb = ef * r.alpha * T + f * r.alpha * self.eT + 2 * U * Xb
            self.e_qb = torch.where(r.some, (eXb + qb * self.eDen) / self.den1 + U * qb, zero)

    def conditions(self):
        """What keeps a bound from hiding a failure, from the reference alone: under gamma != 1 every non-empty class of the mask has
        u >= 0.1 (below that u^(1/gamma - 1) amplifies the error of u without limit); under gamma == 1 such a class has u > 4 eu, so
        fp32 and float64 agree on which classes have a gradient.  A u of exactly 0 in the reference passes: random logits never give
        one, and a test that builds one builds it so that fp32 arithmetic gives exactly 0 too (and says how)."""
        r = self.r
        live = r.mask[None, :] & ~r.empty
        u = r.u.detach()
        if r.focal:
            assert ((u[live] >= 0.1) | (u[live] == 0)).all(), ("u < 0.1 under gamma != 1", u[live].min().item())
        else:
            assert ((u[live] > 4 * self.eu[live]) | (u[live] == 0)).all(), "u within 4 eu of 0"

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
            if r.tversky_coef != 0:
                q = r.q()
                e_q = r._px(self.e_qb) + r.y * r._px(self.e_qa) + U * q.abs()
                dot = (self.p * q).sum(-1, keepdim=True)
                e_dot = (self.ep * q.abs() + self.p * e_q).sum(-1, keepdim=True) + C * U * (self.p * q.abs()).sum(-1, keepdim=True)
                diff = q - dot
                e_diff = e_q + e_dot + U * diff.abs()
                bound = bound + abs(gg * r.tversky_coef) * (self.ep * diff.abs() + self.p * e_diff + 5 * U * self.p * diff.abs())
            bound = bound + U * d.abs() + 1e-30
            bound = torch.where(k, bound, torch.zeros_like(bound))
            if old is not None:
                d = d + old.double()
                bound = bound + torch.where(k, U * d.abs(), torch.zeros_like(bound))
            return d, bound

    def sentinel_margin(self, sen):
        """min over the sentinels of |T without it - T| / eT for the sentinel class (must exceed 4), and the smallest move itself."""
        r, sc = self.r, self.r.C - 1
        worst, move = float("inf"), float("inf")
        with torch.no_grad():
            for b in range(r.B):
                g = b if r.per_image else 0
                pj = self.p[b, sen, sc]
                assert r.keep[b, sen].all() and (r.tc[b, sen] == sc).all()
                num = r.N[g, sc] - pj
                den = r.Den[g, sc] - (r.c0 + r.alpha) * pj - r.beta
                Two = torch.where(den.abs() < 1e-9, torch.ones_like(den), num / den.clamp(min=1e-300))
                dT = (Two - r.T[g, sc]).abs()
                worst = min(worst, (dT / self.eT[g, sc]).min().item())
                move = min(move, dT.min().item())
            assert int(r.Y[:, sc].sum().item()) == r.B * len(sen)          # the seams alone carry the class
        return worst, move
