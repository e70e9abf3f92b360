"""The focal loss of include/dct.h (``dct_focal_*``) three times over, for tests/test_focal_cpu.py and tests/test_focal_gpu.py:

  * ``Ref``: the rule in float64 plain torch with autograd for the gradients, from exactly the fp32 logits and weights the kernels see,
    plus the per-pixel pieces ``q, m, l, k, w`` and the error bounds made of them;
  * ``restate32``: the same formulas evaluated in float32 on the CPU (what a correct fp32 evaluation gives);
  * ``inputs``: the test tensors, with sentinels at the seams of both grids and the planted confident pixels.

The reference forms l = -log p_t as -log1p(-q) while q < 1/2: in float64 too, logsumexp(x) - x_t of a pixel with q ~ 1e-17 is a rounding
error (its absolute error is ~1e-16 |x|), and the bounds below are relative.

The bounds (U: fp32 unit roundoff; T = 6 U: the three ulp tests/test_loss_kernels_scale_gpu.py allows a device transcendental; S: the
DEN = 2^-149: the spacing of the fp32 subnormals; every epsilon is a relative error):
  e_c = exp(x_c - max): the difference rounds once (U |x_c - max| in the argument, so in the result) and expf adds T.
  s = sum e_c and off = sum_{c != t} e_c (terms >= 0, at most C - 1 additions; each term's error weighs what the term contributes):
      eps_s = (C + 5) U + U sum_c p_c |x_c - max|,      eps_off = (C + 5) U + U sum_{c != t} p_c |x_c - max| / q.
  q = off * (1 / s): two roundings more; a q below the normal range keeps DEN absolute:   eps_q = eps_s + eps_off + 2 U + DEN / q.
  l:  q < 1/2:  -log1p(-q); d l / d q = 1 / (1 - q) and l >= q, so the error of q enters as eps_q / (1 - q), and log1pf adds T;
      q >= 1/2: (max - x_t) + log s, two terms >= 0: U (max - x_t) + eps_s + T log s + U l <= eps_s + 7 U l absolute, and l >= log 2.
      Within 0.01 of 1/2 the fp32 q may fall on either side: the larger of the two.
  m = q^gamma = exp2(gamma log2 q): log2f is off by T |log2 q|, the product by U more, exp2f turns the argument's absolute error
      (T + U) gamma |log2 q| into ln 2 times that, relative, and adds T:   eps_m = gamma eps_q + 7 U gamma |ln q| + T   (0 when gamma == 0:
      m is the constant 1).
  p_t = e_t * (1 / s):   eps_pt = eps_s + T + (|x_t - max| + 2) U.
  k = m (1 + gamma p_t (l / q)), a sum of two terms >= 0 (three products, one division, one addition and the last product):
      eps_k = eps_m + 2 U + (eps_l + eps_q + eps_pt + 3 U)   (0 when gamma == 0).
  f = w (m l):   eps_f = eps_m + eps_l + 2 U.
  gradient (g w k) v_c with v_c = p_c (c != t) or -q (c == t):   eps_v = eps_s + T + (|x_c - max| + 2) U + DEN / p_c, or eps_q;
      g = gscale * gmul [/ sum w]: 2 U, under the mean U and SUM_DEPTH U (the fp32 sum of the weights) more, the map's g * dmap U more;
      the products g w k v: 3 U.      The accumulate adds U |old + d|.
  Anything below TINY = 2^-126 may come back as a subnormal or as 0 (a q that underflows to 0 is m = k = 0 by the rule): every bound
  carries TINY times the factors in front of it.
  Sums: a tree of depth SUM_DEPTH adds SUM_DEPTH U sum |f_i|; the mean adds the sum of the weights and the division."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
T = 6 * U
DEN = 2.0 ** -149
TINY = 2.0 ** -126
SUM_DEPTH = 32          # tests/test_loss_kernels_scale_gpu.py: the levels of the kernels' reduction
IGN = 255
MEAN, SUM = 0, 1
RED = {MEAN: "mean", SUM: "sum"}
PLANTS = ("c20", "c40", "c120", "low")
CASES = [  # P, C, gamma, reduction, accumulate, stray targets, weighted (else weight = NULL)
    (1, 2, 2.0, MEAN, False, False, True), (1, 3, 0.0, SUM, True, False, False), (255, 3, 0.5, SUM, False, False, True),
    (255, 8, 1.0, MEAN, True, False, False), (257, 4, 5.0, MEAN, True, True, True), (257, 2, 0.0, SUM, False, False, True),
    (262145, 2, 1.0, SUM, True, False, True), (262145, 4, 2.0, MEAN, False, False, True), (262145, 8, 0.5, SUM, False, True, False),
    (262145, 3, 5.0, MEAN, True, False, True), (2097153, 3, 2.0, MEAN, False, False, True), (2097153, 2, 0.5, SUM, True, False, False),
]


def strides(P):
    b = max(1, (P + 255) // 256)
    return min(b, 1024) * 256, min(b, 8192) * 256


def sentinels(P):
    """tests/test_loss_kernels_scale_gpu.py's: the seams of ``grid_for``'s and ``wide_grid``'s walks."""
    s1, s2 = strides(P)
    return torch.tensor(sorted({i for i in (0, 255, 256, s1 - 1, s1, 2 * s1, s2 - 1, s2, 2 * s2, P - 1) if 0 <= i < P}))


def weights(C, alt=False):
    """A non-dyadic value, a one, a zero and one above 1, cycled to C (tests/test_weighted_ce_gpu.py's set)."""
    if C == 2:
        return torch.tensor([2.5, 0.0] if alt else [0.1, 1.0], dtype=torch.float32)
    return torch.tensor([(0.1, 1.0, 0.0, 2.5)[c % 4] for c in range(C)], dtype=torch.float32)


def inputs(P, C, w, stray, seed):
    """fp32 logits [P, C], targets (a quarter ignored; ``stray``: a few are C and -1), the targets a reference may see (the stray ones
    ignored), the sentinels (target logit -D, the others 0: q = 1, l = D + log(C - 1), on classes of non-zero weight) and the planted
    pixels {name: indices}, on classes of non-zero weight too: ``c20`` / ``c40`` / ``c120``: the target logit 20 / 40 / 120 above the
    largest other one (q ~ 1e-9, ~ 1e-17, and 0 in fp32); ``low``: the target logit 150 below the rest (p_t = 0 in fp32, q = 1).  Two
    pixels of each where there is room; a single pixel is its own sentinel, which is a ``low`` pixel."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g) * 2
    t = torch.randint(0, C, (P,), generator=g)
    t[torch.rand(P, generator=g) < 0.25] = IGN
    used = set()
    if stray:
        idx = (torch.arange(6) * P // 7 + 1) % P
        t[idx[:3]] = C
        t[idx[3:]] = -1
        used |= set(idx.tolist())
    sen = sentinels(P)
    nz = torch.nonzero(w)[:, 0]
    D = max(1e4, 0.1 * P)
    t[sen] = nz[sen % len(nz)]
    x[sen] = 0.0
    x[sen, t[sen]] = -D
    used |= set(sen.tolist())
    free = [i for i in range(min(P, 4096)) if i not in used and i % 5 == 3][:2 * len(PLANTS)]
    plants = {}
    for n, name in enumerate(PLANTS):
        idx = torch.tensor(free[2 * n:2 * n + 2], dtype=torch.int64)
        plants[name] = idx
        if len(idx) == 0:
            continue
        tt = nz[(idx + n) % len(nz)]
        t[idx] = tt
        x[idx, tt] = -1e30
        top = x[idx].max(1).values              # the largest other logit
        x[idx, tt] = top + {"c20": 20.0, "c40": 40.0, "c120": 120.0, "low": -150.0}[name]
    t_ref = torch.where((t < 0) | (t >= C), torch.full_like(t, IGN), t)
    if stray:
        assert int(((t != IGN) & (t_ref == IGN)).sum()) >= 3
    return g, x, t, t_ref, sen, plants


def _pieces(xd, tc, gamma):
    """p, q, l, m, k of every pixel in the dtype of ``xd`` (differentiable in float64), by the formulas of the header."""
    one = torch.ones((), dtype=xd.dtype)
    zero = torch.zeros((), dtype=xd.dtype)
    mx = xd.max(1, keepdim=True).values
    e = torch.exp(xd - mx)
    onehot = F.one_hot(tc, xd.shape[1]).to(xd.dtype)
    s = e.sum(1)
    off = (e * (1 - onehot)).sum(1)
    inv = 1 / s
    p = e * inv[:, None]
    pt = (p * onehot).sum(1)
    xt = (xd * onehot).sum(1)
    q = off * inv
    small = q < 0.5
    l = torch.where(small, -torch.log1p(-torch.where(small, q, zero)), (mx[:, 0] - xt) + torch.log(s))
    if gamma == 0:
        return p, q, l, torch.ones_like(q), torch.ones_like(q), onehot
    some = q > 0
    qs = torch.where(some, q, one)
    pw = torch.exp2(gamma * torch.log2(qs))
    tl = torch.where(pt > 0, pt * (l / qs), zero)
    return p, q, l, torch.where(some, pw, zero), torch.where(some, pw * (1 + gamma * tl), zero), onehot


def restate32(x, t_ref, w, gamma):
    """The rule in float32 on the CPU: (map f [P], sum f, sum w, the gradient's w k (p - y) [P, C]); uncounted pixels 0."""
    C = x.shape[1]
    keep = t_ref != IGN
    tc = t_ref.clamp(max=C - 1)
    with torch.no_grad():
        p, q, l, m, k, onehot = _pieces(x.float(), tc, float(gamma))
        wi = torch.where(keep, w.float()[tc], torch.zeros(()))
        f = torch.where(keep, wi * (m * l), torch.zeros(()))
        v = torch.where(onehot > 0, -q[:, None], p)
        d = torch.where(keep[:, None], (wi * k)[:, None] * v, torch.zeros(()))
    return f, f.sum(), wi.sum(), d


class Ref:
    """float64 reference of one (x, t, w, gamma): values, autograd gradients, pieces and bounds."""

    def __init__(self, x, t_ref, w, C, gamma):
        self.C, self.gamma = C, float(gamma)
        self.wd = w.double()
        self.xd = x.double().requires_grad_(True)
        self.t = t_ref
        self.keep = keep = t_ref != IGN
        self.tc = tc = t_ref.clamp(max=C - 1)
        z = torch.zeros((), dtype=torch.float64)
        self.wi = torch.where(keep, self.wd[tc], z)
        p, q, l, m, k, onehot = _pieces(self.xd, tc, self.gamma)
        self.fmap = torch.where(keep, self.wi * (m * l), z)            # (with a graph)
        with torch.no_grad():
            xd = self.xd
            self.p, self.q, self.l, self.m, self.k, self.onehot = p.detach(), q.detach(), l.detach(), m.detach(), k.detach(), onehot
            self.f = self.fmap.detach()
            self.N, self.D = self.f.sum().item(), self.wi.sum().item()
            self.spread = (xd - xd.max(1, keepdim=True).values).abs()
            q, l, p = self.q, self.l, self.p
            st = (self.spread * onehot).sum(1)
            es = (C + 5) * U + U * (p * self.spread).sum(1)
            eoff = (C + 5) * U + U * (p * self.spread * (1 - onehot)).sum(1) / q.clamp(min=1e-300)
            eq = es + eoff + 2 * U + DEN / q.clamp(min=1e-300)
            el_small = eq / (1 - q).clamp(min=0.49) + T
            el_big = (es + 7 * U * l) / l.clamp(min=0.5)
            el = torch.where(q < 0.49, el_small, torch.where(q > 0.51, el_big, torch.maximum(el_small, el_big)))
            if self.gamma == 0:
                em = ek = torch.zeros_like(q)
            else:
                em = self.gamma * eq + 7 * U * self.gamma * q.clamp(min=1e-300).log().abs() + T
                ept = es + T + (st + 2) * U
                ek = em + 2 * U + el + eq + ept + 3 * U
            self.eq, self.el, self.em, self.ek = eq, el, em, ek
            self.ef_rel = em + el + 2 * U
            self.ef = torch.where(keep, self.f * self.ef_rel + TINY * self.wi.clamp(min=1.0), z)      # per pixel, absolute
            self.ev = torch.where(onehot > 0, eq[:, None], (es + T)[:, None] + (self.spread + 2) * U + DEN / p.clamp(min=1e-300))
            self.v = torch.where(onehot > 0, -q[:, None], p)
            self.num_tol = self.ef.sum().item() + SUM_DEPTH * U * self.N

    def closed_form(self):
        """w k (p - y) of the header, the target's entry as -q."""
        return torch.where(self.keep[:, None], (self.wi * self.k)[:, None] * self.v, torch.zeros((), dtype=torch.float64))

    def value(self, reduction):
        """(loss as a float64 tensor with a graph, tolerance)"""
        total = self.fmap.sum()
        if reduction == MEAN:
            loss = total / self.wi.sum()
            return loss, self.num_tol / self.D + (SUM_DEPTH + 2) * U * abs(loss.item())
        return total, self.num_tol

    def grad(self, loss, gfac, mean=False, per_pixel=False, old=None, grad_outputs=None):
        """gfac * d loss / d x (+ old) by autograd and its bound; ``gfac``: per pixel [P] or scalar, the g of (g w k)(p - y)."""
        (d,) = torch.autograd.grad(loss, self.xd, grad_outputs=grad_outputs, retain_graph=True)
        gw = (torch.as_tensor(gfac, dtype=torch.float64) * self.wi).abs().reshape(-1, 1)
        eg = (2 + (1 + SUM_DEPTH if mean else 0) + (1 if per_pixel else 0) + 3) * U
        bound = torch.where(self.keep[:, None], gw * self.k[:, None] * self.v.abs() * (self.ek[:, None] + self.ev + eg) + TINY * gw.clamp(min=1.0),
                            torch.zeros((), dtype=torch.float64))
        if old is not None:
            d = d + old.double()
            bound = bound + U * d.abs()
        return d, bound


def ce_bounds(r):
    """tests/test_weighted_ce_gpu.py's bounds of dct_ce_weighted_* on the pixels of ``r`` (a ``Ref`` of gamma = 0): (the numerator's
    tolerance, the per-pixel map bound, a function (|g w|, k) -> gradient bound)."""
    C = r.C
    amax = r.xd.detach().abs().max(1).values
    z = torch.zeros((), dtype=torch.float64)
    e = torch.where(r.keep, (C + 8) * U * (3 * amax + math.log(C) + r.l + 1), z)
    num_tol = (r.wi * e).sum().item() + (SUM_DEPTH + 1) * U * r.N

    def grad_bound(gfac, k):
        gw = (torch.as_tensor(gfac, dtype=torch.float64) * r.wi).abs().reshape(-1, 1)
        return torch.where(r.keep[:, None], gw * ((C + 6 + r.spread) * U * r.p + k * U * (r.p - r.onehot).abs()) + 1e-30, z)
    return num_tol, r.wi * e + U * r.f, grad_bound
