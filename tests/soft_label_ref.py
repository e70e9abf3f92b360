"""Reference of the soft pseudo-label consistency term (the rule: include/dct.h, dct_spl_*) for tests/test_soft_label_*.py.

The raw teacher vector ``q``, its first maximum ``k``, the mask ``m`` and the kept map are pseudo_label_ref's (fp32, numpy, in the
rule's order), so that a kernel's teachers can be compared bit for bit.  Given those, the sharpened targets ``t``, the student terms
``n``, the map, d map / d p and the logit gradient are float64, computed from the fp32 probabilities the kernel holds, with
``p + eps`` rounded to fp32 as the kernel forms it.  Every function returns the bound on |fp32 kernel - float64| beside the value.

The bounds (U = 2^-24; TR = 6 U: the three ulp the project allows a device transcendental, tests/focal_ref.py; every line is what
the kernel's arithmetic gives and nothing measured from it):
  z = r (log2 q[c] - log2 q[k]):  a = log2f(q[c]) is off by TR |a|, b = log2f(q[k]) by TR |b|, the difference rounds once, U |a - b|, and
      the product with r once more, U |z|:         dz = r (TR (|a| + |b|) + U |a - b|) + U |z|      (r itself is the kernel's fp32 r, exact here).
  u = exp2f(z), focal_ref's treatment of exp2(gamma log2 q): the argument's absolute error dz becomes the factor 2^dz - 1 on u and
      exp2f adds TR relative; a u below the normal range may come back as a subnormal or as 0:   du = u (2^dz - 1) + TR u + TINY.
      The part of dz that is relative to |z| weighs |z| 2^z <= 1 / (e ln 2) on u, so it stays finite as r grows; the part that comes
      from the cancellation of two logs (TR (|a| + |b|) r) grows with r while 2^z is not yet 0 -- as the true error does.
      u[k] = 1 and u[c] = 0 where q[c] == 0 are exact (du = 0).
  s = u[0] + ... + u[C-1], terms >= 0, C - 1 additions:     ds = sum du + (C - 1) U s;       t = u / s:     dt = du / s + t ds / s + U t.
  n_i = the sum of the kept teachers' t over j != i (at most S - 1 terms >= 0):     dn = sum dt + (S - 1) U n;    ensemble: n = m t, dn = m dt.
  map = w sum n * -log(p + eps): pseudo_label_ref's bound with n real (logf 6 U |L| + U, the product U, the chain of S C adds, w and the
      last product) plus dn |L| per term.
  d map / d p = -(w n) / (p + eps): 4 U relative as pseudo_label_ref allows (w rounded, w n, the division, one spare) plus w dn / (p + eps).
  logit gradient g p (d - sum d p): pseudo_label_ref.logit_grad's bound with the absolute error of d in place of its 4 U |d|.
"""
import math

import numpy as np
import torch

import pseudo_label_ref as PR
from pseudo_label_ref import CROSS, ENSEMBLE, LOG_ULP, SUM_DEPTH, TINY, U  # noqa: F401

TR = 6 * U              # a device transcendental: 3 ulp (tests/focal_ref.py's T)


def rate(temperature):
    """r = 1.f / T as the kernels form it in fp32, as a Python float."""
    return float(np.float32(1.0) / np.float32(temperature))


def raw_vectors(probs, teacher):
    """q [T, P, C] float32: cross: the S views themselves; ensemble: ((p_0 + p_1) + ...), one rounding per add (T = 1)."""
    probs = [np.ascontiguousarray(np.asarray(p, dtype=np.float32)) for p in probs]
    if teacher == CROSS:
        return np.stack(probs)
    s = probs[0].copy()
    for p in probs[1:]:
        s = (s + p).astype(np.float32)
    return s[None]


def teachers(probs, teacher, tau):
    """-> (q [T, P, C] float32 raw vectors, k [T, P] first maxima, m [T, P] mask): k and m are pseudo_label_ref.teachers_fp32's."""
    k, m, _ = PR.teachers_fp32(probs, teacher, tau)
    q = raw_vectors(probs, teacher)
    for j in range(q.shape[0]):
        assert np.array_equal(PR.first_max(q[j])[0], k[j])          # (the same vectors the hard rule takes its argmax of)
    return q, k, m


def top_two_ratio_at_most_half(q):
    """The hard limit's precondition: every raw teacher vector's second-largest entry is at most half its largest."""
    top = np.sort(q.astype(np.float64), axis=-1)
    return bool((top[..., -2] <= 0.5 * top[..., -1]).all())


def sharpen(q, k, temperature):
    """t [T, P, C] float64 = Sharpen(q, T) by the rule from the fp32 vectors ``q``, and the bound dt on |kernel t - t|."""
    r = rate(temperature)
    C = q.shape[-1]
    qd = torch.from_numpy(np.ascontiguousarray(q)).double()
    kt = torch.from_numpy(np.ascontiguousarray(k))[..., None]
    is_k = torch.arange(C)[None, None, :] == kt
    zero = qd == 0
    exact = is_k | zero
    a = torch.log2(qd.clamp(min=1e-300))
    b = torch.log2(qd.gather(-1, kt).clamp(min=1e-300))
    z = r * (a - b)
    u = torch.where(zero, torch.zeros_like(z), torch.exp2(z))
    u = torch.where(is_k, torch.ones_like(u), u)
    dz = r * (TR * (a.abs() + b.abs()) + U * (a - b).abs()) + U * z.abs()
    du = u * torch.expm1(dz * math.log(2.0)) + TR * u + TINY
    du = torch.where(exact, torch.zeros_like(du), du)
    s = u.sum(-1, keepdim=True)
    ds = du.sum(-1, keepdim=True) + (C - 1) * U * s
    t = u / s
    dt = du / s + t * ds / s + U * t
    return t, dt


def terms(t, dt, m, teacher, S):
    """n [S, P, C] float64: what student i meets of class c (cross: the other views' kept sharpened targets; ensemble: the one), and
    its bound dn."""
    mt = torch.from_numpy(np.ascontiguousarray(m)).double()[..., None]
    tm, dtm = t * mt, dt * mt
    if teacher == CROSS:
        n = torch.stack([sum(tm[j] for j in range(S) if j != i) for i in range(S)])
        dn = torch.stack([sum(dtm[j] for j in range(S) if j != i) for i in range(S)]) + (S - 1) * U * n
    else:
        n, dn = tm[0].expand(S, -1, -1).clone(), dtm[0].expand(S, -1, -1).clone()
    return n, dn


def soft_terms(probs, teacher, tau, temperature):
    """-> (m, n, dn): the whole teacher side of one set of fp32 probability maps."""
    q, k, m = teachers(probs, teacher, tau)
    t, dt = sharpen(q, k, temperature)
    n, dn = terms(t, dt, m, teacher, len(probs))
    return m, n, dn


def map_and_grad(probs, n, dn, teacher, eps, fp32_sum=True):
    """Given the student terms: float64 map [P], its bound, d map / d p_i [S, P, C] and the ABSOLUTE bound of that gradient.
    ``fp32_sum``: p + eps is rounded to fp32 first, as the kernels form it (False: the rule in exact arithmetic)."""
    S = len(probs)
    C = probs[0].shape[1]
    w = PR.weight(teacher, S)
    p32 = torch.stack([torch.as_tensor(np.asarray(p)) for p in probs])
    pe = (p32.float() + torch.tensor(eps, dtype=torch.float32)).double() if fp32_sum else p32.double() + eps
    L = torch.log(pe)
    v = w * (n * -L).sum((0, 2))
    vabs = w * (n * L.abs()).sum((0, 2))
    bound = w * (n * (LOG_ULP * U * L.abs() + U) + dn * L.abs()).sum((0, 2)) + (S * C + 3) * U * vabs
    d = -(w * n) / pe
    return v, bound, d, 4 * U * d.abs() + w * dn / pe


def rule_autograd(probs64, q, k, m, teacher, temperature, eps):
    """The rule written out literally with torch ops on float64 leaves ``probs64`` (requires_grad): Sharpen as the normalised power
    (q / q[k]) ** r of the raw vectors, held constant -> map [P]."""
    S = len(probs64)
    r = rate(temperature)
    qd = torch.from_numpy(np.ascontiguousarray(q)).double()
    kt = torch.from_numpy(np.ascontiguousarray(k))[..., None]
    mt = torch.from_numpy(np.ascontiguousarray(m)).double()
    pw = (qd / qd.gather(-1, kt)) ** r
    t = pw / pw.sum(-1, keepdim=True)
    ls = []
    for i in range(S):
        logp = torch.log(probs64[i] + eps)
        if teacher == CROSS:
            li = 0.0
            for j in range(S):
                if j != i:
                    li = li + mt[j] * (t[j] * logp).sum(1)
            ls.append(-li / (S - 1))
        else:
            ls.append(-mt[0] * (t[0] * logp).sum(1))
    return sum(ls) / S


def pairwise_cross_entropy(probs, eps):
    """mean over ordered pairs i != j of sum_c p_j[c] / (sum_c' p_j[c']) * -log(p_i[c] + eps), float64 -> [P]."""
    ps = [torch.as_tensor(np.asarray(p)).double() for p in probs]
    S = len(ps)
    tot = 0.0
    for i in range(S):
        for j in range(S):
            if j != i:
                tot = tot + ((ps[j] / ps[j].sum(1, keepdim=True)) * -torch.log(ps[i] + eps)).sum(1)
    return tot / (S * (S - 1))


def logit_grad(p32, d, dbound, g, C):
    """o = g p (d - sum_c d p) in float64 from the fp32 probabilities the kernel holds, and its bound: d carries ``dbound`` absolute,
    each product of the dot U and its C-term sum C U on the magnitudes, the subtraction U; then g (gscale * gmul / P: 2 U) and the two
    products (pseudo_label_ref.logit_grad with the absolute error of d)."""
    p = torch.as_tensor(np.asarray(p32)).double()
    dp = d * p
    dot = dp.sum(-1, keepdim=True)
    ref = g * p * (d - dot)
    sabs = dp.abs().sum(-1, keepdim=True)
    ddot = (dbound * p).sum(-1, keepdim=True)
    bound = abs(g) * p * (dbound + U * d.abs() + ddot + (6 + C) * U * sabs) + 6 * U * ref.abs() + 1e-30
    return ref, bound
