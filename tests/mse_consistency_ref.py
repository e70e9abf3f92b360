"""Reference of the softmax-MSE consistency term (the rule: include/dct.h, dct_mse_*) for tests/test_mse_consistency_*.py.

The first maximum, the confidence and the mask are pseudo_label_ref's (fp32, numpy, in the rule's order), so that a kernel's kept map can
be compared bit for bit; the ensemble's teacher vector ``q = sum * (1.f / (float)S)`` is the rule's fp32 quantity, formed from
soft_label_ref's fp32 sums with one more fp32 product.  Given those, the map, d map / d p and the logit gradient are float64, computed
from the fp32 probabilities the kernel holds.  Every function returns the bound on |fp32 kernel - float64| beside the value.

The bounds (U = 2^-24; every rounded operation contributes at most one U of its result's magnitude; every line is what the kernel's
arithmetic gives and nothing measured from it):
  e = p_i[c] - t[c] (t = p_j[c] or q[c], both fp32):  one subtraction, U |e|.
  e^2 as a rounded product: the two factors carry U each and the product rounds once, 3 U e^2 (+ TINY: a square below the normal range
      may come back as a subnormal or as 0).
  sq = e[0]^2 + ... + e[C-1]^2, terms >= 0, added in class order from 0 (the first add is exact): (C - 1) U sq.
  a_i = the sum of the kept sq over j != i, from 0: (S - 1) U a_i (cross; ensemble: a_i = sq);  a = a_0 + ... + a_{S-1}: S U a (the step
      kernel may fuse w a into its running sum: one rounding fewer);  w itself (1.f / (float)n: U) and the product w a (U).
      Together (3 + (C - 1) + (S - 1) + S + 2) U = (C + 2 S + 3) U of the value, one spare U on top: all terms are >= 0, so the
      magnitudes are the values.
  d map / d p_i[c] = 2 w * sum_j m_j e_ij[c]:  each e carries U |e|, the chain of at most S - 1 adds (S - 1) U on sum_j |e_ij[c]|, 2 w is
      w's U (the doubling is exact) and the product U:  S U * 2 w * sum_j m_j |e_ij[c]| + 2 U |d|, one spare U |d| on top.
      Ensemble: one e, no chain: U |d| + 2 U |d|, the same spare.
  logit gradient g p (d - sum d p): soft_label_ref.logit_grad's bound with this absolute error of d.
"""
import numpy as np
import torch

import pseudo_label_ref as PR
import soft_label_ref as SR
from soft_label_ref import CROSS, ENSEMBLE, SUM_DEPTH, TINY, U, logit_grad  # noqa: F401


def weight(teacher, S, C):
    """w = 1 / (C S (S - 1)) resp. 1 / (C S), as the exact rational the rule names (the kernel's fp32 w is off by at most U of it)."""
    return 1.0 / (C * S * (S - 1)) if teacher == CROSS else 1.0 / (C * S)


def teachers(probs, teacher, tau):
    """-> (t [T, P, C] float32 teacher vectors, m [T, P] bool mask): m is pseudo_label_ref.teachers_fp32's; cross: t_j = p_j (T = S);
    ensemble: t = q = sum * (1.f / (float)S) in fp32 from soft_label_ref.raw_vectors' sums (T = 1), whose entry at the first maximum is
    pseudo_label_ref's confidence bit for bit (asserted)."""
    S = len(probs)
    k, m, conf = PR.teachers_fp32(probs, teacher, tau)
    raw = SR.raw_vectors(probs, teacher)
    if teacher == CROSS:
        t = raw
    else:
        t = (raw * (np.float32(1.0) / np.float32(S))).astype(np.float32)
    for j in range(t.shape[0]):
        assert np.array_equal(np.take_along_axis(t[j], k[j][:, None], 1)[:, 0], conf[j])
    return t, m


def map_and_grad(probs, t, m, teacher):
    """Given the teacher vectors and masks: float64 map [P], its bound, d map / d p_i [S, P, C] and the ABSOLUTE bound of that gradient."""
    S = len(probs)
    C = probs[0].shape[1]
    w = weight(teacher, S, C)
    p = torch.stack([torch.as_tensor(np.asarray(pp, dtype=np.float32)) for pp in probs]).double()        # [S, P, C]
    td = torch.from_numpy(np.ascontiguousarray(t)).double()                                               # [T, P, C]
    md = torch.from_numpy(np.ascontiguousarray(m)).double()[..., None]                                    # [T, P, 1]
    a = torch.zeros(p.shape[1], dtype=torch.float64)
    d = torch.zeros_like(p)
    dabs = torch.zeros_like(p)
    for i in range(S):
        for j in ([j for j in range(S) if j != i] if teacher == CROSS else [0]):
            e = md[j] * (p[i] - td[j])
            a = a + (e * e).sum(1)
            d[i] += e
            dabs[i] += e.abs()
    v = w * a
    d = 2.0 * w * d
    vb = (C + 2 * S + 4) * U * v + S * S * C * TINY
    chain = S if teacher == CROSS else 1
    db = chain * U * 2.0 * w * dabs + 3 * U * d.abs()
    return v, vb, d, db


def rule(probs, teacher, tau):
    """-> (m, v, vb, d, db): the whole reference of one set of fp32 probability maps."""
    t, m = teachers(probs, teacher, tau)
    return (m,) + map_and_grad(probs, t, m, teacher)


def rule_autograd(probs64, t, m, teacher):
    """The rule written out literally with torch ops on float64 leaves ``probs64`` (requires_grad), the teacher vectors ``t`` and the masks
    as constants (detached by construction: they come in as numpy) -> map [P]: the mean over classes, teacher terms and students of the
    squared error."""
    S = len(probs64)
    td = torch.from_numpy(np.ascontiguousarray(t)).double()
    md = torch.from_numpy(np.ascontiguousarray(m)).double()
    ls = []
    for i in range(S):
        if teacher == CROSS:
            li = 0.0
            for j in range(S):
                if j != i:
                    li = li + md[j] * ((probs64[i] - td[j]) ** 2).mean(1)
            ls.append(li / (S - 1))
        else:
            ls.append(md[0] * ((probs64[i] - td[0]) ** 2).mean(1))
    return sum(ls) / S
