"""Reference of the pseudo-label consistency term (the rule: include/dct.h, dct_pl_*) for tests/test_pseudo_label_*.py.

The teachers (argmax, confidence, mask) are derived in fp32 exactly as the rule states them -- numpy float32, sequential adds for the
ensemble -- so that a kernel's teachers can be compared bit for bit.  Given the teachers, values and gradients are float64, with
``p + eps`` formed in fp32 as the kernels form it (the way tests/test_loss_kernels_scale_gpu.py treats KL), and every function
returns the bound on |fp32 kernel - float64| that follows from the kernels' arithmetic beside the value.
"""
import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
TINY = 2.0 ** -126      # smallest normal fp32
LOG_ULP = 6             # the device logf is allowed 3 ulp = 6U relative to |log q| (tests/test_loss_kernels_scale_gpu.py)
SUM_DEPTH = 32          # levels of the kernels' fp32 reduction of a per-pixel value (tests/test_loss_kernels_scale_gpu.py)
CROSS, ENSEMBLE = "cross", "ensemble"


def first_max(v):
    """Index of the first maximum along the last axis by the rule of dct_argmax: ``v[c] > v[best]``, starting at 0."""
    v = np.asarray(v)
    best = np.zeros(v.shape[:-1], dtype=np.int64)
    bv = v[..., 0].copy()
    for c in range(1, v.shape[-1]):
        up = v[..., c] > bv
        best = np.where(up, c, best)
        bv = np.where(up, v[..., c], bv)
    return best, bv


def teachers_fp32(probs, teacher, tau):
    """``probs``: S float32 arrays [P, C].  -> (k [T, P] int64, m [T, P] bool, q [T, P] float32) with T = S teacher views for
    ``cross`` and T = 1 for ``ensemble``; every operation in fp32, in the rule's order."""
    probs = [np.ascontiguousarray(np.asarray(p, dtype=np.float32)) for p in probs]
    S = len(probs)
    tau = np.float32(tau)
    if teacher == CROSS:
        assert S >= 2
        kq = [first_max(p) for p in probs]
        k = np.stack([a for a, _ in kq])
        q = np.stack([b for _, b in kq]).astype(np.float32)
    else:
        assert teacher == ENSEMBLE and S >= 1
        s = probs[0].copy()
        for p in probs[1:]:
            s = (s + p).astype(np.float32)                  # ((p_0 + p_1) + ...), one rounding per add
        k, bv = first_max(s)                                # on the unscaled sums
        q = (bv.astype(np.float32) * (np.float32(1.0) / np.float32(S))).astype(np.float32)
        k, q = k[None], q[None]
    return k, q >= tau, q


def kept_map(m, teacher, S):
    """The per-pixel kept map, float32: kept teacher terms of the pixel / its total (S for cross, 1 for ensemble)."""
    if teacher == CROSS:
        return (m.sum(0).astype(np.float32) / np.float32(S)).astype(np.float32)
    return m[0].astype(np.float32)


def term_counts(k, m, teacher, S, C):
    """n [S, P, C] float64: the kept teacher terms of class c that student i meets (cross: the other views'; ensemble: the vote's)."""
    P = k.shape[1]
    onehot = (k[:, :, None] == np.arange(C)[None, None, :]) & m[:, :, None]          # [T, P, C]
    if teacher == CROSS:
        tot = onehot.sum(0)
        n = np.stack([tot - onehot[i] for i in range(S)])
    else:
        n = np.broadcast_to(onehot[0], (S, P, C))
    return torch.from_numpy(np.ascontiguousarray(n).astype(np.float64))


def weight(teacher, S):
    return 1.0 / (S * (S - 1)) if teacher == CROSS else 1.0 / S


def map_and_grad(probs, n, teacher, eps, fp32_sum=True):
    """Given the teacher terms ``n``: float64 map [P], its bound, d map / d p_i [S, P, C] and the relative bound of that gradient.
    ``fp32_sum``: p + eps is rounded to fp32 first, as the kernels form it (False: the rule in exact arithmetic)."""
    S = len(probs)
    C = probs[0].shape[1]
    w = weight(teacher, S)
    p32 = torch.stack([torch.as_tensor(np.asarray(p)) for p in probs])
    pe = (p32.float() + torch.tensor(eps, dtype=torch.float32)).double() if fp32_sum else p32.double() + eps
    L = torch.log(pe)
    terms = n * -L                                           # [S, P, C]
    v = w * terms.sum((0, 2))
    # per term: logf 6U|L| + U and the product U; the chain of at most S C fused adds U each on the magnitudes; w (rounded) and the final
    # product 2U
    vabs = w * (n * L.abs()).sum((0, 2))
    bound = w * (n * (LOG_ULP * U * L.abs() + U)).sum((0, 2)) + (S * C + 3) * U * vabs
    d = -(w * n) / pe
    # w rounded, w n, the division: 3U relative (one more when the map backward multiplies by dmap)
    return v, bound, d, 4 * U


def rule_autograd(probs64, k, m, teacher, eps):
    """The rule written out literally with torch ops on float64 leaves ``probs64`` (requires_grad), the teachers as constants:
    -> map [P].  The closed-form gradient of ``map_and_grad`` is checked against autograd through this."""
    S = len(probs64)
    kt, mt = torch.from_numpy(k), torch.from_numpy(m).double()
    ls = []
    for i in range(S):
        if teacher == CROSS:
            li = 0.0
            for j in range(S):
                if j != i:
                    li = li + mt[j] * torch.log(probs64[i].gather(1, kt[j][:, None])[:, 0] + eps)
            ls.append(-li / (S - 1))
        else:
            ls.append(-mt[0] * torch.log(probs64[i].gather(1, kt[0][:, None])[:, 0] + eps))
    return sum(ls) / S


def logit_grad(p32, d, g, C):
    """o = g p (d - sum_c d p) in float64 from the fp32 probabilities the kernel holds, and its bound: d carries 4U relative, each
    product of the dot U and its C-term sum C U on the magnitudes, the subtraction U; then g (gscale * gmul / P: 2U) and the two
    products."""
    p = torch.as_tensor(np.asarray(p32)).double()
    dp = d * p
    dot = dp.sum(-1, keepdim=True)
    ref = g * p * (d - dot)
    sabs = dp.abs().sum(-1, keepdim=True)
    bound = abs(g) * p * (5 * U * d.abs() + (6 + C) * U * sabs) + 6 * U * ref.abs() + 1e-30
    return ref, bound
