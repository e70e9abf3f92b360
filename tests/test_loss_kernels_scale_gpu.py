"""The kernels of csrc/loss.hip at training scale, against float64 CPU references computed from exactly the fp32 tensors the
kernels see: cross entropy, softmax, entropy, JSD, KL and argmax over pixel counts that cross every grid cap (``grid_for``: 1024
blocks, so a thread walks several pixels above 262,144; ``wide_grid``: 8192 blocks, above 2,097,152), Dice counts at slice size, and
the device-state Adam path (table lookup, out-of-table fallback, FusedAdam's in-place table rebuild).

Every tolerance is derived from the fp32 error of the operation (comments at each bound; U is the fp32 unit roundoff).  The reductions
carry *sentinel* pixels -- at 0, 255, 256, stride - 1, stride, 2 stride and P - 1 of both grids -- each worth far more than the bound,
so a kernel that loses or double-counts one pixel fails; per-pixel outputs are pre-filled with NaN, so a pixel never written fails."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
from oracle.dice import _one_hots  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24          # fp32 unit roundoff
IGN = 255
TINY = 2.0 ** -126      # smallest normal fp32: a result below it may come back flushed to zero
EPS_ENT = 1e-16         # entropy_px / dent (loss.py:80)
EPS_KL = float(np.float32(1e-10))   # the KL eps as the kernels receive it
# The device logf is allowed 3 ulp (6U relative to |log q|): it lands 2.4 ulp off at log(1e-16f), the log of every underflowed probability.
# Levels of the kernels' fp32 reduction of a per-pixel value: <= 9 grid-stride trips per thread (P <= 2,097,153 over 1024 x 256
# threads), 6 wave-shuffle levels, the 4 wave sums, the finalize's 4 strided partials and its 8-level LDS tree.  A sum along a tree of
# depth d is off by at most d U sum|terms| (first order).
SUM_DEPTH = 32
MARGIN_SAT = 40.0       # softmax saturated: the other probabilities ~e^-35, far below U, so fp32 rounds the top one to exactly 1
MARGIN_UFL = 120.0      # the other probabilities underflow to 0 in fp32: the +eps terms carry the logs

# Pixel counts of the sweeps: 1, 255, 257: partial blocks; 262,144 / 262,145: at the 1024-block cap and one past; 263,144: part of the
# threads take the two-pixel trip of jsd_step_kernel; 524,288 / 524,291: cfg2's batch (two-pixel trips plus a ragged tail); 2,097,152 /
# 2,097,153: the 8192-block cap and one past; 1,638,400: cfg5 (16 x 320 x 320).


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _strides(P):
    b = max(1, (P + 255) // 256)
    return min(b, 1024) * 256, min(b, 8192) * 256


def _sentinels(P):
    s1, s2 = _strides(P)
    return torch.tensor(sorted({i for i in (0, 255, 256, s1 - 1, s1, 2 * s1, s2 - 1, s2, 2 * s2, P - 1) if 0 <= i < P}))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _check(got, ref, bound, what):
    """|got - ref| <= bound elementwise (float64 on the CPU); NaN anywhere in got fails."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} out of bound; first at flat {i}: got {got.reshape(-1)[i].item()!r} "
                             f"ref {ref.reshape(-1)[i].item()!r} bound {bound.reshape(-1)[i].item() if torch.is_tensor(bound) and bound.numel() > 1 else float(bound)!r}")


def _logits(g, P, C, scale=2.0):
    """Random logits; about a quarter of the pixels saturated (MARGIN_SAT) and a quarter underflowing (MARGIN_UFL) on a random class."""
    x = torch.randn(P, C, generator=g) * scale
    kind = torch.randint(0, 4, (P,), generator=g)
    top = torch.randint(0, C, (P,), generator=g)
    r = torch.arange(P)
    x[r, top] += torch.where(kind == 1, MARGIN_SAT, torch.where(kind == 2, MARGIN_UFL, 0.0))
    return x


def _sm64(x):
    """float64 softmax of fp32 logits and |x - max| (the argument of each expf, whose rounding scales the error of p)."""
    xd = x.double()
    return torch.softmax(xd, 1), (xd - xd.max(1, keepdim=True).values).abs()


def _ent_err(p, lq, spread, k):
    """Bound on |fp32 - exact| of H = -sum_c p_c log q_c (q = p + eps) when each p_c carries (k + |x_c - m|) U relative error.
    Per class: the p error enters as dp (|log q| + 1) (through the factor and through log q), logf adds 6U|log q| + U and the product
    and the C-term sum U each, so |dH| <= U sum_c (k + 6 + |x_c - m|) p_c (1 + |log q_c|).  A probability above 1 - 2^-26 is exactly 1 in
    fp32 (its softmax denominator rounds to 1): its term is exactly 0 there and -(1 - p) + O((1 - p)^2) in the reference."""
    one = p > 1 - 2.0 ** -26
    t = torch.where(one, 2 * (1 - p), U * (k + 6 + spread) * p * (1 + lq.abs()))
    return t.sum(-1)


# ------------------------------------------------------------------------------------------------------------------ cross entropy
CE_CASES = [  # P, C, ignored, accumulate
    (1, 2, False, False), (255, 3, True, False), (257, 4, False, True), (262144, 5, True, False), (262145, 6, False, True),
    (263144, 7, True, True), (524288, 8, False, False), (524291, 4, True, True), (2097152, 2, False, True), (2097153, 3, True, False),
    (1638400, 2, True, True),
]


@pytest.mark.parametrize("P,C,ignored,accumulate", CE_CASES)
def test_ce_at_scale(ops, P, C, ignored, accumulate):
    g = torch.Generator().manual_seed(P + 7 * C)
    x = torch.randn(P, C, generator=g) * 2          # background losses O(1) per pixel
    t = torch.randint(0, C, (P,), generator=g)
    if ignored:
        t[torch.rand(P, generator=g) < 0.25] = IGN
    # sentinels: target logit -D, the others 0 -> loss D + log(C - 1), each >= 1 % of the total (background losses are O(1) per pixel)
    sen = _sentinels(P)
    D = max(1e4, 0.1 * P)
    t[sen] = sen % C
    x[sen] = 0.0
    x[sen, t[sen]] = -D
    keep = t != IGN
    count = int(keep.sum())

    xd = x.double()
    ref = oracle.cross_entropy_2d(xd.t().reshape(1, C, P, 1), t.reshape(1, P, 1)).item()
    lse = torch.logsumexp(xd, 1)
    tc = t.clamp(max=C - 1)
    lpx = torch.where(keep, lse - xd.gather(1, tc[:, None])[:, 0], torch.zeros(()))
    amax = xd.abs().max(1).values
    assert (lpx[sen] >= 0.01 * lpx.sum()).all()
    # per pixel: max, C expf (argument x - m rounded: U |x - m| <= 2U max|x|), the C-term sum, logf, m + log s and - x_t:
    # |e_i| <= (C + 8) U (3 max|x| + log C + l_i + 1); the fp32 sum adds SUM_DEPTH U sum l_i; the division by the exact count U.
    e = torch.where(keep, (C + 8) * U * (3 * amax + math.log(C) + lpx + 1), torch.zeros(()))
    tol = (e.sum().item() + SUM_DEPTH * U * lpx.sum().item()) / count + 2 * U * ref
    assert lpx[sen].min().item() / count > 4 * tol                  # one lost sentinel is far outside the bound

    # gradient: g (p_c - [t == c]) with g = gscale gmul / count; p_c carries (C + 6 + |x_c - m|) U relative error, p - 1 rounds once,
    # g three times (gscale * gmul / count) and the product once: |d| err <= |g| ((C + 6 + |x - m|) U p + 4 U |p - 1_t|); the
    # accumulate rounds the sum once more (U |old + d|).  Ignored pixels are exactly 0 (exactly old).
    gscale, gmul = 0.61, 8.0
    gg = float(np.float32(gscale)) * gmul / count
    p, spread = _sm64(x)
    onehot = torch.nn.functional.one_hot(tc, C).double()
    dref = torch.where(keep[:, None], gg * (p - onehot), torch.zeros(()))
    bound = torch.where(keep[:, None], abs(gg) * ((C + 6 + spread) * U * p + 4 * U * (p - onehot).abs()) + 1e-30, torch.zeros(()))
    old = torch.randn(P, C, generator=g) if accumulate else None
    if accumulate:
        dref = dref + old.double()
        bound = bound + U * dref.abs()

    xg, tg = x.to(DEV), t.to(DEV)
    gs = torch.tensor([gscale], device=DEV)
    out = ops.ce_fwd(xg, tg, C, IGN)
    d1 = old.to(DEV) if accumulate else _nan(P, C)
    ops.ce_bwd(xg, tg, C, out[1:2], d1, gscale=gs, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    d2 = old.to(DEV) if accumulate else _nan(P, C)
    out2 = ops.ce_step(xg, tg, C, d2, gscale=gs, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    torch.cuda.synchronize()
    # (the count is summed in fp32: exact up to 2^24 pixels, far above any batch here)
    for o, what in ((out, "ce_fwd"), (out2, "ce_step")):
        assert o[1].item() == count, (what, o[1].item(), count)
        assert abs(o[0].item() - ref) <= tol, (what, o[0].item(), ref, tol)
    _check(d1, dref, bound, "ce_bwd")
    _check(d2, dref, bound, "ce_step gradient")


@pytest.mark.parametrize("P,C", [(1, 2), (257, 5), (262145, 4), (2097153, 8)])
def test_ce_all_targets_ignored(ops, P, C):
    """A batch whose every target is ignored: the loss is what the reference gives (0/0 = NaN), the count 0, the gradient exactly 0."""
    g = torch.Generator().manual_seed(5 + P)
    x = _logits(g, P, C)
    t = torch.full((P,), IGN, dtype=torch.int64)
    ref = oracle.cross_entropy_2d(x.double().t().reshape(1, C, P, 1), t.reshape(1, P, 1))
    assert math.isnan(ref.item())
    xg, tg = x.to(DEV), t.to(DEV)
    out = ops.ce_fwd(xg, tg, C, IGN)
    d1 = _nan(P, C)
    ops.ce_bwd(xg, tg, C, out[1:2], d1, ignore_index=IGN)
    d2 = _nan(P, C)
    out2 = ops.ce_step(xg, tg, C, d2, ignore_index=IGN)
    old = torch.randn(P, C, generator=g).to(DEV)
    d3 = old.clone()
    ops.ce_step(xg, tg, C, d3, ignore_index=IGN, accumulate=True)
    torch.cuda.synchronize()
    for o in (out, out2):
        assert math.isnan(o[0].item()) and o[1].item() == 0.0
    assert torch.equal(d1, torch.zeros_like(d1)) and torch.equal(d2, torch.zeros_like(d2))
    assert torch.equal(d3, old)


# ------------------------------------------------------------------------------------------------ softmax, entropy, argmax
SM_CASES = [(1, 2), (255, 3), (257, 8), (262144, 4), (262145, 5), (263144, 6), (524288, 7), (524291, 8), (2097152, 4),
            (2097153, 2), (2097153, 3), (1638400, 2)]


@pytest.mark.parametrize("P,C", SM_CASES)
def test_softmax_entropy_argmax_at_scale(ops, P, C):
    g = torch.Generator().manual_seed(3 * P + C)
    x = _logits(g, P, C)
    tie = torch.arange(P) % 5 == 3          # two classes share the maximum: argmax must give the first
    if C > 1:
        a = torch.randint(0, C - 1, (P,), generator=g)
        b = a + 1 + (torch.rand(P, generator=g) * (C - 1 - a)).long()
        r = torch.arange(P)[tie]
        mx = x[tie].max(1).values + 1.0
        x[r, a[tie]] = mx
        x[r, b[tie]] = mx
    xg = x.to(DEV)
    acc = P % 2 == 1
    probs = _nan(P, C)
    ops.call("dct_softmax_fwd", ops.ptr(xg), ops.ptr(probs), P, C, ops.stream())
    cls = torch.full((P,), -1, dtype=torch.int64, device=DEV)
    ops.call("dct_argmax", ops.ptr(xg), ops.ptr(cls), P, C, ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(cls.cpu(), x.argmax(1))          # exact, first index on ties

    # softmax: expf's argument x - m rounds (U |x - m| relative), expf, the C-term sum and the reciprocal ~(C + 2) U, the product U
    p64, spread = _sm64(x)
    _check(probs, p64, (C + 6 + spread) * U * p64 + TINY, "softmax_fwd")
    assert (probs == 0).any() or P < 256            # some probabilities underflowed (MARGIN_UFL rows)

    # from here on the inputs are the kernel's own fp32 probabilities
    pf = probs.cpu()
    pd = pf.double()
    # q = p + 1e-16 evaluated as the kernel does, in fp32 (for p > ~2e-9 it IS p there, while float64 keeps 1e-16 / p of it)
    lq = torch.log((pf + EPS_ENT).double())
    dprobs = torch.randn(P, C, generator=g)
    old = torch.randn(P, C, generator=g) if acc else None
    dl = old.to(DEV) if acc else _nan(P, C)
    ops.call("dct_softmax_bwd", ops.ptr(probs), ops.ptr(dprobs.to(DEV)), ops.ptr(dl), P, C, int(acc), ops.stream())
    ent = _nan(P)
    ops.call("dct_entropy_fwd", ops.ptr(probs), ops.ptr(ent), P, C, ops.stream())
    dmap = torch.randn(P, generator=g)
    dent = _nan(P, C)
    ops.call("dct_entropy_bwd", ops.ptr(probs), ops.ptr(dmap.to(DEV)), ops.ptr(dent), P, C, ops.stream())
    torch.cuda.synchronize()

    # softmax backward p (d - sum d p): the dot rounds C times on sum|d p|, d - dot once, the product once
    dd = dprobs.double()
    dot = (dd * pd).sum(1, keepdim=True)
    ref = pd * (dd - dot)
    bound = pd * (C * U * (dd * pd).abs().sum(1, keepdim=True) + 2 * U * (dd - dot).abs())
    if acc:
        ref = ref + old.double()
        bound = bound + U * ref.abs()
    _check(dl, ref, bound + TINY, "softmax_bwd")

    # entropy -sum p log q: exact inputs, so only logf (6U |log q| + U), the product and the C-term sum round
    h = -(pd * lq).sum(1)
    _check(ent, h, (C + 7) * U * (pd * (1 + lq.abs())).sum(1), "entropy_fwd")

    # entropy backward  dmap * -(log q + p / q): logf 6U |log q|, the division U, then the sum and the product by dmap round once
    # each on the whole: U (8 |log q| + 3 p / q) |dmap|
    q = (pf + EPS_ENT).double()
    dref = -dmap.double()[:, None] * (lq + pd / q)
    _check(dent, dref, dmap.double().abs()[:, None] * U * (8 * lq.abs() + 3 * pd / q + 2) + TINY, "entropy_bwd")


# ------------------------------------------------------------------------------------------------------------------------ JSD
JSD_CASES = [  # P, S, C, accumulate
    (1, 2, 2, False), (255, 3, 3, True), (257, 1, 4, False), (262144, 2, 4, False), (262145, 2, 2, True), (263144, 2, 4, True),
    (263144, 7, 7, False), (262145, 5, 6, True), (262145, 8, 8, False), (524288, 2, 4, False), (524291, 2, 2, True),
    (524291, 1, 3, False), (524291, 3, 5, True), (2097152, 2, 2, False), (2097153, 2, 4, True), (1638400, 3, 2, False),
]


def _jsd_inputs(g, P, S, C):
    """S models' logits: the background agrees (identical logits, saturated or underflowing: per-pixel JSD ~1e-15); every 97th pixel
    is random per model; the sentinels disagree maximally (model s sure of class s mod C)."""
    base = torch.randn(P, C, generator=g) * 2
    top = torch.randint(0, C, (P,), generator=g)
    r = torch.arange(P)
    base[r, top] += torch.where(torch.rand(P, generator=g) < 0.5, MARGIN_SAT, MARGIN_UFL)
    rnd = r % 97 == 13
    sen = _sentinels(P)
    xs = []
    for s in range(S):
        x = base.clone()
        x[rnd] = torch.randn(int(rnd.sum()), C, generator=g) * 2
        x[sen] = 0.0
        x[sen, s % C] = MARGIN_SAT
        xs.append(x)
    return xs, sen


def _jsd_ref(xs, C):
    """float64: per-pixel JSD (oracle.jsd_2d), its bound, and the logit gradients of the mean JSD (times 1 / P) with their bounds."""
    S, P = len(xs), xs[0].shape[0]
    ps, spreads = zip(*[_sm64(x) for x in xs])
    jmap = oracle.jsd_2d([p.t().reshape(1, C, P, 1) for p in ps]).reshape(P)
    mean = sum(ps) / S
    spread_max = torch.stack(spreads).max(0).values
    lq = [torch.log(p + EPS_ENT) for p in ps]
    lqm = torch.log(mean + EPS_ENT)
    hs = [-(p * l).sum(1) for p, l in zip(ps, lq)]
    hm = -(mean * lqm).sum(1)
    # per pixel: the S entropies (softmax error C + 6 + |x - m|), the mean's (S more roundings of the probabilities) and the final
    # hsum / S subtraction ((S + 2) U on the magnitudes)
    b = sum(_ent_err(p, l, sp, C + 6) for p, l, sp in zip(ps, lq, spreads)) / S + _ent_err(mean, lqm, spread_max, C + 6 + S) \
        + (S + 2) * U * (hm + sum(hs) / S)

    def dent(p, l):
        return -(l + p / (p + EPS_ENT))
    dm = dent(mean, lqm)
    grads, gbounds = [], []
    for p, l, sp in zip(ps, lq, spreads):
        d = (dm - dent(p, l)) / S
        dot = (d * p).sum(1, keepdim=True)
        grads.append(p * (d - dot) / P)
        # dent(mean) - dent(p): each log carries (C + 8 + S + |x - m|) U relative error of its argument plus 6U |log q|; times 1/S;
        # the dot adds C U sum|d p| and the errors of the d it sums; p (d - dot) adds p's own error times |d - dot|
        E = U * (C + 12 + S + spread_max) * (2 + lqm.abs() + l.abs()) / S
        inner = E + (p * E).sum(1, keepdim=True) + C * U * (p * d.abs()).sum(1, keepdim=True)
        gbounds.append((p * inner + (C + 6 + sp) * U * p * (d - dot).abs()) / P + 4 * U * (p * (d - dot)).abs() / P)
    return jmap, b, grads, gbounds, ps


@pytest.mark.parametrize("P,S,C,accumulate", JSD_CASES)
def test_jsd_at_scale(ops, P, S, C, accumulate):
    g = torch.Generator().manual_seed(11 * P + 3 * S + C)
    xs, sen = _jsd_inputs(g, P, S, C)
    jmap, b, grads, gbounds, ps = _jsd_ref(xs, C)
    ref = jmap.mean().item()
    # the kernels' mean: per-pixel bounds, the fp32 sum of P terms (SUM_DEPTH U sum|j|), the division by P
    tol = (b.sum().item() + SUM_DEPTH * U * jmap.abs().sum().item()) / P + 2 * U * abs(ref)
    if S >= 2:
        assert jmap[sen].min().item() / P > 4 * tol                 # one lost sentinel is far outside the bound
    else:
        assert ref == 0.0                                           # S = 1: nothing to disagree with
    if P <= 257:                                                    # the analytic gradient is the oracle's
        ls = [x.double().t().reshape(1, C, P, 1).requires_grad_(True) for x in xs]
        jj = oracle.jsd_2d([oracle.softmax_channels(l) for l in ls]).mean()
        for gr, want in zip(torch.autograd.grad(jj, ls), grads):
            np.testing.assert_allclose(gr.reshape(C, P).t().numpy(), want.numpy(), rtol=1e-9, atol=1e-15)

    gscale, gmul = 0.37, 4.0
    gg = float(np.float32(gscale)) * gmul
    olds = [torch.randn(P, C, generator=g) for _ in range(S)] if accumulate else None
    refs = [gg * gr + (olds[s].double() if accumulate else 0) for s, gr in enumerate(grads)]
    # g = gscale * gmul / P rounds 3 times (folded into 4U |o| above); the accumulate's add once more
    bnds = [gg * gb + (U * r.abs() if accumulate else 0) + 1e-30 for gb, r in zip(gbounds, refs)]

    xg = [x.to(DEV) for x in xs]
    gs = torch.tensor([gscale], device=DEV)
    v = ops.jsd_logits_fwd(xg, C)
    d1 = [olds[s].to(DEV) if accumulate else _nan(P, C) for s in range(S)]
    ops.jsd_logits_bwd(xg, C, d1, gscale=gs, gmul=gmul, accumulate=accumulate)
    d2 = [olds[s].to(DEV) if accumulate else _nan(P, C) for s in range(S)]
    pr = [_nan(P, C) for _ in range(S)]
    v2 = torch.empty(1, device=DEV)
    ws = ops._loss_ws(DEV)
    ops.call("dct_jsd_logits_step", ops._ptr_array(xg), S, P, C, ops.ptr(v2), ops._ptr_array(pr), ops.ptr(gs), gmul, ops._ptr_array(d2),
             int(accumulate), ops.ptr(ws), ws.numel(), ops.stream())
    torch.cuda.synchronize()
    for val, what in ((v, "jsd_logits_fwd"), (v2, "jsd_logits_step")):
        assert abs(val.item() - ref) <= tol, (what, val.item(), ref, tol)
    for s in range(S):
        _check(d1[s], refs[s], bnds[s], f"jsd_logits_bwd model {s}")
        _check(d2[s], refs[s], bnds[s], f"jsd_logits_step gradient model {s}")
        _, sp = _sm64(xs[s])
        _check(pr[s], ps[s], (C + 6 + sp) * U * ps[s] + TINY, f"jsd_logits_step softmax model {s}")

    # the probability-map forms, from the kernel's own fp32 probabilities; p + 1e-16 in fp32 as the kernel forms it
    pf = [p.cpu() for p in pr]
    pd = [p.double() for p in pf]
    mean32 = sum(pd) / S
    lq = [torch.log((p + EPS_ENT).double()) for p in pf]
    lqm = torch.log((mean32.float() + EPS_ENT).double())
    zero = torch.zeros(P, C, dtype=torch.float64)
    jm = -(mean32 * lqm).sum(1) + sum((p * l).sum(1) for p, l in zip(pd, lq)) / S
    bm = sum(_ent_err(p, l, zero, 1) for p, l in zip(pd, lq)) / S + _ent_err(mean32, lqm, zero, S + 2) \
        + (S + 2) * U * (-(mean32 * lqm).sum(1) - sum((p * l).sum(1) for p, l in zip(pd, lq)) / S)
    dmap = torch.randn(P, generator=g)
    jmg = _nan(P)
    ops.call("dct_jsd_map_fwd", ops._ptr_array(pr), S, ops.ptr(jmg), P, C, ops.stream())
    dps = [_nan(P, C) for _ in range(S)]
    ops.call("dct_jsd_map_bwd", ops._ptr_array(pr), S, ops.ptr(dmap.to(DEV)), ops._ptr_array(dps), P, C, ops.stream())
    torch.cuda.synchronize()
    _check(jmg, jm, bm, "jsd_map_fwd")
    dm = -(lqm + mean32 / (mean32.float() + EPS_ENT).double())
    for s in range(S):
        dp = -(lq[s] + pd[s] / (pf[s] + EPS_ENT).double())
        ref_s = dmap.double()[:, None] * (dm - dp) / S
        # the fp32 mean carries (S + 1) U relative error; each log 6U |log q| + U; dividing, subtracting, scaling: 3U on the result
        E = U * (S + 10) * (2 + lqm.abs() + lq[s].abs()) / S
        _check(dps[s], ref_s, dmap.double().abs()[:, None] * E + 3 * U * ref_s.abs() + TINY, f"jsd_map_bwd model {s}")


# ------------------------------------------------------------------------------------------------------------------------- KL
KL_CASES = [(1, 3), (255, 2), (257, 5), (262144, 6), (262145, 7), (263144, 8), (524291, 4), (2097152, 3), (2097153, 2), (1638400, 2)]


def _kl_ref(xp, xy, C, gg):
    """float64: per-pixel KL(y || p) of the softmaxes of fp32 logits (oracle.kl_divergence_2d), its bound, the gradient ``gg`` * d sum_pix KL /
    d p-logits and its bound, and the two softmaxes."""
    P = xp.shape[0]
    same = (xp == xy).all(1)
    p, sp = _sm64(xp)
    y, sy = _sm64(xy)
    kmap = oracle.kl_divergence_2d(p.t().reshape(1, C, P, 1), y.t().reshape(1, C, P, 1), eps=EPS_KL).reshape(P)
    lqp, lqy = torch.log(p + EPS_KL), torch.log(y + EPS_KL)
    # per pixel (differing inputs): y and p carry (C + 6 + |x - m|) U relative error, each logf 6U|log q| + U, the products and the
    # two C-term sums U each, the subtraction U on the magnitudes; identical inputs give exactly 0 on both sides
    b = torch.where(same, torch.zeros(()), U * ((C + 12 + sy + sp) * y * (2 + lqy.abs() + lqp.abs())).sum(1))
    # gradient of the mean w.r.t. the p logits: d = -y / (p + eps); o = g p (d - sum d p)
    d = -y / (p + EPS_KL)
    dot = (d * p).sum(1, keepdim=True)
    gref = gg * p * (d - dot)
    # d: y's and p's errors and the division, (2C + 14 + |xy - m| + |xp - m|) U relative; the dot C U sum|d p| more
    rel = (2 * C + 14 + sy + sp) * U
    gb = abs(gg) * p * (rel * d.abs() + (rel * (d * p).abs()).sum(1, keepdim=True) + C * U * (d * p).abs().sum(1, keepdim=True)) \
        + (C + 6 + sp) * U * gref.abs() + 4 * U * gref.abs() + 1e-30
    return kmap, b, gref, gb, p, y


@pytest.mark.parametrize("P,C", KL_CASES)
def test_kl_at_scale(ops, P, C):
    """KL(y || p): the background has p and y from identical logits (per-pixel KL exactly 0 in both arithmetics), every 97th pixel
    differs, and the sentinels are sure of different classes (KL ~ -log(eps) = 23: the eps term carries it)."""
    g = torch.Generator().manual_seed(13 * P + C)
    xp = _logits(g, P, C)
    xy = xp.clone()
    r = torch.arange(P)
    rnd = r % 97 == 13
    xy[rnd] = torch.randn(int(rnd.sum()), C, generator=g) * 2
    sen = _sentinels(P)
    xp[sen] = 0.0
    xy[sen] = 0.0
    xp[sen, 0] = MARGIN_SAT
    xy[sen, 1] = MARGIN_SAT
    same = (xp == xy).all(1)

    gscale, gmul = 0.5, 2.0
    gg = float(np.float32(gscale)) * gmul / P
    kmap, b, gref, gb, p, y = _kl_ref(xp, xy, C, gg)
    ref = kmap.mean().item()
    tol = (b.sum().item() + SUM_DEPTH * U * kmap.abs().sum().item()) / P + 2 * U * abs(ref)
    assert kmap[sen].min().item() / P > 4 * tol and (kmap[same] == 0).all()

    xpg, xyg = xp.to(DEV), xy.to(DEV)
    gs = torch.tensor([gscale], device=DEV)
    v = ops.kl_logits_fwd(xpg, xyg, C, eps=1e-10)
    dk = _nan(P, C)
    ops.kl_logits_bwd(xpg, xyg, C, dk, gscale=gs, gmul=gmul, eps=1e-10)
    old = torch.randn(P, C, generator=g)
    dk2 = old.to(DEV)
    ops.kl_logits_bwd(xpg, xyg, C, dk2, gscale=gs, gmul=gmul, eps=1e-10, accumulate=True)
    torch.cuda.synchronize()
    assert abs(v.item() - ref) <= tol, (v.item(), ref, tol)
    _check(dk, gref, gb, "kl_logits_bwd")
    _check(dk2, gref + old.double(), gb + U * (gref + old.double()).abs(), "kl_logits_bwd accumulate")

    # map forms on fp32 probabilities (the reference's rounded to fp32); p + eps in fp32 as the kernel forms it
    pf, yf = p.float(), y.float()
    pd, yd = pf.double(), yf.double()
    lp32, ly32 = torch.log((pf + EPS_KL).double()), torch.log((yf + EPS_KL).double())
    km = (yd * ly32).sum(1) - (yd * lp32).sum(1)
    same32 = (pf == yf).all(1)
    bm = torch.where(same32, torch.zeros(()), (C + 7) * U * (yd * (2 + ly32.abs() + lp32.abs())).sum(1))
    pg, yg = pf.to(DEV), yf.to(DEV)
    kmg = _nan(P)
    ops.call("dct_kl_map_fwd", ops.ptr(pg), ops.ptr(yg), ops.ptr(kmg), P, C, EPS_KL, ops.stream())
    dmap = torch.randn(P, generator=g)
    dpg = _nan(P, C)
    ops.call("dct_kl_map_bwd", ops.ptr(pg), ops.ptr(yg), ops.ptr(dmap.to(DEV)), ops.ptr(dpg), P, C, EPS_KL, ops.stream())
    torch.cuda.synchronize()
    _check(kmg, km, bm, "kl_map_fwd")
    dref = dmap.double()[:, None] * (-yd / (pf + EPS_KL).double())
    _check(dpg, dref, 3 * U * dref.abs() + TINY, "kl_map_bwd")


# ---------------------------------------------------------------------------------------------------------------------- Dice
@pytest.mark.parametrize("B,H,C,method", [(1, 256, 2, "2d"), (8, 256, 4, "3d"), (16, 320, 8, "2d"), (8, 320, 2, "3d"),
                                          (16, 256, 4, "3d"), (1, 320, 8, "2d")])
def test_dice_counts_and_meter_at_slice_size(ops, B, H, C, method):
    """Counts of dct_dice_counts (64 blocks per image: several trips per thread at slice size) exactly equal the oracle's, argmax ties
    resolve to the first class, a class absent from prediction and label scores 1 by the smoothing alone, and DiceMeter's running
    report equals the oracle's Dice rows."""
    from dct_amd.metrics import DiceMeter
    g = torch.Generator().manual_seed(B * H + C)
    meter = DiceMeter(method=method, C=C)
    rows = []
    for k in range(2):
        x = torch.randn(B, C, H, H, generator=g)
        gt = torch.randint(0, C, (B, 1, H, H), generator=g)
        # ties: on every 7th pixel two classes share the maximum; the label is one of the two
        flat = x.permute(0, 2, 3, 1).reshape(-1, C)
        lab = gt.reshape(-1)
        n = flat.shape[0]
        idx = torch.arange(n)[torch.arange(n) % 7 == 2]
        a = torch.randint(0, C - 1, (len(idx),), generator=g)
        b = a + 1
        mx = flat[idx].max(1).values + 0.5
        flat[idx, a] = mx
        flat[idx, b] = mx
        lab[idx] = torch.where(torch.rand(len(idx), generator=g) < 0.5, a, b)
        x = flat.reshape(B, H, H, C).permute(0, 3, 1, 2).contiguous()
        gt = lab.reshape(B, 1, H, H)
        # class C - 1 absent from image 0 in prediction and label
        gt[0][gt[0] == C - 1] = 0
        x[0, C - 1] = -1e4
        ohp, ohg = _one_hots(x, gt)
        inter, psum, gsum = (ohp & ohg).sum((2, 3)), ohp.sum((2, 3)), ohg.sum((2, 3))
        ci, cp, cg = ops.dice_counts(x.permute(0, 2, 3, 1).contiguous().reshape(B, H * H, C).to(DEV), gt.reshape(B, -1).to(DEV), B, C)
        torch.cuda.synchronize()
        assert torch.equal(ci.cpu(), inter.int()) and torch.equal(cp.cpu(), psum.int()) and torch.equal(cg.cpu(), gsum.int())
        d = oracle.dice_2d(x, gt) if method == "2d" else oracle.dice_3d(x, gt)[None]
        if method == "2d":
            assert d[0, C - 1].item() == 1.0 and inter[0, C - 1] == 0 and psum[0, C - 1] == 0
        rows.append(d.double())
        meter.add(x.to(DEV), gt.to(DEV))
        # the meter's rows: (2 inter + smooth) / (sizes + smooth) in fp32 from exact integer counts -- the oracle's own fp32 formula;
        # allow one rounding of the division either way
        np.testing.assert_allclose(meter.diceLog[-1].cpu().numpy(), d.numpy(), rtol=2 * U, atol=0)
    log = torch.cat(rows)
    (mm, ms), (cm, cs) = meter.value()
    rep = log.mean(1)
    # means / stds of <= 32 rows accumulated in float64 and reported in fp32: the rows' own 2U, the final rounding U; the variance's
    # float64 cancellation (sum v^2 - n mean^2) costs ~1e-16 n / var, nothing here.  The report mean of a row is summed over the C
    # classes in fp32 by the kernel ((C + 1) U of the row), which moves a standard deviation by up to twice that absolutely.
    top = log.abs().max().item()
    np.testing.assert_allclose(cm.numpy(), log.mean(0).numpy(), rtol=4 * U, atol=0)
    np.testing.assert_allclose(cs.numpy(), log.std(0).numpy(), rtol=4 * U, atol=4 * U * top)
    np.testing.assert_allclose(float(mm), rep.mean().item(), rtol=(C + 3) * U, atol=0)
    np.testing.assert_allclose(float(ms), rep.std().item(), rtol=4 * U, atol=2 * (C + 3) * U * top)


# ---------------------------------------------------------------------------------------------------------------------- Adam
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def _unet_total():
    from dct_amd.arch import get_arch
    return get_arch("unet", {"num_classes": 4}).flat_params.total


def _dev_state(t, lr, base, length):
    """dct_adam_flat_dev's state {t, lr, table base, table length} and FusedAdam's table: {1 - b1^t, sqrt(1 - b2^t)} in float64 as the
    host computes them, for t = base + 1 ... base + length."""
    table = torch.tensor([(1.0 - B1 ** k, math.sqrt(1.0 - B2 ** k)) for k in range(base + 1, base + 1 + length)], dtype=torch.float64)
    state = torch.tensor([float(t), lr, float(base), float(length)], dtype=torch.float64)
    return state.to(DEV), table.to(DEV)


@pytest.mark.parametrize("n,shadow,grad_scale,wd", [
    (1, False, 1.0, 0.0), (2, True, 1.0, 1e-4), (3, False, 1 / 1024, 1e-4), (5, True, 1 / 1024, 0.0),
    (100003, True, 1.0, 1e-4), (100003, False, 1 / 1024, 0.0), ("unet", True, 1.0, 1e-4), ("unet", False, 1 / 1024, 1e-4),
])
def test_adam_flat_dev_table_path_is_bit_identical(ops, n, shadow, grad_scale, wd):
    """dct_adam_flat_dev, step count / lr / table on the device, gives bit for bit what dct_adam_flat gives when fed the host's
    lr / (1 - b1^t) and sqrt(1 - b2^t) (the promise of adam_kernel's comment) -- through a learning-rate change, the tail-only sizes
    (n < 4, n = 5), several grid-stride trips (the UNet's flat buffer), the bf16 shadow, a loss-scale and weight decay."""
    if n == "unet":
        n = _unet_total()
    g = torch.Generator(device=DEV).manual_seed(17)
    p0 = torch.randn(n, device=DEV, generator=g)
    pa, pb = p0.clone(), p0.clone()
    ma, mb, va, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    sa = torch.empty(n + 8, dtype=torch.bfloat16, device=DEV)[:n] if shadow else None
    sb = torch.empty(n + 8, dtype=torch.bfloat16, device=DEV)[:n] if shadow else None
    lr = 1e-3
    state, table = _dev_state(0, lr, 0, 8)
    for t in range(1, 6):
        if t == 3:
            lr = 3e-4
            state[1:2].fill_(lr)
        gr = torch.randn(n, device=DEV, generator=g) * 0.1 / grad_scale
        ops.adam_flat(pa, gr, ma, va, lr / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t), B1, B2, ADAM_EPS, wd, bf16_shadow=sa,
                      grad_scale=grad_scale)
        ops.adam_flat_dev(pb, gr, mb, vb, state, table, B1, B2, ADAM_EPS, wd, bf16_shadow=sb, grad_scale=grad_scale)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), f"step {t}"
        assert not torch.equal(pa, p0)
        if shadow:
            assert torch.equal(sa, sb) and torch.equal(sb, pb.to(torch.bfloat16))
    assert state[0].item() == 5.0


def _adam64(p, gr, m, v, t, lr, wd):
    """One Adam step in float64 (oracle.adam_reference_step) from the kernel's fp32 state; returns (p, m, v)."""
    p, m, v = p.double().cpu(), m.double().cpu(), v.double().cpu()
    oracle.adam_reference_step(p, gr.double().cpu(), m, v, t, lr=lr, beta1=B1, beta2=B2, eps=ADAM_EPS, weight_decay=wd)
    return p, m, v


def _adam_close(got, want, what):
    # test_adam_flat's tolerances.  Each comparison is ONE fp32 step from the state the reference starts from too: the kernel rounds
    # g + wd p, the lerp, v b2 + (1 - b2) g^2, the sqrt, the divisions and the final subtraction once each (<= 10 U ~ 6e-7 relative of
    # the largest term), inside rtol 2e-6; near-zero p / m the absolute parts (update ~ lr: 10 U lr ~ 6e-10; m: 2U 0.1 |g| ~ 4e-9) sit
    # inside atol 2e-8 / 1e-8.
    pk, mk, vk = (x.cpu().numpy() for x in got)
    pr, mr, vr = (x.numpy() for x in want)
    np.testing.assert_allclose(pk, pr, rtol=2e-6, atol=2e-8, err_msg=what + " p")
    np.testing.assert_allclose(mk, mr, rtol=2e-6, atol=1e-8, err_msg=what + " m")
    np.testing.assert_allclose(vk, vr, rtol=2e-6, atol=1e-12, err_msg=what + " v")


@pytest.mark.parametrize("n", [5, 100003])
def test_adam_flat_dev_steps_past_the_table(ops, n):
    """A device table of 4 steps and 10 steps with no host scalar changing between them: steps 5 - 10 take the kernel's own float64
    pow() fallback; every step matches a float64 Adam step from the same state."""
    g = torch.Generator(device=DEV).manual_seed(23)
    p = torch.randn(n, device=DEV, generator=g)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lr, wd = 1e-3, 1e-4
    state, table = _dev_state(0, lr, 0, 4)
    for t in range(1, 11):
        gr = torch.randn(n, device=DEV, generator=g) * 0.1
        want = _adam64(p, gr, m, v, t, lr, wd)
        ops.adam_flat_dev(p, gr, m, v, state, table, B1, B2, ADAM_EPS, wd)
        torch.cuda.synchronize()
        _adam_close((p, m, v), want, f"step {t} ({'table' if t <= 4 else 'fallback'})")
    assert state[0].item() == 10.0


def test_fused_adam_against_torch_adam_in_float64(ops, monkeypatch):
    """FusedAdam with a 4-step table over 30 steps against torch.optim.Adam in float64 on the same gradients: table rebuilds in place
    every 4 steps, a learning-rate change through refresh_lr, three graph-style replays of the step's kernel (the device counter runs
    past the table: pow fallback) followed by note_replayed_steps, another lr change (rebuild in place at the new base).  Each step is
    compared from the state the fused optimizer reached (one fp32 step against one float64 step)."""
    from dct_amd.arch.flat import FlatParams
    from dct_amd.optim import FusedAdam
    monkeypatch.setattr(FusedAdam, "TABLE_STEPS", 4)
    torch.manual_seed(29)
    net = torch.nn.Sequential(torch.nn.Linear(37, 29), torch.nn.Linear(29, 5)).to(DEV)
    flat = FlatParams(list(net.parameters()))
    flat.ensure()
    params = list(net.parameters())
    opt = FusedAdam(params, lr=1e-3, weight_decay=1e-4, flat=flat)
    refp = [torch.nn.Parameter(p.detach().double().cpu()) for p in params]
    ref = torch.optim.Adam(refp, lr=1e-3, weight_decay=1e-4)
    g = torch.Generator(device=DEV).manual_seed(31)
    addrs = None

    def grads():
        flat.ensure_grads()
        flat.gflat.copy_(torch.randn(flat.total, device=DEV, generator=g) * 0.1)
        for p, rp in zip(params, refp):
            rp.grad = p.grad.detach().double().cpu()

    def sync_ref():                   # the reference starts each step from the fused optimizer's fp32 state
        with torch.no_grad():
            for p, rp in zip(params, refp):
                rp.copy_(p.detach().double().cpu())
                if rp in ref.state:
                    ref.state[rp]["exp_avg"].copy_(opt.state[p]["exp_avg"].double().cpu())
                    ref.state[rp]["exp_avg_sq"].copy_(opt.state[p]["exp_avg_sq"].double().cpu())

    def compare(what):
        torch.cuda.synchronize()
        for p, rp in zip(params, refp):
            st, rs = opt.state[p], ref.state[rp]
            _adam_close((p.detach(), st["exp_avg"], st["exp_avg_sq"]), (rp.detach(), rs["exp_avg"], rs["exp_avg_sq"]), what)

    step = 0
    while step < 30:
        if step == 10:
            for grp in (opt.param_groups[0], ref.param_groups[0]):
                grp["lr"] = 5e-4
            opt.refresh_lr()
        if step == 18:
            # three replays of the captured step: the same kernel on the same device state, the host count untouched
            b1, b2 = opt.param_groups[0]["betas"]
            for _ in range(3):
                grads()
                sync_ref()
                ops.adam_flat_dev(flat.flat, flat.gflat, opt._m, opt._v, opt._dev_state, opt._dev_table, b1, b2, ADAM_EPS, 1e-4)
                ref.step()
                step += 1
                compare(f"replay to step {step}")
            opt.note_replayed_steps(3)
            addrs = (opt._dev_state.data_ptr(), opt._dev_table.data_ptr())
            for grp in (opt.param_groups[0], ref.param_groups[0]):
                grp["lr"] = 2e-4
            opt.refresh_lr()
            assert (opt._dev_state.data_ptr(), opt._dev_table.data_ptr()) == addrs      # rebuilt in place: graphs hold these
            assert opt._table_base == step and opt._dev_state[2].item() == step
        grads()
        sync_ref()
        opt.step()
        ref.step()
        step += 1
        compare(f"step {step}")
        assert opt._dev_state[0].item() == step == opt._steps
    assert addrs == (opt._dev_state.data_ptr(), opt._dev_table.data_ptr())
