"""The top-k cross entropy kernels (``dct_topk_ce_*``, include/dct.h) and ``TopKCrossEntropyLoss2d`` on top of them.

What is exact is held exactly, against the device's OWN stored map brought to the CPU: the map is ``dct_ce_map_fwd``'s bit for bit;
``counts4`` = {K, N, n_gt, n_eq} and tau are those of ``torch.kthvalue`` on that map; pixels below tau and uncounted pixels get a gradient
of exactly 0 (exactly the old value under accumulate); ``_step`` is ``_fwd`` + ``_bwd`` and a second run is the first, bit for bit.

What is rounded is held to derived bounds (U: the fp32 unit roundoff, SUM_DEPTH: the levels of the kernels' reduction, e_i: the per-pixel
map bound of ``focal_ref.ce_bounds``, tests/test_weighted_ce_gpu.py's):
  * value against the float64 top-k mean of the device's map:  (SUM_DEPTH U sum|v_i| + 3 U |sum|) / K over the K selected entries;
  * value against the float64 reference end to end:  max_i e_i + the summation term -- the top-k mean is 1-Lipschitz in the sup norm of
    v.  Being monotone in every entry it also lies between the top-k means of v - e and v + e, which is held too (and is tighter: the
    sentinels' e_i, with logits of 1e4 and more, do not enter unless they are selected);
  * gradient against the device's own selection: a_i from the device's map by the header's tie rule, then (g a_i / K) w_i (p - y) of the
    float64 reference within ``ce_bounds``' gradient bound with 6 + 3 roundings on the factor: gscale * gmul / (float) K as for the
    weighted mean, the two conversions and the division of the tie share, and its product with g;
  * gradient against the float64 reference's autograd through ``torch.topk``: on every counted pixel that is on the same side of tau in
    every map within e of the reference's (v_i - e_i above the K-th largest of v + e, or v_i + e_i below that of v - e).  That is every
    pixel with |v_i - tau| > 2 max e and more; the pixels left out may number at most max(8, 0.01 % of N) where nothing is planted at
    tau (a planted tie group, cluster or the zero-weight class's tie at 0 under k = 100 sit there by design).

Pixel counts: 1, 255, 257 (partial blocks), 262,145 (one past the 1024 blocks of the histogram launches: a second trip) and 2,097,153
(one past the 8192 blocks of the backward kernel); C: 2, 3, 4, 8; k: 0.1, 1, 10, 33.3, 50, 100, spread over the cases; the plants of
tests/topk_ref.py by name."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_loss_kernels_scale_gpu import DEV, IGN, SUM_DEPTH, U, _check, _nan, _sentinels  # noqa: E402

import focal_ref  # noqa: E402
import topk_ref as R  # noqa: E402

assert (R.U, R.SUM_DEPTH, R.IGN) == (U, SUM_DEPTH, IGN)

CASES = [  # P, C, k, accumulate, stray targets, weighted (else weight = NULL), plant
    (1, 2, 10.0, False, False, True, None), (1, 3, 100.0, True, False, False, None),
    (255, 3, 33.3, False, False, True, None), (255, 8, 1.0, True, False, False, None), (255, 4, 50.0, False, False, True, "same"),
    (257, 4, 10.0, True, True, True, "tie"), (257, 2, 0.1, False, False, True, None), (257, 3, 100.0, False, True, True, None),
    (262145, 2, 10.0, True, False, False, "cluster"), (262145, 4, 10.0, False, False, True, None), (262145, 8, 1.0, False, True, False, "tie"),
    (262145, 3, 100.0, True, False, True, None), (262145, 3, 33.3, False, False, True, "tie"), (262145, 2, 50.0, False, True, True, None),
    (2097153, 3, 10.0, False, False, True, None), (2097153, 2, 0.1, True, False, False, None), (2097153, 4, 1.0, False, True, True, None),
    (2097153, 8, 10.0, True, False, False, None),
    # (with these every pixel count above has run at every C of 2, 3, 4, 8)
    (1, 4, 33.3, False, False, True, None), (1, 8, 0.1, True, False, False, None), (255, 2, 10.0, True, True, False, None),
    (257, 8, 33.3, False, False, True, "tie"),
]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a.cpu(), b.cpu())


def _ratio(got, ref, bound):
    return ((got.detach().cpu().double() - ref).abs() / bound.clamp(min=1e-300)).max().item()


@pytest.mark.parametrize("P,C,k,accumulate,stray,weighted,plant", CASES)
def test_topk_ce_at_scale(ops, P, C, k, accumulate, stray, weighted, plant):
    w = focal_ref.weights(C) if weighted else torch.ones(C)
    g, x, t, t_ref, sen, idx = R.inputs(P, C, w, stray, seed=P + 7 * C + int(k), plant=plant, k=k)
    assert torch.equal(sen, _sentinels(P))
    keep = t_ref != IGN
    if plant == "cluster":
        k = R.k_for(int(keep.sum()), len(sen) + R.CLUSTER // 2)          # tau inside the cluster (the sentinels lie above it)
    r = R.Ref(x, t_ref, w, C, k)
    ref = r.value.item()
    gscale, gmul = 0.61, 8.0
    gg = float(np.float32(gscale)) * gmul
    old = torch.randn(P, C, generator=g) if accumulate else None
    xg, tg = x.to(DEV), t.to(DEV)
    wg = w.to(DEV) if weighted else None
    gs = torch.tensor([gscale], device=DEV)

    def fresh():
        return old.to(DEV) if accumulate else _nan(P, C)
    kw = dict(weight=wg, gscale=gs, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    out2, counts4, vmap = ops.topk_ce_fwd(xg, tg, C, wg, k, IGN)
    d1 = ops.topk_ce_bwd(xg, tg, C, vmap, out2, counts4, fresh(), **kw)
    runs = []
    for _ in range(2):
        d2 = fresh()
        runs.append(ops.topk_ce_step(xg, tg, C, d2, k_percent=k, **kw) + (d2,))
    m = ops.ce_map_fwd(xg, tg, C, wg, IGN)
    torch.cuda.synchronize()

    # the map, and bit equality: the step against the two calls, run against run
    assert _same_bits(vmap, m)
    for o2, c4, vm2, d2 in runs:
        assert _same_bits(o2, out2) and _same_bits(c4, counts4) and _same_bits(vm2, vmap) and _same_bits(d2, d1)

    # the selection, exactly, on the device's own map
    vm = vmap.cpu()
    K, N, tau, n_gt, n_eq, a = R.selection(vm, keep, k)
    assert (K, N) == (r.K, r.N)
    assert counts4.tolist() == [K, N, n_gt, n_eq], (counts4.tolist(), [K, N, n_gt, n_eq])
    assert out2[1].item() == tau.item(), (out2[1].item(), tau.item())

    # the value: against the float64 top-k mean of the device's map, then against the reference end to end
    top = torch.topk(vm[keep].double(), K).values
    mean_dev = top.sum().item() / K
    tol1 = (SUM_DEPTH * U * top.abs().sum().item() + 3 * U * abs(top.sum().item())) / K
    got = out2[0].item()
    sum_tol = r.sum_tol(r.top_abs, K) + 3 * U * abs(ref)
    e_max = r.e[keep].max().item()
    tau_lo, tau_hi, mean_lo, mean_hi = r.bracket()
    print(f"topk P={P} C={C} k={k:.4g} {'weighted' if weighted else 'NULL'} {plant}: K={K} N={N} n_gt={n_gt} n_eq={n_eq} tau={tau.item()!r} "
          f"value {got!r}; vs own map err {abs(got - mean_dev):.3e} of {tol1:.3e}; vs float64 err {abs(got - ref):.3e} of "
          f"{e_max + sum_tol:.3e} (bracket [{mean_lo - sum_tol!r}, {mean_hi + sum_tol!r}])")
    assert abs(got - mean_dev) <= tol1, (got, mean_dev, tol1)
    assert abs(got - ref) <= e_max + sum_tol, (got, ref, e_max, sum_tol)
    slack = SUM_DEPTH * U * e_max                           # (the summation term of a map that is e above the reference's)
    assert mean_lo - sum_tol - slack <= got <= mean_hi + sum_tol + slack, (mean_lo, got, mean_hi, sum_tol)

    # the gradient against the device's own selection
    gfac = gg * a / K
    want = gfac[:, None] * r.r.closed_form()
    bound = r.grad_bound(gfac, 9)
    if accumulate:
        want = want + old.double()
        bound = bound + U * want.abs()
    print(f"  gradient vs own selection: max err / bound {_ratio(d1, want, bound):.3f}")
    _check(d1, want, bound, "topk_ce_bwd")
    d1c = d1.cpu()
    gone = ~keep | (a == 0)
    if gone.any():
        assert torch.equal(d1c[gone], old[gone] if accumulate else torch.zeros(int(gone.sum()), C))
    assert bool(torch.isfinite(d1c).all())

    # the gradient against the float64 reference, where every map within e of the reference's selects alike
    v64, e = r.v, r.e
    above, below = keep & (v64 - e > tau_hi), keep & (v64 + e < tau_lo)
    safe = above | below
    left_out = int((keep & ~safe).sum())
    assert not (keep & ~safe & ((v64 - r.tau).abs() > 2 * e_max)).any()           # every pixel beyond 2 max e of tau is held
    at_tau_by_design = plant is not None or (weighted and k == 100.0) or N <= 1
    print(f"  vs float64 autograd: {left_out} counted pixels left out (cap {max(8, 1e-4 * N):.0f}{', planted at tau' if at_tau_by_design else ''})")
    if not at_tau_by_design:
        assert left_out <= max(8, 1e-4 * N), (left_out, N)
    dref = r.grad(gg, old)
    rbound = r.grad_bound(gg / K * above.double(), 9)
    if accumulate:
        rbound = rbound + U * dref.abs()
    _check(d1c[safe], dref[safe], rbound[safe], "topk_ce_bwd against autograd")
    assert above.sum() <= K <= P - below.sum()

    # the plants, by name
    if plant in ("tie", "same"):
        assert n_eq == len(idx) and 0 < K - n_gt <= n_eq and (plant == "same" or K - n_gt < n_eq)
        assert bool((a[idx] == (K - n_gt) / n_eq).all())
        if not accumulate:
            rows = _bits(d1)[idx]
            assert bool((rows == rows[0]).all())             # every member of the group gets the same share
        assert bool((d1c[idx] - (old[idx] if accumulate else 0)).abs().sum() > 0)
    if plant == "same":
        assert n_gt == 0 and n_eq == N == P
    if plant == "cluster":
        D = 1000.0 + torch.arange(R.CLUSTER, dtype=torch.float64) * R.ULP_1000
        assert torch.equal(vm[idx].double(), D)              # v_j = D_j exactly: the last pass's digits alone tell them apart
        assert n_eq == 1 and n_gt == K - 1 and tau.item() == D[R.CLUSTER - R.CLUSTER // 2].item()
    if weighted and k == 100.0 and N > 1:
        # the mass tie at 0 straddles K: the zero-weight class, and the planted confident pixels whose fp32 cross entropy is 0
        zero_w = int((keep & (r.r.wi == 0)).sum())
        assert tau.item() == 0.0 and zero_w > 0 and zero_w <= n_eq <= zero_w + 6 and K == N == n_gt + n_eq


@pytest.mark.parametrize("P,C", [(257, 3), (262145, 4)])
def test_negative_weights_and_minus_zero(ops, P, C):
    """Weights need not be >= 0: the map then holds negative values and -0 (a negative weight times l = 0 at a planted confident
    pixel), and under k = 100 tau is the most negative entry.  The selection is exact on the device's map under float order with
    -0 == +0, the value is the float64 top-k mean of that map, run against run and step against the two calls bit for bit."""
    w = torch.tensor([(-1.5, 0.5, -0.0, 2.5)[c % 4] for c in range(C)])
    g, x, t, t_ref, sen, _ = R.inputs(P, C, torch.ones(C), True, seed=P + C)
    i120 = torch.nonzero(t_ref != IGN)[:4, 0]
    x[i120] = 0.0
    x[i120, 0] = 120.0                                       # l = 0 in fp32
    t[i120] = 0
    t_ref[i120] = 0
    keep = t_ref != IGN
    xg, tg, wg = x.to(DEV), t.to(DEV), w.to(DEV)
    for k in (10.0, 60.0, 100.0):
        out2, counts4, vmap = ops.topk_ce_fwd(xg, tg, C, wg, k, IGN)
        d1 = ops.topk_ce_bwd(xg, tg, C, vmap, out2, counts4, _nan(P, C), weight=wg, gmul=4.0, ignore_index=IGN)
        d2 = _nan(P, C)
        o2, c4, vm2 = ops.topk_ce_step(xg, tg, C, d2, weight=wg, k_percent=k, gmul=4.0, ignore_index=IGN)
        torch.cuda.synchronize()
        assert _same_bits(vmap, ops.ce_map_fwd(xg, tg, C, wg, IGN))
        assert _same_bits(o2, out2) and _same_bits(c4, counts4) and _same_bits(vm2, vmap) and _same_bits(d2, d1)
        vm = vmap.cpu()
        assert bool((vm[keep] < 0).any()) and bool((_bits(vmap)[i120] == -2 ** 31).all())        # negative entries, and -0 where planted
        K, N, tau, n_gt, n_eq, a = R.selection(vm, keep, k)
        assert counts4.tolist() == [K, N, n_gt, n_eq] and out2[1].item() == tau.item()
        top = torch.topk(vm[keep].double(), K).values
        tol = (SUM_DEPTH * U * top.abs().sum().item() + 3 * U * abs(top.sum().item())) / K
        assert abs(out2[0].item() - top.sum().item() / K) <= tol
        gone = ~keep | (a == 0)
        assert torch.equal(d1.cpu()[gone], torch.zeros(int(gone.sum()), C))
        if k == 100.0:
            assert tau.item() == vm[keep].min().item() < 0 and K == N


@pytest.mark.parametrize("P,C", [(257, 4), (262145, 3), (2097153, 2)])
def test_k_100_without_weights_is_the_cross_entropy_step(ops, P, C):
    """k = 100 with weight = NULL is the plain mean cross entropy: value and gradient agree with ``dct_ce_step`` within the sum of the
    two computations' bounds (not bitwise: the sums are folded in other orders and the gradient's factor is formed otherwise)."""
    w = torch.ones(C)
    g, x, t, t_ref, sen, _ = R.inputs(P, C, w, False, seed=5 * P + C)
    r = R.Ref(x, t_ref, w, C, 100.0)
    num_tol, _, grad_bound = focal_ref.ce_bounds(r.r)
    xg, tg = x.to(DEV), t.to(DEV)
    gs = torch.tensor([0.61], device=DEV)
    gg = float(np.float32(0.61)) * 8.0
    da, db = _nan(P, C), _nan(P, C)
    out2, counts4, _ = ops.topk_ce_step(xg, tg, C, da, k_percent=100.0, gscale=gs, gmul=8.0, ignore_index=IGN)
    ce = ops.ce_step(xg, tg, C, db, gscale=gs, gmul=8.0, ignore_index=IGN)
    torch.cuda.synchronize()
    assert counts4[0].item() == counts4[1].item() == r.N == int(ce[1].item())
    tol = num_tol / r.N + (SUM_DEPTH + 2) * U * abs(r.value.item())
    assert abs(out2[0].item() - ce[0].item()) <= 2 * tol, (out2[0].item(), ce[0].item(), tol)
    assert abs(out2[0].item() - r.value.item()) <= tol
    _check(da, db.cpu().double(), grad_bound(gg / r.N, 9) + grad_bound(gg / r.N, 6), "gradient")


@pytest.mark.parametrize("P,C", [(257, 4), (262145, 3)])
def test_nothing_counted(ops, P, C):
    """N = 0: K = 0, the value is NaN and every gradient entry is exactly 0 (the old value under accumulate)."""
    g = torch.Generator().manual_seed(3 + P)
    x = torch.randn(P, C, generator=g)
    t = torch.full((P,), IGN, dtype=torch.int64)
    t[::3] = C
    t[1::7] = -1
    old = torch.randn(P, C, generator=g)
    xg, tg = x.to(DEV), t.to(DEV)
    for acc in (False, True):
        d = old.to(DEV) if acc else _nan(P, C)
        out2, counts4, vmap = ops.topk_ce_step(xg, tg, C, d, k_percent=10.0, gmul=8.0, ignore_index=IGN, accumulate=acc)
        assert math.isnan(out2[0].item()) and counts4.tolist() == [0, 0, 0, 0]
        assert torch.equal(vmap.cpu(), torch.zeros(P)) and torch.equal(d.cpu(), old if acc else torch.zeros(P, C))
        o, c, v = ops.topk_ce_fwd(xg, tg, C, None, 10.0, IGN)
        assert math.isnan(o[0].item()) and c.tolist() == [0, 0, 0, 0]


def test_a_counted_nan_makes_the_value_nan(ops):
    P, C = 4099, 3
    g = torch.Generator().manual_seed(9)
    x = torch.randn(P, C, generator=g)
    t = torch.randint(0, C, (P,), generator=g)
    x[1234, 1] = float("nan")
    for k in (0.01, 10.0, 100.0):                            # tau itself is the NaN, or lies below it
        out2, counts4, _ = ops.topk_ce_fwd(x.to(DEV), t.to(DEV), C, None, k, IGN)
        assert math.isnan(out2[0].item()) and counts4[1].item() == P, k
    t[1234] = IGN
    out2, _, _ = ops.topk_ce_fwd(x.to(DEV), t.to(DEV), C, None, 10.0, IGN)
    assert math.isfinite(out2[0].item())                     # (an uncounted NaN is not looked at)


def test_topk_ce_status_codes(ops):
    P, C = 64, 3
    x = torch.zeros(P, C, device=DEV)
    t = torch.zeros(P, dtype=torch.int64, device=DEV)
    w = torch.ones(8, device=DEV)
    out, cnt, vm, dl = torch.zeros(2, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(P, device=DEV), torch.zeros(P, 9, device=DEV)
    need = ops._lib.load().dct_topk_ce_workspace_bytes(P)
    assert need == ops._lib.load().dct_topk_ce_workspace_bytes(2 ** 31 - 1) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p, st = ops.ptr, ops.stream

    def fwd(**a):
        return ["dct_topk_ce_fwd", a.get("x", p(x)), a.get("t", p(t)), a.get("P", P), a.get("C", C), IGN, p(w), a.get("k", 10.0),
                a.get("out", p(out)), a.get("cnt", p(cnt)), a.get("vm", p(vm)), a.get("ws", p(ws)), a.get("wsb", ws.numel()), st()]

    def bwd(**a):
        return ["dct_topk_ce_bwd", a.get("x", p(x)), a.get("t", p(t)), a.get("P", P), a.get("C", C), IGN, p(w), a.get("vm", p(vm)),
                a.get("out", p(out)), a.get("cnt", p(cnt)), None, 1.0, a.get("dl", p(dl)), 0, st()]

    def step(**a):
        return ["dct_topk_ce_step", a.get("x", p(x)), a.get("t", p(t)), a.get("P", P), a.get("C", C), IGN, p(w), a.get("k", 10.0),
                a.get("out", p(out)), a.get("cnt", p(cnt)), a.get("vm", p(vm)), None, 1.0, a.get("dl", p(dl)), 0, a.get("ws", p(ws)),
                a.get("wsb", ws.numel()), st()]
    for f in (fwd, bwd, step):
        ops.call(*f())
        bad = [dict(x=None), dict(t=None), dict(P=0), dict(out=None), dict(cnt=None), dict(vm=None)]
        if f is not bwd:
            ops.call(*f(k=100.0))
            ops.call(*f(k=1e-300))
            bad += [dict(k=0.0), dict(k=-1.0), dict(k=100.00001), dict(k=float("nan")), dict(k=float("inf"))]
        bad += [dict(dl=None)] if f in (bwd, step) else []
        for b in bad:
            with pytest.raises(RuntimeError, match=r"status -1"):
                ops.call(*f(**b))
        for b in (dict(C=1), dict(C=9), dict(P=2 ** 31)):
            with pytest.raises(RuntimeError, match=r"status -2"):
                ops.call(*f(**b))
        if f is not bwd:
            for b in (dict(wsb=need - 4), dict(ws=None)):
                with pytest.raises(RuntimeError, match=r"status -4"):
                    ops.call(*f(**b))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("C,k", [(2, 10.0), (4, 33.3)])
@pytest.mark.parametrize("strided", [False, True])
def test_module_against_the_reference(ops, C, k, strided):
    """TopKCrossEntropyLoss2d(k, weight) and its backward at [2, C, 16, 24] with an upstream gradient that is not 1, once through a
    non-contiguous NCHW input; ``last_topk``; then the same module after an in-place change of its device weights."""
    from dct_amd.loss import TopKCrossEntropyLoss2d, get_loss_fn
    B, H, W = 2, 16, 24
    g = torch.Generator().manual_seed(17 + C)
    w = focal_ref.weights(C)
    crit = get_loss_fn("topk_ce", k=k, weight=w.tolist())
    assert type(crit) is TopKCrossEntropyLoss2d
    x = torch.randn(B, C, H, 2 * W if strided else W, generator=g) * 2
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.25] = IGN
    leaf = x.to(DEV).requires_grad_(True)
    inp = leaf[..., ::2] if strided else leaf
    xs = x[..., ::2] if strided else x
    flat = xs.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    r = R.Ref(flat, t.reshape(-1), w, C, k)
    got = crit(inp, t.to(DEV))
    assert got.dim() == 0
    (3 * got).backward()
    torch.cuda.synchronize()
    out2, counts4 = crit.last_topk
    assert out2.is_cuda and counts4.is_cuda and counts4.dtype == torch.int64 and out2[0].item() == got.item()
    vm = ops.ce_map_fwd(flat.to(DEV), t.reshape(-1).to(DEV), C, w.to(DEV), IGN).cpu()
    K, N, tau, n_gt, n_eq, a = R.selection(vm, r.keep, k)
    assert counts4.tolist() == [K, N, n_gt, n_eq] and out2[1].item() == tau.item() and (K, N) == (r.K, r.N)
    assert abs(got.item() - r.value.item()) <= r.e[r.keep].max().item() + r.sum_tol(r.top_abs, K) + 3 * U * abs(r.value.item())
    gx = leaf.grad[..., ::2] if strided else leaf.grad
    gfac = 3.0 * a / K
    _check(gx.permute(0, 2, 3, 1).reshape(-1, C), gfac[:, None] * r.r.closed_form(), r.grad_bound(gfac, 9), "module gradient")
    if strided:
        assert torch.equal(leaf.grad[..., 1::2], torch.zeros_like(leaf.grad[..., 1::2]))
    buf = crit.device_weight(DEV, C)
    assert buf is crit.device_weight(DEV) and torch.equal(buf.cpu(), w)
    buf.mul_(2.0)
    again = crit(inp.detach(), t.to(DEV))
    np.testing.assert_allclose(again.item(), 2.0 * got.item(), rtol=1e-5)            # no denominator of weights: the value doubles
    assert crit.last_topk[1].tolist() == counts4.tolist()


def test_module_launches_the_topk_kernels(ops, monkeypatch):
    from dct_amd.loss import TopKCrossEntropyLoss2d
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 16, 24, generator=g).to(DEV).requires_grad_(True)
    t = torch.randint(0, 3, (2, 16, 24), generator=g).to(DEV)
    seen = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    TopKCrossEntropyLoss2d(k=100)(x, t).backward()
    assert seen == ["dct_topk_ce_fwd", "dct_topk_ce_bwd"], seen
    with pytest.raises(ValueError, match="TopKCrossEntropyLoss2d: 4 class weights for logits of 3 classes"):
        TopKCrossEntropyLoss2d(weight=[0.1, 1, 2.5, 0])(x, t)
