"""Boundary loss on the device: the signed distance maps against the float64 references of tests/test_boundary_cpu.py, the loss and
gradient kernels against float64 at bounds derived from the operations (the method of tests/test_loss_kernels_scale_gpu.py), the
modules, the status codes and one small co-training run on the generic step.

Bounds.  U = 2^-24.
  Maps, unit spacing: every squared distance is an integer below 2^24 (exact in fp32); outside, sqrtf is correctly rounded; inside, the
    kernel takes 1 - sqrt in fp64 and rounds once, the reference's own operations (1.f - sqrtf(d2) would round twice and miss this
    check by an ulp of the difference, e.g. at 1 - sqrt(2)).  So the map is the float64 reference rounded once: bit-equal to np.float32(sdf_ref).
  Maps, spacing (1.5, 0.75): the kernels form (run sy)^2 [two roundings], d = df sx [one] and fma(d, d, g) [one]: at most 4U relative on d2,
    hence 2U on the exact root and 2.5U on the rounded one, plus U on the "- 1" (inside: 2U on the root and U/2 on the one rounding of the
    difference): |phi - ref| <= 4U (d_ref + 1), d_ref the reference's unsigned distance.
  Loss: per counted pixel a = sum_{c in mask} s_c phi_c as an fma chain.  s_c carries (C + 6 + |x_c - m|) U relative error (the softmax
    of that file), the chain adds U per step on partial sums <= sum |s phi|: |e_i| <= sum_c (2C + 6 + |x_c - m|) U s_c |phi_c|.  The
    fp32 sum over pixels adds SUM_DEPTH U sum_i sum_c s_c |phi_c|; N K is exact and the division rounds once (2U |L| covers it).
  Gradient: d = (g s_c)(q_c - dot), q_c = phi_c / (N K) [U], dot = fma chain of s_k q_k:
    E_dot = sum_k (2C + 7 + |x_k - m|) U s_k |q_k|;  |d err| <= |g| s_c (((C + 6 + |x_c - m|) + 4) U |q_c - dot| + U |q_c| + E_dot)
    (the 4: g = gscale gmul, g s_c, the subtraction, the final product); accumulate rounds the sum once more (U |old + d|)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_boundary_cpu import IGN, boundary_grad64, sdf_ref, structured_cases, unsigned_ref  # noqa: E402
from test_loss_kernels_scale_gpu import DEV, MARGIN_SAT, SUM_DEPTH, U, _check, _nan, _sentinels, _sm64  # noqa: E402

SPACINGS = [(1.0, 1.0), (1.5, 0.75)]
MAP_SHAPES = [  # B, H, W, C, classes
    (2, 13, 9, 4, None),            # below one wave, odd
    (1, 70, 300, 3, None),          # W over 256 and not a multiple of 4
    (3, 257, 64, 2, None),          # H just past a power of two
    (1, 1, 40, 2, None),            # one row
    (1, 40, 1, 2, None),            # one column
    (1, 4, 1024, 2, None),          # the extent limit
    (2, 24, 20, 8, [1, 3, 7]),      # masked-out classes are exactly 0
]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from dct_amd import hip_ops
    return hip_ops


def _device_map(ops, gt, C, classes, spacing):
    """The chain's output over a NaN pre-fill of its output buffer (an element never written stays NaN)."""
    from dct_amd import _lib
    from dct_amd._lib import ptr, stream
    t = torch.from_numpy(gt).to(DEV)
    B, H, W = t.shape
    phi = _nan(B, H, W, C)
    ws = torch.empty(_lib.load().dct_signed_distance_workspace_bytes(B, H, W, C), dtype=torch.uint8, device=DEV)
    mask = (1 << C) - 1 if classes is None else sum(1 << c for c in classes)
    _lib.call("dct_signed_distance", ptr(t), B, H, W, C, mask, float(spacing[0]), float(spacing[1]), ptr(phi), ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    return phi


# ------------------------------------------------------------------------------------------------------------------ 1. the maps
@pytest.mark.parametrize("B,H,W,C,classes", MAP_SHAPES)
def test_maps_against_the_float64_reference(ops, B, H, W, C, classes):
    ulp_off = []
    for name, gt in structured_cases(B, H, W, C).items():
        for spacing in SPACINGS:
            ref = sdf_ref(gt, C, classes, spacing)
            got = _device_map(ops, gt, C, classes, spacing).cpu().numpy()
            assert not np.isnan(got).any(), (name, spacing, "an element was never written")
            assert np.array_equal(got, ops.signed_distance(torch.from_numpy(gt).to(DEV), C, classes, spacing).cpu().numpy()), (name, spacing)
            if classes is not None:
                assert not got[..., [c for c in range(C) if c not in classes]].any(), (name, spacing)
            if spacing == (1.0, 1.0):
                want = ref.astype(np.float32)
                if not np.array_equal(got, want):
                    ulp_off.append((name, int((got != want).sum()), float(np.abs(got.astype(np.float64) - ref).max())))
            else:
                bound = 4 * U * (unsigned_ref(ref) + 1.0)
                bound[ref == 0.0] = 0.0             # the zero rule is exact (no distance is exactly 1 at this spacing)
                err = np.abs(got.astype(np.float64) - ref)
                print(f"{name} {spacing}: max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
                assert (err <= bound).all(), (name, spacing, float(err.max()), int((err > bound).sum()))
    assert not ulp_off, ulp_off


# ------------------------------------------------------------------------------------------------ 3. loss and gradient against float64
def _spread_logits(g, P, C):
    """Logits with a spread of margins: a third plain, a third with one class lifted by a margin in [0, 12], a third saturated."""
    x = torch.randn(P, C, generator=g) * 2
    kind = torch.randint(0, 3, (P,), generator=g)
    top = torch.randint(0, C, (P,), generator=g)
    lift = torch.where(kind == 1, torch.rand(P, generator=g) * 12, torch.where(kind == 2, torch.tensor(MARGIN_SAT), torch.tensor(0.0)))
    x[torch.arange(P), top] += lift
    return x


def _loss_case(ops, x, t, phi, C, classes, accumulate, gscale, gmul, seed):
    """dct_boundary_fwd / _bwd on (x [P, C], t [P], phi [P, C], all on the host in fp32 / int64) against float64 at the derived bounds."""
    P = x.shape[0]
    g = torch.Generator().manual_seed(seed)
    mask_list = list(range(C)) if classes is None else list(classes)
    K = len(mask_list)
    m = torch.zeros(C, dtype=torch.float64)
    m[mask_list] = 1.0
    counted = (t != IGN) & (t >= 0) & (t < C)
    N = int(counted.sum())
    assert N > 0
    # sentinels: a counted pixel with uniform softmax and |phi| = D on every class of the mask: each is >= 1 % of sum |s phi|
    sen = _sentinels(P)
    D = max(1e4, 0.1 * P)
    t[sen] = sen % C
    counted[sen] = True
    N = int(counted.sum())
    x[sen] = 0.0
    phi[sen] = torch.where(sen[:, None] % 2 == 0, D, -D).to(torch.float32) * torch.ones(C)

    p, spread = _sm64(x)
    f = phi.double()
    a = (p * f * m).sum(1) * counted
    absa = (p * f.abs() * m).sum(1) * counted
    L_ref = a.sum().item() / (N * K)
    e = ((2 * C + 6 + spread) * U * p * f.abs() * m).sum(1) * counted
    tol = (e.sum().item() + SUM_DEPTH * U * absa.sum().item()) / (N * K) + 2 * U * abs(L_ref)
    assert absa[sen].min().item() / (N * K) > 4 * tol                   # one lost or doubled sentinel is far outside the bound

    gs_host = 1.0 if gscale is None else float(np.float32(gscale))
    gg = gs_host * gmul
    q = m * f / (N * K)
    dot = (p * q).sum(1, keepdim=True)
    dref = boundary_grad64(x.double(), t, f, mask_list, gg)
    e_dot = ((2 * C + 7 + spread) * U * p * q.abs()).sum(1, keepdim=True)
    bound = abs(gg) * p * ((C + 10 + spread) * U * (q - dot).abs() + U * q.abs() + e_dot) + 1e-30
    bound = torch.where(counted[:, None], bound, torch.zeros(()))
    old = torch.randn(P, C, generator=g) if accumulate else None
    if accumulate:
        dref = dref + old.double()
        bound = bound + U * dref.abs()

    xg, tg, fg = x.to(DEV), t.to(DEV), phi.to(DEV)
    gsd = None if gscale is None else torch.tensor([gscale], device=DEV)
    mask = sum(1 << c for c in mask_list)
    out = ops.boundary_fwd(xg, tg, fg, C, mask, IGN)
    d = old.to(DEV) if accumulate else _nan(P, C)
    ops.boundary_bwd(xg, tg, fg, C, out[1:2], d, class_mask=mask, gscale=gsd, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    # 2. the same call again: bit-identical
    out_b = ops.boundary_fwd(xg, tg, fg, C, mask, IGN)
    d_b = old.to(DEV) if accumulate else _nan(P, C)
    ops.boundary_bwd(xg, tg, fg, C, out_b[1:2], d_b, class_mask=mask, gscale=gsd, gmul=gmul, ignore_index=IGN, accumulate=accumulate)
    torch.cuda.synchronize()
    print(f"P {P} C {C}: L {out[0].item()!r} ref {L_ref!r} err {abs(out[0].item() - L_ref):.3e} tol {tol:.3e}")
    assert out[1].item() == N, (out[1].item(), N)
    assert abs(out[0].item() - L_ref) <= tol, (out[0].item(), L_ref, tol)
    _check(d, dref, bound, "boundary_bwd")
    assert torch.equal(out, out_b) and torch.equal(d, d_b)
    # uncounted pixels: exactly 0, exactly the old value under accumulate
    un = ~counted
    if un.any():
        want = old[un] if accumulate else torch.zeros(int(un.sum()), C)
        assert torch.equal(d.cpu()[un], want)


LOSS_CASES = [  # B, H, W, C, classes, ignored, accumulate, gscale, gmul
    (2, 13, 9, 4, None, False, False, None, 1.0),
    (2, 13, 9, 4, [1, 2, 3], True, True, 0.5, 1024.0),
    (2, 70, 300, 3, [1, 2], True, False, 0.5, 1.0),
    (2, 70, 300, 3, None, False, True, None, 1024.0),
]


@pytest.mark.parametrize("B,H,W,C,classes,ignored,accumulate,gscale,gmul", LOSS_CASES)
def test_loss_and_gradient_against_float64(ops, B, H, W, C, classes, ignored, accumulate, gscale, gmul):
    """The reference reads the device's own map and the very fp32 logits the kernels saw: the map's error is the maps test's business."""
    g = torch.Generator().manual_seed(17 * H + C)
    gt = structured_cases(B, H, W, C)["ignored" if ignored else "blobs"]
    if ignored:
        gt = gt.copy()
        gt.reshape(-1)[torch.nonzero(torch.rand(gt.size, generator=g) < 0.2)[:, 0].numpy()] = IGN
    t = torch.from_numpy(gt)
    phi = ops.signed_distance(t.to(DEV), C, classes, (1.5, 0.75)).cpu().reshape(-1, C)
    assert phi.abs().max() > 1
    _loss_case(ops, _spread_logits(g, B * H * W, C), t.reshape(-1).clone(), phi, C, classes, accumulate, gscale, gmul, seed=H)


@pytest.mark.parametrize("C,classes,accumulate,gscale,gmul", [(4, [1, 2, 3], False, 0.5, 1024.0), (8, None, True, None, 1.0), (5, [0, 4], True, 0.5, 1.0)])
def test_loss_one_pixel_past_the_grid_cap(ops, C, classes, accumulate, gscale, gmul):
    """262,145 pixels as one strip: one pixel more than 1024 blocks of 256 threads take in one trip; a synthetic map."""
    P = 262145
    g = torch.Generator().manual_seed(C)
    t = torch.randint(0, C, (P,), generator=g)
    t[torch.rand(P, generator=g) < 0.25] = IGN
    t[torch.rand(P, generator=g) < 0.01] = C + 1
    phi = (torch.randn(P, C, generator=g) * 20).to(torch.float32)
    _loss_case(ops, _spread_logits(g, P, C), t, phi, C, classes, accumulate, gscale, gmul, seed=C)


@pytest.mark.parametrize("P,C", [(117, 4), (262145, 3)])
def test_nothing_counted(ops, P, C):
    """N = 0: the loss is exactly 0, the gradient exactly 0 (exactly the old value under accumulate)."""
    g = torch.Generator().manual_seed(P)
    x = _spread_logits(g, P, C).to(DEV)
    t = torch.full((P,), IGN, dtype=torch.int64)
    t[::3] = C
    t = t.to(DEV)
    phi = (torch.randn(P, C, generator=g) * 5).to(DEV)
    out = ops.boundary_fwd(x, t, phi, C, None, IGN)
    d = _nan(P, C)
    ops.boundary_bwd(x, t, phi, C, out[1:2], d, ignore_index=IGN)
    old = torch.randn(P, C, generator=g).to(DEV)
    d2 = old.clone()
    ops.boundary_bwd(x, t, phi, C, out[1:2], d2, gmul=1024.0, ignore_index=IGN, accumulate=True)
    torch.cuda.synchronize()
    assert out[0].item() == 0.0 and out[1].item() == 0.0
    assert torch.equal(d, torch.zeros_like(d)) and torch.equal(d2, old)


# -------------------------------------------------------------------------------------------------------------------- 4. the modules
@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(99)
    B, C, H, W = 2, 4, 37, 45
    gt = structured_cases(B, H, W, C)["ignored"]
    x = (torch.randn(B, C, H, W, generator=g) * 2).to(DEV)
    return x, torch.from_numpy(gt).to(DEV), C


def test_boundary_module_equals_the_kernel_calls(ops, batch):
    from dct_amd.loss import BoundaryLoss, signed_distance_map
    x, t, C = batch
    classes, spacing = [1, 2, 3], (1.5, 0.75)
    crit = BoundaryLoss(classes, spacing)
    xr = x.clone().requires_grad_()
    loss = crit(xr, t)
    loss.backward()
    lp = x.permute(0, 2, 3, 1).contiguous()
    phi = ops.signed_distance(t, C, classes, spacing)
    out = ops.boundary_fwd(lp, t.reshape(-1), phi, C, 0b1110, IGN)
    dl = ops.boundary_bwd(lp, t.reshape(-1), phi, C, out[1:2], torch.empty_like(lp), class_mask=0b1110, gscale=torch.ones(1, device=DEV))
    assert torch.equal(loss.detach(), out[0]) and torch.equal(xr.grad, dl.permute(0, 3, 1, 2))
    # the map handed in: bit for bit the map computed; two calls are identical
    dmap = signed_distance_map(t[:, None], C, classes, spacing)
    assert tuple(dmap.shape) == tuple(x.shape) and not dmap.requires_grad
    assert torch.equal(dmap, phi.permute(0, 3, 1, 2)) and torch.equal(dmap, signed_distance_map(t, C, classes, spacing))
    xr2 = x.clone().requires_grad_()
    loss2 = crit(xr2, t, dist_map=dmap)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(xr2.grad, xr.grad)
    # bf16 and NCHW-contiguous inputs: the module works on their fp32 NHWC copy
    xb = x.to(torch.bfloat16).contiguous().requires_grad_()
    lb = crit(xb, t)
    lb.backward()
    xf = xb.detach().float().requires_grad_()
    lf = crit(xf, t)
    lf.backward()
    assert torch.equal(lb.detach(), lf.detach()) and xb.grad.dtype == torch.bfloat16
    assert torch.equal(xb.grad, xf.grad.to(torch.bfloat16))


def test_ce_boundary_module_is_the_sum_of_its_terms(batch):
    """value = a CE(weight) + b Boundary to fp32 rounding of the final sum: each coefficient rounds to fp32, each product rounds and
    the sum rounds: 3U (|a ce| + |b bd|), asserted at 4U.  Gradient: autograd hands fl(a) / fl(b) to the kernels as gscale, where it
    goes through at most three roundings (g = gscale gmul [/ count], g w or g s_c, the final product) against the same three in the
    reference's g = 1 kernel followed by the test's exact a * d, plus fl(a) itself and the sum of the two gradients: 8U (|a dce| + |b dbd|)."""
    from dct_amd.loss import BoundaryLoss, CrossEntropyBoundaryLoss2d, CrossEntropyLoss2d
    x, t, C = batch
    Wt, a, b = [0.5, 1.0, 2.0, 1.5], 0.7, 0.3

    def run(crit):
        xr = x.clone().requires_grad_()
        v = crit(xr, t)
        v.backward()
        return v.detach().double().cpu(), xr.grad.double().cpu()
    ce, dce = run(CrossEntropyLoss2d(weight=Wt))
    bd, dbd = run(BoundaryLoss())
    both = CrossEntropyBoundaryLoss2d(weight=Wt, ce_coef=a, boundary_coef=b)
    v, dv = run(both)
    assert abs(v - (a * ce + b * bd)) <= 4 * U * (abs(a * ce) + abs(b * bd))
    assert ((dv - (a * dce + b * dbd)).abs() <= 8 * U * ((a * dce).abs() + (b * dbd).abs()) + 1e-30).all()
    assert torch.equal(both.last_terms[0].double().cpu(), ce) and torch.equal(both.last_terms[1].double().cpu(), bd)
    # boundary_coef is read at every call
    both.boundary_coef = 2 * b
    v2, _ = run(both)
    assert abs(v2 - (a * ce + 2 * b * bd)) <= 4 * U * (abs(a * ce) + abs(2 * b * bd)) and v2 != v
    # a coefficient of exactly 0 removes its term: bit for bit the CE module (weighted and not)
    for w in (Wt, None):
        v0, d0 = run(CrossEntropyBoundaryLoss2d(weight=w, boundary_coef=0.0))
        vc, dc = run(CrossEntropyLoss2d(weight=w))
        assert torch.equal(v0, vc) and torch.equal(d0, dc)
    vb, db = run(CrossEntropyBoundaryLoss2d(ce_coef=0.0, boundary_coef=1.0))
    assert torch.equal(vb, bd) and torch.equal(db, dbd)


# ---------------------------------------------------------------------------------------------------------------- 5. status codes
def test_refusals_launch_nothing(ops):
    from dct_amd import _lib
    lib = _lib.load()
    BAD, UNS, WSP = -1, -2, -4
    B, H, W, C = 2, 8, 12, 4
    t = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)
    t[:, 2:5, 3:7] = 1
    phi = _nan(B * H * W * C + 4)
    ws = torch.empty(lib.dct_signed_distance_workspace_bytes(B, H, W, C) + 16, dtype=torch.uint8, device=DEV)
    inf, nan = float("inf"), float("nan")

    def sd(tp=t.data_ptr(), B=B, H=H, W=W, C=C, mask=15, sy=1.0, sx=1.0, pp=phi.data_ptr(), wp=ws.data_ptr(), wb=ws.numel()):
        return lib.dct_signed_distance(tp, B, H, W, C, mask, sy, sx, pp, wp, wb, 0)
    for kw, want in ((dict(tp=0), BAD), (dict(pp=0), BAD), (dict(wp=0), BAD), (dict(sy=0.0), BAD), (dict(sx=-1.0), BAD), (dict(sy=inf), BAD),
                     (dict(sx=nan), BAD), (dict(mask=0), BAD), (dict(mask=16), BAD), (dict(B=0), BAD), (dict(H=0), BAD), (dict(W=-1), BAD),
                     (dict(pp=phi.data_ptr() + 4), BAD), (dict(tp=t.data_ptr() + 8), BAD), (dict(wp=ws.data_ptr() + 4), BAD),
                     (dict(C=1), UNS), (dict(C=9), UNS), (dict(H=1025), UNS), (dict(W=1025), UNS), (dict(B=65536), UNS),
                     (dict(wb=lib.dct_signed_distance_workspace_bytes(B, H, W, C) - 1), WSP)):
        assert sd(**kw) == want, (kw, want)
    torch.cuda.synchronize()
    assert torch.isnan(phi).all()

    P = B * H * W
    x = torch.randn(P * C + 4, device=DEV)
    f = torch.randn(P * C + 4, device=DEV)
    tt = t.reshape(-1)
    out = _nan(2)
    lws = torch.empty(lib.dct_loss_workspace_bytes(0), dtype=torch.uint8, device=DEV)

    def fwd(xp=x.data_ptr(), tp=tt.data_ptr(), fp=f.data_ptr(), P=P, C=C, mask=15, op=out.data_ptr(), wp=lws.data_ptr(), wb=lws.numel()):
        return lib.dct_boundary_fwd(xp, tp, fp, P, C, IGN, mask, op, wp, wb, 0)
    for kw, want in ((dict(xp=0), BAD), (dict(tp=0), BAD), (dict(fp=0), BAD), (dict(op=0), BAD), (dict(wp=0), BAD), (dict(P=0), BAD),
                     (dict(mask=0), BAD), (dict(mask=48), BAD), (dict(xp=x.data_ptr() + 4), BAD), (dict(fp=f.data_ptr() + 4), BAD),
                     (dict(C=1), UNS), (dict(C=9), UNS), (dict(wb=lws.numel() - 1), WSP)):
        assert fwd(**kw) == want, (kw, want)
    cnt = torch.full((1,), float(P), device=DEV)
    dl = _nan(P * C + 4)

    def bwd(xp=x.data_ptr(), tp=tt.data_ptr(), fp=f.data_ptr(), P=P, C=C, mask=15, cp=cnt.data_ptr(), dp=dl.data_ptr()):
        return lib.dct_boundary_bwd(xp, tp, fp, P, C, IGN, mask, cp, 0, 1.0, dp, 0, 0)
    for kw, want in ((dict(xp=0), BAD), (dict(tp=0), BAD), (dict(fp=0), BAD), (dict(cp=0), BAD), (dict(dp=0), BAD), (dict(P=-3), BAD),
                     (dict(mask=0), BAD), (dict(dp=dl.data_ptr() + 4), BAD), (dict(xp=x.data_ptr() + 8), BAD), (dict(C=1), UNS), (dict(C=9), UNS)):
        assert bwd(**kw) == want, (kw, want)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dl).all()
    # (and the accepted calls do write)
    assert sd() == 0 and fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(phi[:P * C]).any() and not torch.isnan(out).any() and not torch.isnan(dl[:P * C]).any()


# -------------------------------------------------------------------------------------------------------------------- 6. the trainer
def _train(tmp_path, sup, n=2):
    """test_dice_graph_replay_equals_eager_step_sequence's construction: Enet, C = 3, B = 2, 64 x 64, fp32, FGSM on."""
    from dct_amd.loss import get_loss_fn
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, B, H = 3, 2, 64
    segs = []
    for seed in (11, 12):
        torch.manual_seed(seed)
        segs.append(Segmentator({"name": "enet", "num_classes": C, "compute_dtype": torch.float32},
                                {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4}, {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    lab = [FakeLoader(batches(81 + i, n, B, H, C), B) for i in range(2)]
    unl = FakeLoader(batches(91, n, B, H, C), B)
    crit = {"sup": sup, "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    tr = CoTrainer(segs, lab, unl, unl, crit, max_epoch=1, save_dir=str(tmp_path), device=DEV, axises=[1, 2],
                   cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
                   adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05},
                   adv_training_dict={"eplision": 0.03}, use_tqdm=False, steps_per_epoch=n)
    assert not tr._fused_ok()                    # every trainer of this test runs the generic step
    for s in segs:
        s.train()
    before = [torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]).clone() for s in segs]
    values = []
    for k in range(n):
        lb = [(lab[i][k][0][0], lab[i][k][0][1]) for i in range(2)]
        out = tr._run_step(lb, (unl[k][0][0], unl[k][0][1]), True, True, (0, 1))
        values.append([float(v) for v in out["sup"]] + [float(out["jsd"]), float(out["adv"])])
    torch.cuda.synchronize()
    after = [torch.cat([p.detach().flatten() for p in s.torchnet.parameters()]) for s in segs]
    return tr, values, before, after


def test_trainer_runs_ce_boundary_on_the_generic_step(tmp_path):
    from dct_amd.loss import get_loss_fn
    from dct_amd.loss import CrossEntropyLoss2d

    class GenericCE(CrossEntropyLoss2d):        # (the trainer keeps the exact type on the fused step: a subclass goes through the module)
        pass
    tr, vals, before, after = _train(tmp_path / "bd", get_loss_fn('ce_boundary', boundary_coef=0.1, classes=[1, 2]))
    assert all(math.isfinite(v) for step in vals for v in step)
    assert all(not torch.equal(b, a) and bool(torch.isfinite(a).all()) for b, a in zip(before, after))
    assert tr.criterions["sup"].last_terms[1] is not None
    # a plain-CE trainer on the generic path: the supervised values differ (no silent fall-through to CE) ...
    ce_tr, ce_vals, _, ce_after = _train(tmp_path / "ce", GenericCE())
    for x, y in zip(vals[0][:2], ce_vals[0][:2]):
        assert abs(x - y) > 1e-3 * abs(y), (x, y)
    # ... and with boundary_coef = 0 they are that trainer's, bit for bit
    _, z_vals, _, z_after = _train(tmp_path / "zero", get_loss_fn('ce_boundary', boundary_coef=0.0, classes=[1, 2]))
    assert z_vals == ce_vals
    assert all(torch.equal(a, b) for a, b in zip(z_after, ce_after))
