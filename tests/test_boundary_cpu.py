"""Boundary loss, host side: the float64 references of the signed distance maps (scipy's Euclidean distance transform and an all-pairs
search, which must agree exactly), the gradient identity of include/dct.h against float64 autograd, the registry, the constructors'
refusals and the workspace query.  tests/test_boundary_gpu.py imports the references and the structured label fields from here."""
import numpy as np
import pytest
import torch

IGN = 255


# ------------------------------------------------------------------------------------------------------------------ references
def _live(m, c, classes):
    """The zero rule: class c has a map in this image only if it is in ``classes`` and its mask is neither empty nor the whole image."""
    return (classes is None or c in classes) and 0 < int(m.sum()) < m.size


def sdf_ref(gt, C, classes=None, spacing=(1., 1.)):
    """float64 [B, H, W, C]: the rule of include/dct.h by scipy.ndimage.distance_transform_edt on both sides of every mask."""
    from scipy.ndimage import distance_transform_edt as edt
    gt = np.asarray(gt)
    B, H, W = gt.shape
    phi = np.zeros((B, H, W, C))
    for b in range(B):
        for c in range(C):
            m = gt[b] == c
            if _live(m, c, classes):
                phi[b, :, :, c] = np.where(m, -(edt(m, sampling=spacing) - 1.0), edt(~m, sampling=spacing))
    return phi


def sdf_brute(gt, C, classes=None, spacing=(1., 1.)):
    """The same rule by a search over all pairs of pixels."""
    gt = np.asarray(gt)
    B, H, W = gt.shape
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d2 = (spacing[0] * (yy.reshape(-1, 1) - yy.reshape(1, -1))) ** 2 + (spacing[1] * (xx.reshape(-1, 1) - xx.reshape(1, -1))) ** 2
    phi = np.zeros((B, H, W, C))
    for b in range(B):
        for c in range(C):
            m = (gt[b] == c).reshape(-1)
            if _live(m, c, classes):
                to_in = np.sqrt(d2[:, m].min(1))
                to_out = np.sqrt(d2[:, ~m].min(1))
                phi[b, :, :, c] = np.where(m, -(to_out - 1.0), to_in).reshape(H, W)
    return phi


def unsigned_ref(phi_ref):
    """The reference's unsigned distance: phi where it is positive, 1 - phi inside the class."""
    return np.where(phi_ref > 0, phi_ref, 1.0 - phi_ref)


# ------------------------------------------------------------------------------------------------------------ structured label fields
def structured_cases(B, H, W, C, seed=0):
    """name -> int64 [B, H, W]: every place where the distance chain can go wrong, at any shape (one row, one column included)."""
    rng = np.random.RandomState(seed + 131 * H + W)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cases = {}

    blobs = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for c in range(1, C):       # one ellipse per foreground class, later classes on top
            cy, cx = rng.randint(0, H), rng.randint(0, W)
            ry, rx = 1 + rng.randint(0, max(1, H // 3)), 1 + rng.randint(0, max(1, W // 3))
            blobs[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = c
    cases["blobs"] = blobs

    absent = blobs.copy()           # class 1 absent from image 0, present in the last image (one image: absent)
    absent[0][absent[0] == 1] = 0
    absent[B - 1, H // 2, W // 2] = 1 if B > 1 else absent[B - 1, H // 2, W // 2]
    cases["absent"] = absent

    full = blobs.copy()             # class 1 fills image 0
    full[0] = 1
    cases["full"] = full

    one = np.zeros((B, H, W), np.int64)     # a one-pixel class, in a corner in the last image
    one[:, H // 3, W // 3] = 1
    one[B - 1] = 0
    one[B - 1, H - 1, W - 1] = 1
    cases["one_pixel"] = one

    frame = np.zeros((B, H, W), np.int64)   # class 1 touches all four borders
    frame[:, 0, :] = frame[:, H - 1, :] = frame[:, :, 0] = frame[:, :, W - 1] = 1
    cases["borders"] = frame

    cases["checkerboard"] = np.broadcast_to((yy + xx) % 2, (B, H, W)).astype(np.int64).copy()

    ign = blobs.copy()              # a few ignore_index pixels and one target of C + 1
    flat = ign.reshape(-1)
    flat[rng.choice(flat.size, size=min(5, flat.size), replace=False)] = IGN
    flat[rng.randint(0, flat.size)] = C + 1
    cases["ignored"] = ign

    cases["random"] = rng.randint(0, C, size=(B, H, W)).astype(np.int64)
    return cases


# ------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("spacing", [(1.0, 1.0), (1.5, 0.75)])
def test_scipy_and_all_pairs_references_agree_exactly(spacing):
    for name, gt in structured_cases(2, 13, 9, 4).items():
        for classes in (None, [1, 3]):
            a, b = sdf_ref(gt, 4, classes, spacing), sdf_brute(gt, 4, classes, spacing)
            assert np.array_equal(a, b), (name, classes, np.abs(a - b).max())


def test_reference_zero_rules_and_checkerboard():
    cases = structured_cases(2, 13, 9, 4)
    assert not sdf_ref(cases["full"], 4)[0].any()                   # image 0: class 1 fills it, the others are absent
    assert not sdf_ref(cases["absent"], 4)[0, :, :, 1].any() and sdf_ref(cases["absent"], 4)[1, :, :, 1].any()
    assert not sdf_ref(cases["blobs"], 4, [1, 3])[..., [0, 2]].any()
    cb = sdf_ref(cases["checkerboard"], 4)
    gt = cases["checkerboard"]
    for c in (0, 1):                # every distance is 1: phi is 1 outside and -(1 - 1) = 0 inside
        assert np.array_equal(cb[..., c], np.where(gt == c, 0.0, 1.0))
    ig = sdf_ref(cases["ignored"], 4)
    assert (ig[cases["ignored"] >= 4] >= 0).all()                   # a target outside [0, C) is background for every class


def boundary_loss64(x, t, phi, classes, ignore_index=IGN):
    """float64 L of include/dct.h: x [P, C], t [P], phi [P, C] -> (L, N)."""
    C = x.shape[1]
    counted = (t != ignore_index) & (t >= 0) & (t < C)
    N = int(counted.sum())
    m = torch.zeros(C, dtype=torch.float64)
    m[list(range(C)) if classes is None else list(classes)] = 1.0
    if N == 0:
        return x.sum() * 0.0, 0
    s = torch.softmax(x, 1)
    return (s * phi * m * counted[:, None]).sum() / (N * m.sum()), N


def boundary_grad64(x, t, phi, classes, g=1.0, ignore_index=IGN):
    """The gradient formula of include/dct.h in float64."""
    C = x.shape[1]
    counted = (t != ignore_index) & (t >= 0) & (t < C)
    N = int(counted.sum())
    m = torch.zeros(C, dtype=torch.float64)
    m[list(range(C)) if classes is None else list(classes)] = 1.0
    if N == 0:
        return torch.zeros_like(x)
    s = torch.softmax(x, 1)
    q = m * phi / (N * m.sum())
    return torch.where(counted[:, None], g * s * (q - (s * q).sum(1, keepdim=True)), torch.zeros((), dtype=torch.float64))


@pytest.mark.parametrize("classes", [None, [1, 2]])
def test_gradient_identity_against_float64_autograd(classes):
    g = torch.Generator().manual_seed(3)
    gt = structured_cases(2, 13, 9, 4)["ignored"]
    t = torch.from_numpy(gt).reshape(-1)
    phi = torch.from_numpy(sdf_ref(gt, 4, classes, (1.5, 0.75))).reshape(-1, 4)
    x = (torch.randn(t.numel(), 4, generator=g, dtype=torch.float64) * 3).requires_grad_()
    L, N = boundary_loss64(x, t, phi, classes)
    assert 0 < N < t.numel()
    (auto,) = torch.autograd.grad(L, x)
    formula = boundary_grad64(x.detach(), t, phi, classes)
    assert (auto - formula).abs().max().item() < 1e-15
    assert not formula[(t == IGN) | (t >= 4)].any()


def test_registry_returns_the_two_criteria():
    from dct_amd.loss import LOSS, BoundaryLoss, CrossEntropyBoundaryLoss2d, get_loss_fn
    assert type(get_loss_fn('boundary')) is BoundaryLoss
    crit = get_loss_fn('ce_boundary', boundary_coef=0.5, classes=[1, 2], spacing=(1.5, 0.75))
    assert type(crit) is CrossEntropyBoundaryLoss2d
    assert crit.boundary_coef == 0.5 and crit.ce_coef == 1.0 and crit.classes == [1, 2] and crit.spacing == (1.5, 0.75)
    assert LOSS['boundary'] is BoundaryLoss and LOSS['ce_boundary'] is CrossEntropyBoundaryLoss2d
    with pytest.raises(ValueError):
        get_loss_fn("no_such_loss")


def test_constructors_refuse_bad_classes_and_spacing():
    from dct_amd.loss import BoundaryLoss, CrossEntropyBoundaryLoss2d, signed_distance_map
    for make in (BoundaryLoss, lambda **kw: CrossEntropyBoundaryLoss2d(None, 1.0, 0.01, **kw)):
        with pytest.raises(ValueError, match="empty"):
            make(classes=[])
        with pytest.raises(ValueError, match="negative"):
            make(classes=[-1, 2])
        for bad in ((0.0, 1.0), (1.0, -2.0), (float("inf"), 1.0), (float("nan"), 1.0), (1.0,), 1.0):
            with pytest.raises(ValueError, match="spacing"):
                make(spacing=bad)
        assert make(classes=range(1, 4), spacing=(2, 3)).spacing == (2.0, 3.0)
    x, t = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    # too large a class shows once C is known: at the call, before anything else is looked at
    for call in (lambda: BoundaryLoss(classes=[1, 3])(x, t), lambda: CrossEntropyBoundaryLoss2d(classes=[1, 3])(x, t),
                 lambda: signed_distance_map(t, 3, classes=[3])):
        with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
            call()
    for call in (lambda: BoundaryLoss()(x, t), lambda: CrossEntropyBoundaryLoss2d()(x, t), lambda: signed_distance_map(t, 3),
                 lambda: signed_distance_map(t[:, None], 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="both 0"):
        CrossEntropyBoundaryLoss2d(ce_coef=0.0, boundary_coef=0.0)(x, t)


def test_workspace_query():
    from dct_amd import _lib
    ws = _lib.load().dct_signed_distance_workspace_bytes
    for B, H, W, C in ((2, 16, 16, 1), (2, 16, 16, 9), (2, 1025, 16, 4), (2, 16, 1025, 4), (0, 16, 16, 4), (65536, 16, 16, 4)):
        assert ws(B, H, W, C) == 0, (B, H, W, C)
    sizes = [ws(B, 256, 256, 4) for B in (1, 2, 8, 16, 64)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert ws(1, 1024, 1024, 8) >= 1024 * 1024 * 9 * 4
    assert ws(1, 1, 1, 2) > 0
