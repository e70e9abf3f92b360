"""Hausdorff distance (include/dct.h ``dct_hausdorff``): the numpy references the GPU tests compare against, checked against each
other here, plus what can be said of the product side without a device.

Rule (medpy ``metric.binary.hd``): per class, surface = foreground pixels with a background neighbour among the 4 in-plane (2-D) /
6 (3-D) neighbours, everything outside the array being background; hd2 = the larger of the two directed maxima of the squared
(spacing-scaled) distance to the nearest surface pixel of the other mask; undefined (NaN) when either mask is empty.

Two references: ``hd2_all_pairs`` is the definition, ``hd2_separable`` the column-then-row distance transform (exact integers with
unit spacing), which is what makes the 256 x 256 noise cases affordable."""
import numpy as np
import pytest

_NONE = np.int64(1) << 40


# ------------------------------------------------------------------------------------------------------------- references
def surface(mask):
    """mask: bool [H, W] or [Z, H, W] -> its surface (4- / 6-neighbourhood, outside = background)."""
    p = np.pad(mask, 1, constant_values=False)
    inner = np.ones_like(mask)
    core = tuple(slice(1, -1) for _ in range(mask.ndim))
    for ax in range(mask.ndim):
        for sh in (-1, 1):
            inner &= np.roll(p, sh, axis=ax)[core]
    return mask & ~inner


def _scale(spacing, ndim):
    """None -> exact integers; else float64 weights of the squared index differences, last ndim entries of (sz, sy, sx)."""
    if spacing is None:
        return [np.int64(1)] * ndim, np.int64
    return [np.float64(s) ** 2 for s in tuple(spacing)[-ndim:]], np.float64


def hd2_all_pairs(a, b, spacing=None, chunk=2048):
    """Squared Hausdorff distance of two bool masks by brute force over all pairs of surface pixels; None when undefined."""
    if not a.any() or not b.any():
        return None
    w, dt = _scale(spacing, a.ndim)
    pa, pb = np.argwhere(surface(a)).astype(dt), np.argwhere(surface(b)).astype(dt)
    w = np.array(w, dtype=dt)

    def directed(p, q):
        worst = dt(0)
        for i in range(0, len(p), chunk):
            best = None
            for j in range(0, len(q), chunk):
                d = p[i:i + chunk, None, :] - q[None, j:j + chunk, :]
                m = (d * d * w).sum(-1).min(1)
                best = m if best is None else np.minimum(best, m)
            worst = max(worst, best.max())
        return worst

    return max(directed(pa, pb), directed(pb, pa))


def _column_transform(surf, axis, w, dt):
    """Squared distance along ``axis`` to the nearest surface pixel of the same line (two running scans), _NONE / inf without one."""
    n = surf.shape[axis]
    shape = [1] * surf.ndim
    shape[axis] = n
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    above = np.maximum.accumulate(np.where(surf, idx, -_NONE), axis=axis)
    below = np.flip(np.minimum.accumulate(np.flip(np.where(surf, idx, _NONE), axis), axis=axis), axis)
    d = np.minimum(idx - above, below - idx)
    none = d >= _NONE // 2
    if dt is np.int64:
        return np.where(none, _NONE, d * d)
    return np.where(none, np.inf, (d * d).astype(np.float64) * w)


def _distance_map(surf, spacing):
    """Squared distance to the nearest surface pixel within the same image row, at every x of that row's columns: the transform
    along y (and then z), i.e. everything but the last axis."""
    w, dt = _scale(spacing, surf.ndim)
    g = _column_transform(surf, surf.ndim - 2, w[-2], dt)
    if surf.ndim == 3:
        Z = surf.shape[0]
        z = np.arange(Z, dtype=np.int64)
        dz = ((z[:, None] - z[None, :]) ** 2).astype(dt) * w[0]
        g = (dz[:, :, None, None] + g[None]).min(1)
    return g, w[-1], dt


def hd2_separable(a, b, spacing=None, chunk=4096):
    """The same number by the separable transform: columns (and slices) first, then per surface pixel of the other mask the
    minimum over its row.  Exact integer arithmetic with spacing None."""
    if not a.any() or not b.any():
        return None
    sa, sb = surface(a), surface(b)

    def directed(points_of, target):
        g, wx, dt = _distance_map(target, spacing)
        pts = np.argwhere(points_of)
        xs = np.arange(a.shape[-1], dtype=np.int64)
        worst = dt(0)
        for i in range(0, len(pts), chunk):
            p = pts[i:i + chunk]
            rows = g[tuple(p[:, k] for k in range(a.ndim - 1))]                   # [n, W]
            dx = ((p[:, -1][:, None] - xs[None, :]) ** 2).astype(dt) * wx
            worst = max(worst, (dx + rows).min(1).max())
        return worst

    return max(directed(sa, sb), directed(sb, sa))


def reference_hd2(logits_bhwc, gt_bhw, method3d=False, spacing=None, fn=hd2_separable):
    """float64 [rows, C] as dct_hausdorff defines it (NaN = undefined): argmax with ties to the first class, gt values outside
    [0, C) in no class."""
    logits_bhwc, gt_bhw = np.asarray(logits_bhwc), np.asarray(gt_bhw)
    B, H, W, C = logits_bhwc.shape
    pred = logits_bhwc.argmax(-1)
    out = np.full((1 if method3d else B, C), np.nan)
    for c in range(C):
        P, G = pred == c, gt_bhw == c
        if method3d:
            v = fn(P, G, spacing)
            out[0, c] = np.nan if v is None else float(v)
        else:
            for b in range(B):
                v = fn(P[b], G[b], spacing)
                out[b, c] = np.nan if v is None else float(v)
    return out


def blob_field(rng, B, H, W, C, rounds=6):
    """Smoothed noise [B, H, W, C] fp32: its argmax is a map of blobs a few pixels to tens of pixels across."""
    f = rng.standard_normal((B, H, W, C))
    for _ in range(rounds):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5.0
    return np.ascontiguousarray(f.astype(np.float32))


def blob_pair(rng, H, W, rounds=4):
    """Two bool masks: thresholded smoothed noise (sometimes touching the edges, sometimes in several pieces)."""
    f = blob_field(rng, 2, H, W, 1, rounds)[..., 0]
    return f[0] > np.quantile(f[0], 0.7), f[1] > np.quantile(f[1], 0.6)


# ------------------------------------------------------------------------------------------------------------------ tests
def test_surface_rule_on_hand_built_masks():
    full = np.ones((5, 7), bool)
    frame = np.ones((5, 7), bool)
    frame[1:-1, 1:-1] = False
    assert np.array_equal(surface(full), frame)                      # a full image's surface is its frame
    one = np.zeros((5, 7), bool)
    one[2, 3] = True
    assert np.array_equal(surface(one), one)
    plus = np.zeros((5, 5), bool)
    plus[2, :] = plus[:, 2] = True
    s = plus.copy()
    s[2, 2] = False
    assert np.array_equal(surface(plus), s)                          # 4-neighbourhood: the centre's background diagonals do not count
    blk = np.zeros((5, 5), bool)
    blk[1:4, 1:4] = True
    s = blk.copy()
    s[2, 2] = False
    assert np.array_equal(surface(blk), s)
    vol = np.ones((3, 3, 3), bool)
    s3 = vol.copy()
    s3[1, 1, 1] = False
    assert np.array_equal(surface(vol), s3)


def test_the_two_references_agree_exactly_on_random_blob_pairs():
    rng = np.random.default_rng(7)
    for k in range(20):
        H, W = int(rng.integers(9, 40)), int(rng.integers(9, 40))
        a, b = blob_pair(rng, H, W)
        x, y = hd2_all_pairs(a, b), hd2_separable(a, b)
        assert x is not None and x == y and isinstance(x, np.integer), (k, x, y)
    for k in range(4):                                               # volumes, and float spacing
        a = np.stack([blob_pair(rng, 14, 17)[0] for _ in range(5)])
        b = np.stack([blob_pair(rng, 14, 17)[1] for _ in range(5)])
        assert hd2_all_pairs(a, b) == hd2_separable(a, b)
        sp = (10.0, 1.25, 1.25)
        np.testing.assert_allclose(hd2_all_pairs(a, b, sp), hd2_separable(a, b, sp), rtol=1e-12)
        np.testing.assert_allclose(hd2_all_pairs(a[0], b[0], sp), hd2_separable(a[0], b[0], sp), rtol=1e-12)
    empty = np.zeros((6, 6), bool)
    assert hd2_all_pairs(empty, a[0]) is None and hd2_separable(a[0][:6, :6], empty) is None


def test_hand_values():
    a, b = np.zeros((8, 9), bool), np.zeros((8, 9), bool)
    a[1, 2] = True
    b[6, 8] = True
    assert hd2_all_pairs(a, b) == hd2_separable(a, b) == 25 + 36
    assert hd2_separable(a, a) == 0
    full = np.ones((8, 9), bool)
    assert hd2_separable(full, a) == hd2_all_pairs(full, a) == 6 ** 2 + 6 ** 2      # the frame's far corner (7, 8) from (1, 2)
    np.testing.assert_allclose(hd2_separable(a, b, (1.0, 1.5, 0.75)), (5 * 1.5) ** 2 + (6 * 0.75) ** 2, rtol=1e-14)


def test_references_match_scipy_distance_transform():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for k in range(20):
        a, b = blob_pair(rng, int(rng.integers(9, 40)), int(rng.integers(9, 40)))
        sp = None if k % 2 == 0 else (1.0, 1.5, 0.75)
        sa = a ^ ndi.binary_erosion(a, ndi.generate_binary_structure(2, 1))
        sb = b ^ ndi.binary_erosion(b, ndi.generate_binary_structure(2, 1))
        assert np.array_equal(sa, surface(a)) and np.array_equal(sb, surface(b))
        sampling = None if sp is None else sp[1:]
        da, db = ndi.distance_transform_edt(~sa, sampling=sampling), ndi.distance_transform_edt(~sb, sampling=sampling)
        hd = max(db[sa].max(), da[sb].max())
        for fn in (hd2_all_pairs, hd2_separable):
            assert abs(np.sqrt(float(fn(a, b, sp))) - hd) <= 1e-9, (k, fn.__name__)


def test_meter_rejects_cpu_tensors():
    import torch
    from dct_amd.metrics import HausdorffMeter
    import dct_amd.metrics as M
    assert "HausdorffMeter" in M.__all__
    m = HausdorffMeter(method='2d', C=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 8, 8, dtype=torch.int64))
    (rm, rs), (cm, cs) = m.value()                                   # nothing added: nothing is defined, nothing raises
    assert np.isnan(float(rm)) and cm.shape == (3,) and bool(torch.isnan(cm).all())
    assert m.defined.tolist() == [0, 0, 0]


def test_workspace_size_needs_no_device():
    from dct_amd import _lib
    lib = _lib.load()
    for m3 in (0, 1):
        sizes = [lib.dct_hausdorff_workspace_bytes(B, 256, 256, 4, m3) for B in (1, 2, 8, 16, 64)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.dct_hausdorff_workspace_bytes(10, 256, 256, 4, 1) > lib.dct_hausdorff_workspace_bytes(10, 256, 256, 4, 0)
    # the distance maps alone are 2 sides x C classes x 4 bytes per pixel
    assert lib.dct_hausdorff_workspace_bytes(16, 256, 256, 4, 0) >= 2 * 4 * 4 * 16 * 256 * 256
    assert lib.dct_hausdorff_workspace_bytes(37, 53, 2, 3, 0) > 0
