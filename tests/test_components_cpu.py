"""Largest connected component (include/dct.h ``dct_largest_component``): the scipy reference the GPU tests compare against, checked
here on hand-built maps with known answers, plus what can be said of the product side without a device.

Rule: per row (a slice, or the batch as a volume) and class, components under 4- / 6-connectivity (``full``: 8- / 26-); the largest
is kept, ties to the one whose first pixel in raster order comes first (``np.argmax`` over the sizes of ``scipy.ndimage.label``'s
labels: scipy numbers components in that order); the rest of the class goes to ``background``."""
import inspect

import numpy as np
import pytest
from scipy import ndimage as ndi


def reference_lcc(logits, method3d=False, full=False, classes=None, background=0):
    """logits [B, H, W, C] -> (cleaned class map int64 [B, H, W], stats int32 [rows, C, 3] = components, largest, pixels)."""
    logits = np.asarray(logits)
    B, H, W, C = logits.shape
    cls = logits.argmax(-1).astype(np.int64)
    classes = [c for c in range(C) if c != background] if classes is None else list(classes)
    assert background not in classes
    out = cls.copy()
    rows_in = [cls] if method3d else list(cls)
    rows_out = [out] if method3d else list(out)
    stats = np.zeros((len(rows_in), C, 3), np.int32)
    for r, (m, o) in enumerate(zip(rows_in, rows_out)):
        st = ndi.generate_binary_structure(m.ndim, m.ndim if full else 1)
        for c in range(C):
            lab, n = ndi.label(m == c, structure=st)
            if n == 0:
                continue
            sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            stats[r, c] = (n, sizes.max(), sizes.sum())
            if c in classes:
                o[(m == c) & (lab != 1 + int(np.argmax(sizes)))] = background
    return out, stats


def onehot(cls, C):
    """class map [B, H, W] -> logits whose argmax it is"""
    return (np.asarray(cls)[..., None] == np.arange(C)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ tests
def test_equal_blobs_keep_the_first_in_raster_order():
    m = np.zeros((1, 9, 12), np.int64)
    m[0, 5:7, 1:4] = 1                      # 6 pixels, starts at (5, 1)
    m[0, 1:4, 8:10] = 1                     # 6 pixels, starts at (1, 8): first in raster order
    m[0, 8, 5:8] = 1                        # 3 pixels
    for full in (False, True):
        out, stats = reference_lcc(onehot(m, 2), full=full)
        want = np.zeros_like(m)
        want[0, 1:4, 8:10] = 1
        assert np.array_equal(out, want)
        assert stats[0, 1].tolist() == [3, 6, 15] and stats[0, 0].tolist() == [1, 108 - 15, 108 - 15]


def test_diagonal_chain_is_one_component_only_with_full():
    N = 7
    m = np.zeros((1, N, N), np.int64)
    m[0, np.arange(N), np.arange(N)] = 2
    out, stats = reference_lcc(onehot(m, 3), full=True)
    assert np.array_equal(out, m) and stats[0, 2].tolist() == [1, N, N] and stats[0, 1].tolist() == [0, 0, 0]
    out, stats = reference_lcc(onehot(m, 3), full=False)
    want = np.zeros_like(m)
    want[0, 0, 0] = 2                       # N singletons: the tie rule keeps the first
    assert np.array_equal(out, want) and stats[0, 2].tolist() == [N, 1, N]
    assert stats[0, 0].tolist() == [2, (N * N - N) // 2, N * N - N]      # the diagonal cuts the background in two under 4-connectivity
    # the same chain through a volume: one component with 26 neighbours, N with 6
    v = np.zeros((N, N, N), np.int64)
    v[np.arange(N), np.arange(N), np.arange(N)] = 1
    assert reference_lcc(onehot(v, 2), method3d=True, full=True)[1][0, 1].tolist() == [1, N, N]
    assert reference_lcc(onehot(v, 2), method3d=True, full=False)[1][0, 1].tolist() == [N, 1, N]


def test_classes_and_background_of_the_reference():
    m = np.zeros((1, 6, 10), np.int64)
    m[0, 0, 0:3] = 1; m[0, 3, 0] = 1        # noqa: E702
    m[0, 5, 5:9] = 2; m[0, 0, 9] = 2        # noqa: E702
    out, _ = reference_lcc(onehot(m, 4), classes=[2], background=3)
    want = m.copy()
    want[0, 0, 9] = 3
    assert np.array_equal(out, want)        # class 1 is not listed: its stray pixel stays
    with pytest.raises(AssertionError):
        reference_lcc(onehot(m, 4), classes=[1, 3], background=3)


def test_workspace_size_needs_no_device():
    from dct_amd import _lib
    lib = _lib.load()
    for m3 in (0, 1):
        assert lib.dct_components_workspace_bytes(8, 256, 256, 4, m3) >= 9 * 8 * 256 * 256        # class byte, label and size per pixel
        assert lib.dct_components_workspace_bytes(8, 256, 256, 9, m3) == 0
        assert lib.dct_components_workspace_bytes(1, 1, 1, 1, m3) > 0
        assert lib.dct_components_workspace_bytes(0, 4, 4, 2, m3) == 0
    assert lib.dct_components_workspace_bytes(3, 1 << 15, 1 << 15, 2, 0) > 0                      # a row of 2^30 pixels
    assert lib.dct_components_workspace_bytes(3, 1 << 15, 1 << 15, 2, 1) == 0                     # 3 * 2^30 as one row: labels are 32-bit
    assert lib.dct_components_workspace_bytes(1, 1 << 16, 1 << 15, 2, 0) == 0


def test_component_meter_statistics_on_hand_made_stats():
    import torch
    import dct_amd.metrics as M
    assert "ComponentMeter" in M.__all__ and "keep_largest_component" in M.__all__
    m = M.ComponentMeter(method='2d', C=3)
    (cm, cs), (rm, rs) = m.value()                                   # nothing added: nothing is defined, nothing raises
    assert cm.shape == (3,) and bool(torch.isnan(cm).all()) and bool(torch.isnan(rm).all()) and m.defined.tolist() == [0, 0, 0]
    #                      class 0          class 1        class 2 (never present)
    m.add(torch.tensor([[[1, 90, 90], [3, 6, 10], [0, 0, 0]],
                        [[2, 50, 100], [0, 0, 0], [0, 0, 0]]], dtype=torch.int32))
    m.add(torch.tensor([[[1, 100, 100], [1, 8, 8], [0, 0, 0]]], dtype=torch.int32))
    (cm, cs), (rm, rs) = m.value()
    np.testing.assert_allclose(cm.numpy(), [4 / 3, 2.0, np.nan], rtol=1e-15)
    np.testing.assert_allclose(cs.numpy(), [np.std([1, 2, 1], ddof=1), np.std([3, 1], ddof=1), np.nan], rtol=1e-15)
    np.testing.assert_allclose(rm.numpy(), [0.5 / 3, 0.2, np.nan], rtol=1e-15)
    np.testing.assert_allclose(rs.numpy(), [np.std([0, 0.5, 0], ddof=1), np.std([0.4, 0.0], ddof=1), np.nan], rtol=1e-15)
    assert m.defined.tolist() == [3, 2, 0]
    s = m.summary()
    assert list(s) == ["CC0", "CC1", "CC2", "removed0", "removed1", "removed2"] and s["CC1"] == 2.0 and np.isnan(s["removed2"])
    with pytest.raises(RuntimeError, match="stats"):
        m.add(torch.zeros(2, 4, 3, dtype=torch.int32))
    m.reset()
    assert m.defined.tolist() == [0, 0, 0]


def test_the_filter_rejects_cpu_tensors():
    import torch
    from dct_amd import hip_ops as K
    from dct_amd.metrics import keep_largest_component
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        keep_largest_component(torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.largest_component(torch.zeros(2, 8, 8, 3))


def test_new_arguments_default_to_off():
    from dct_amd import summary
    from dct_amd.trainer import CoTrainer
    p = inspect.signature(summary.summarize).parameters
    assert p["largest_component"].default is None and p["lcc_classes"].default is None and p["lcc_full"].default is False
    assert list(p)[:10] == ["models", "val_dataloader", "device", "ensemble_method", "report_axises", "hausdorff", "spacing", "kappa", "iou",
                            "kappa_classes"]
    assert inspect.signature(CoTrainer.__init__).parameters["val_largest_component"].default is False
