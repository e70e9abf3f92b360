"""``dct_largest_component`` / ``keep_largest_component`` / ``ComponentMeter`` / the ``_lcc`` tables of ``summary.summarize`` /
``CoTrainer``'s ``val_lcc`` on the GPU, against the scipy reference of test_components_cpu.py.  Class maps, counts and one-hot floats:
every comparison of the filter's outputs is ``==``, and so is every comparison of a table with the table the same meters give on the
reference's cleaned map.  Only where a table is compared with a number computed on the host (the meter's fp32 square root of an exact
integer hd2, a float64 mean) is there a rounding bound, stated where it is used."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_components_cpu import onehot, reference_lcc  # noqa: E402
from test_hausdorff_cpu import blob_field, reference_hd2  # noqa: E402

DEV = "cuda:0"
SEGMENT = 64        # csrc/components.hip: the initial labels chain inside 64-pixel wave segments of the raster order, blocks hold 4 of them
COMBOS = [(False, False), (False, True), (True, False), (True, True)]       # (method3d, full)


def run(logits, method3d=False, full=False, classes=None, background=0):
    from dct_amd import hip_ops as K
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(DEV)
    oh, cls, stats = K.largest_component(lg, method3d, full, classes, background, want_cls=True)
    B, H, W, C = logits.shape
    assert oh.dtype == torch.float32 and tuple(oh.shape) == (B, H, W, C) and cls.dtype == torch.int64 and tuple(cls.shape) == (B, H, W)
    assert stats.dtype == torch.int32 and tuple(stats.shape) == (1 if method3d else B, C, 3)
    return oh.cpu().numpy(), cls.cpu().numpy(), stats.cpu().numpy()


def check(logits, method3d=False, full=False, classes=None, background=0, ref=None, what=""):
    ref_cls, ref_stats = ref if ref is not None else reference_lcc(logits, method3d, full, classes, background)
    oh, cls, stats = run(logits, method3d, full, classes, background)
    C = logits.shape[-1]
    print(what, "3d" if method3d else "2d", "full" if full else "faces", "components", ref_stats[..., 0].sum(0).tolist(),
          "moved", int((ref_cls != np.asarray(logits).argmax(-1)).sum()))
    assert np.array_equal(stats, ref_stats), (what, stats, ref_stats)
    assert np.array_equal(cls, ref_cls), (what, np.argwhere(cls != ref_cls)[:5])
    assert np.array_equal(oh, onehot(ref_cls, C)), what
    return cls, stats


# ---------------------------------------------------------------------------------------------------------------- blob fields
BLOB_SHAPES = [(2, 37, 53, 3), (4, 64, 64, 4), (3, 40, 700, 2), (6, 48, 40, 4)]


@functools.lru_cache(maxsize=None)
def blob_logits(shape):
    return blob_field(np.random.default_rng(7), *shape)


@functools.lru_cache(maxsize=None)
def blob_reference(shape, method3d, full):
    return reference_lcc(blob_logits(shape), method3d, full)


@pytest.mark.parametrize("method3d,full", COMBOS)
@pytest.mark.parametrize("shape", BLOB_SHAPES)
def test_blob_fields(shape, method3d, full):
    ref = blob_reference(shape, method3d, full)
    present = ref[1][..., 2] > 0
    assert present.any() and (ref[1][..., 0][present] >= 2).all(), ref[1]        # doing nothing cannot pass
    assert (ref[0] != blob_logits(shape).argmax(-1)).any()
    check(blob_logits(shape), method3d, full, ref=ref, what=f"blobs {shape}")


@pytest.mark.parametrize("method3d,full", COMBOS)
def test_iid_noise(method3d, full):
    """Thousands of tiny components, many of equal size below the maximum."""
    logits = np.random.default_rng(3).standard_normal((4, 64, 64, 4)).astype(np.float32)
    _, stats = check(logits, method3d, full, what="noise")
    assert stats[..., 0].sum() > (100 if full and method3d else 4000)       # (p = 1/4 percolates under 26 neighbours: few components there)


# ------------------------------------------------------------------------------------------------------------- hand-built maps
def serpentine(H=33, W=131):
    """One pixel wide, covers the image: full even rows joined alternately at the right and the left end."""
    s = np.zeros((H, W), np.int64)
    s[::2, :] = 1
    for y in range(1, H, 2):
        s[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return s


def hand_built():
    """name -> (class map [B, H, W], C)"""
    cases = {}
    s = serpentine()
    cases["serpentine"] = (np.stack([s, s[::-1].copy(), s[:, ::-1].copy()]), 2)
    u = np.zeros((2, 50, 90), np.int64)
    u[:, :, 3] = 1; u[:, :, 80] = 1; u[:, 49, 3:81] = 1; u[1, 10:14, 40:44] = 1          # noqa: E702  the arms meet in the last row only
    cases["u"] = (u, 2)
    comb = np.zeros((2, 40, 150), np.int64)
    comb[0, :, ::2] = 2; comb[0, 39, :] = 2                                                 # noqa: E702  teeth down to a spine in the last row
    comb[1, :, ::3] = 2; comb[1, 0, :] = 2; comb[1, 20:, 1::3] = 1                          # noqa: E702  spine first; loose teeth of class 1 (ties)
    cases["comb"] = (comb, 3)
    cb = 1 + (np.add.outer(np.arange(20), np.arange(70)) % 2)
    cases["checkerboard"] = (np.stack([cb, 3 - cb, cb]), 3)
    W = 3 * SEGMENT + 5                     # rows start at raster offsets 0, 5, 10, ... inside a segment: a full row crosses three or four borders
    x = np.zeros((2, 9, W), np.int64)
    x[:, 1, :] = 1; x[:, 3, :] = 1; x[:, 2, W - 1] = 1; x[:, 5, :] = 1; x[:, 4, 0] = 1     # noqa: E702  one component over rows 1-5
    x[:, 7, 10:SEGMENT + 20] = 1            # a shorter one that crosses one border
    x[1, :, SEGMENT - 1] = 2; x[1, :, SEGMENT] = 2                                          # noqa: E702  a class-2 bar along a border cuts class 1
    cases["segment_borders"] = (x, 3)
    cases["one_class_fills_the_image"] = (np.ones((3, 40, 300), np.int64), 2)
    a = np.zeros((2, 24, 31), np.int64)
    a[:, 2:6, 3:9] = 1; a[:, 10:14, 20:26] = 1; a[:, 18:22, 2:8] = 1; a[0, 8, 8] = 1       # noqa: E702  three blobs of 24: the first is kept
    a[:, 16:19, 12:15] = 2; a[:, 1:4, 22:25] = 2                                            # noqa: E702  two of 9; class 3 absent
    cases["ties_and_an_absent_class"] = (a, 4)
    b = np.zeros((3, 6, 7), np.int64)
    b[0, 1:3, 1:3] = 1; b[2, 3:5, 3:5] = 1; b[1, 2, 3] = 1                                 # noqa: E702  (0,2,2)-(1,2,3): edge; (1,2,3)-(2,3,3): edge
    b[1, 2, 2] = 0
    cases["bridge_voxel_by_edges"] = (b, 2)
    f = np.zeros((3, 6, 7), np.int64)
    f[0, 1:3, 1:3] = 1; f[2, 2:4, 2:4] = 1; f[1, 2, 2] = 1                                 # noqa: E702  faces: (0,2,2)-(1,2,2)-(2,2,2)
    cases["bridge_voxel_by_faces"] = (f, 2)
    k = np.zeros((2, 6, 6), np.int64)
    k[0, 0:3, 0:3] = 1; k[1, 3:6, 3:6] = 1                                                 # noqa: E702  (0,2,2) and (1,3,3) share a corner only
    cases["corner_across_z"] = (k, 2)
    cases["one_pixel_images"] = (np.array([1, 0, 1, 1]).reshape(4, 1, 1), 2)
    cases["one_column"] = (np.array([[1, 1, 0, 1], [0, 1, 1, 1]]).reshape(2, 4, 1), 2)
    cases["one_row"] = (np.array([[2, 2, 0, 2, 1], [1, 0, 1, 1, 2]]).reshape(2, 1, 5), 3)
    # 40 slices x 3 classes = 120 (row, class) words inside one block's pixels: more than the 64 it combines in LDS
    cases["many_tiny_images"] = (np.random.default_rng(12).integers(0, 3, (40, 2, 3)), 3)
    return cases


@pytest.mark.parametrize("method3d,full", COMBOS)
def test_hand_built_maps(method3d, full):
    got = {}
    for name, (m, C) in hand_built().items():
        got[name] = check(onehot(m, C), method3d, full, what=name)
    if not method3d:
        cls, stats = got["serpentine"]
        n = int(serpentine().sum())
        assert stats[:, 1].tolist() == [[1, n, n]] * 3          # one component, its root hundreds of hops from its last pixel
        assert np.array_equal(cls, hand_built()["serpentine"][0])
        cls, stats = got["checkerboard"]
        if full:                            # one component per class
            assert np.array_equal(cls, hand_built()["checkerboard"][0]) and stats[:, 1:, 0].tolist() == [[1, 1]] * 3
        else:                               # every pixel its own component: the tie rule keeps the first of each class
            want = np.zeros_like(cls)
            want[:, 0, 0] = [1, 2, 1]
            want[:, 0, 1] = [2, 1, 2]
            assert np.array_equal(cls, want) and stats[:, 1:, 0].tolist() == [[700, 700]] * 3 and stats[:, 1:, 1].tolist() == [[1, 1]] * 3
        cls, stats = got["ties_and_an_absent_class"]
        assert stats[0].tolist() == [[1, 31 * 24 - 91, 31 * 24 - 91], [4, 24, 73], [2, 9, 18], [0, 0, 0]]
        assert (cls[:, 2:6, 3:9] == 1).all() and (cls == 1).sum() == 48 and (cls[:, 16:19, 12:15] == 0).all() and (cls[:, 1:4, 22:25] == 2).all()
        assert (got["one_class_fills_the_image"][1][:, 1] == [1, 12000, 12000]).all()
        assert got["one_pixel_images"][0].ravel().tolist() == [1, 0, 1, 1]
    else:
        assert got["bridge_voxel_by_edges"][1][0, 1].tolist() == ([1, 9, 9] if full else [3, 4, 9])
        assert got["bridge_voxel_by_faces"][1][0, 1].tolist() == [1, 9, 9]
        assert got["corner_across_z"][1][0, 1].tolist() == ([1, 18, 18] if full else [2, 9, 18])
        assert (got["corner_across_z"][0][1] == 1).sum() == (9 if full else 0)
        assert got["one_pixel_images"][1][0].tolist() == [[1, 1, 1], [2, 2, 3]]


def test_views_that_start_inside_their_storage():
    """A dense slice of a larger batch is not 16-byte aligned when H * W * C is odd: the op and the filter take it all the same."""
    from dct_amd import hip_ops as K
    from dct_amd.metrics import keep_largest_component
    logits = blob_field(np.random.default_rng(4), 3, 15, 13, 3)
    lg = torch.from_numpy(logits).to(DEV)
    assert lg[1:].data_ptr() % 16 != 0 and lg[1:].is_contiguous()
    ref_cls, ref_stats = reference_lcc(logits[1:])
    oh, cls, stats = K.largest_component(lg[1:], want_cls=True)
    assert np.array_equal(cls.cpu().numpy(), ref_cls) and np.array_equal(stats.cpu().numpy(), ref_stats)
    assert np.array_equal(oh.cpu().numpy(), onehot(ref_cls, 3))
    kept = keep_largest_component(lg.permute(0, 3, 1, 2)[1:])
    assert np.array_equal(kept.permute(0, 2, 3, 1).cpu().numpy(), onehot(ref_cls, 3))


# ----------------------------------------------------------------------------------------------------- classes, background, status
def test_classes_and_background():
    from dct_amd import hip_ops as K
    logits = blob_logits((6, 48, 40, 4))
    for method3d in (False, True):
        before = logits.argmax(-1)
        cls, _ = check(logits, method3d, False, classes=[1, 3], background=2, what="classes [1, 3] -> 2")
        assert np.array_equal(cls == 0, before == 0)                                       # class 0 is not listed: untouched
        moved = cls != before
        assert moved.any() and np.isin(before[moved], [1, 3]).all() and (cls[moved] == 2).all() and (cls[before == 2] == 2).all()
        check(logits, method3d, True, classes=[0], background=3, what="classes [0] -> 3")
        check(logits, method3d, False, classes=[], background=1, what="no class")
    lg = torch.from_numpy(logits).to(DEV)
    with pytest.raises(ValueError, match="background"):
        K.largest_component(lg, classes=[0, 1], background=0)
    with pytest.raises(ValueError):
        K.largest_component(lg, classes=[4])
    with pytest.raises(RuntimeError, match=r"status -2"):
        K.largest_component(torch.zeros(2, 8, 8, 9, device=DEV))


def test_status_codes_through_the_raw_binding():
    from dct_amd import _lib
    B, H, W, C = 2, 16, 16, 3
    lg = torch.zeros(B, H, W, C, device=DEV)
    oh = torch.zeros(B, H, W, C, device=DEV)
    cls = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)
    stats = torch.zeros(B, C, 3, dtype=torch.int32, device=DEV)
    need = _lib.load().dct_components_workspace_bytes(B, H, W, C, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = lambda **k: [k.get("lg", lg.data_ptr()), B, k.get("H", H), W, k.get("C", C), 0, k.get("full", 0), k.get("mask", 0b110),      # noqa: E731
                        k.get("bg", 0), k.get("oh", oh.data_ptr()), k.get("cls", cls.data_ptr()), stats.data_ptr(), ws.data_ptr(),
                        k.get("n", ws.numel()), _lib.stream()]
    _lib.call("dct_largest_component", *args())
    _lib.call("dct_largest_component", *args(oh=None))
    _lib.call("dct_largest_component", *args(cls=None))
    for bad in (dict(lg=None), dict(oh=None, cls=None), dict(H=0), dict(full=2), dict(bg=3), dict(bg=-1), dict(mask=0b111), dict(mask=0b1010),
                dict(lg=lg.data_ptr() + 4), dict(oh=oh.data_ptr() + 8), dict(cls=cls.data_ptr() + 4)):
        with pytest.raises(RuntimeError, match=r"status -1"):
            _lib.call("dct_largest_component", *args(**bad))
    with pytest.raises(RuntimeError, match=r"status -2"):
        _lib.call("dct_largest_component", *args(C=9))
    with pytest.raises(RuntimeError, match=r"status -4"):
        _lib.call("dct_largest_component", *args(n=need - 1))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- reproducible, nothing waits
def test_bit_identical_from_run_to_run():
    from dct_amd import hip_ops as K
    noise = torch.from_numpy(np.random.default_rng(9).standard_normal((4, 64, 64, 4)).astype(np.float32)).to(DEV)
    blobs = torch.from_numpy(blob_logits((6, 48, 40, 4))).to(DEV)
    for lg in (noise, blobs):
        for method3d, full in COMBOS:
            a = K.largest_component(lg, method3d, full, want_cls=True)
            b = K.largest_component(lg, method3d, full, want_cls=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


@pytest.mark.parametrize("method3d", [False, True])
def test_the_call_is_captured_in_a_graph_and_replayed_on_another_input(method3d):
    """Nothing in the call waits for the device or asks it anything: it records into a graph, and the replay cleans whatever the
    captured input buffer then holds (the workspace is cleared by the launches themselves)."""
    from dct_amd import hip_ops as K
    first, second = blob_logits((6, 48, 40, 4)), blob_field(np.random.default_rng(21), 6, 48, 40, 4)
    buf = torch.from_numpy(first).to(DEV)
    K.largest_component(buf, method3d, True, want_cls=True)                  # warm-up: code objects loaded, nothing left to do lazily
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oh, cls, stats = K.largest_component(buf, method3d, True, want_cls=True)
    buf.copy_(torch.from_numpy(second))
    graph.replay()
    torch.cuda.synchronize()
    ref_cls, ref_stats = reference_lcc(second, method3d, True)
    assert np.array_equal(cls.cpu().numpy(), ref_cls) and np.array_equal(stats.cpu().numpy(), ref_stats)
    assert np.array_equal(oh.cpu().numpy(), onehot(ref_cls, 4))
    assert not np.array_equal(ref_cls, blob_reference((6, 48, 40, 4), method3d, True)[0])


# -------------------------------------------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("method", ["2d", "3d"])
def test_filter_in_front_of_the_meters(method):
    """bf16, NCHW-contiguous input; the cleaned map gives every meter exactly what the reference's cleaned map gives it."""
    from dct_amd.metrics import AgreementMeter, DiceMeter, HausdorffMeter, keep_largest_component
    C, shape = 4, (6, 48, 40, 4)
    rng = np.random.default_rng(17)
    pred = torch.from_numpy(blob_field(rng, *shape)).permute(0, 3, 1, 2).contiguous().to(DEV).to(torch.bfloat16)
    other = torch.from_numpy(blob_field(rng, *shape)).permute(0, 3, 1, 2).contiguous().to(DEV)
    gt = torch.from_numpy(blob_field(rng, *shape).argmax(-1)).unsqueeze(1).to(DEV)
    assert pred.is_contiguous() and pred.dtype == torch.bfloat16
    kept, stats = keep_largest_component(pred, method=method, return_stats=True)
    assert kept.dtype == torch.float32 and tuple(kept.shape) == tuple(pred.shape) and kept.permute(0, 2, 3, 1).is_contiguous()
    as_f32 = pred.float().permute(0, 2, 3, 1).cpu().numpy()
    ref_cls, ref_stats = reference_lcc(as_f32, method == "3d", False)
    assert (ref_cls != as_f32.argmax(-1)).any() and np.array_equal(stats.cpu().numpy(), ref_stats)
    want = torch.from_numpy(onehot(ref_cls, C)).permute(0, 3, 1, 2).to(DEV)
    assert torch.equal(kept, want)
    assert torch.equal(keep_largest_component(pred, method=method), kept)
    for make in (lambda: DiceMeter(method=method, C=C), lambda: HausdorffMeter(method=method, C=C)):
        a, b = make(), make()
        a.add(kept, gt)
        b.add(want, gt)
        assert torch.equal(torch.nan_to_num(a.log, nan=-1.0), torch.nan_to_num(b.log, nan=-1.0))
    a, b = AgreementMeter(method=method, C=C, n_models=2), AgreementMeter(method=method, C=C, n_models=2)
    a.add([kept, other], gt)
    b.add([want, other], gt)
    assert torch.equal(a.confusion(), b.confusion())
    full = keep_largest_component(pred, method=method, classes=[1, 2], background=3, full_connectivity=True)
    assert np.array_equal(full.permute(0, 2, 3, 1).cpu().numpy(), onehot(reference_lcc(as_f32, method == "3d", True, [1, 2], 3)[0], C))


def test_component_meter_on_device_stats():
    from dct_amd import hip_ops as K
    from dct_amd.metrics import ComponentMeter
    logits = blob_logits((6, 48, 40, 4)).copy()
    logits[..., 3] = -10.0                      # class 3 is never predicted
    m = ComponentMeter(method='2d', C=4)
    lg = torch.from_numpy(logits).to(DEV)
    m.add(K.largest_component(lg[:4])[2])
    m.add(K.largest_component(lg[4:])[2])
    st = reference_lcc(logits)[1].astype(np.float64)
    (cm, cs), (rm, rs) = m.value()
    np.testing.assert_allclose(cm.numpy()[:3], st[:, :3, 0].mean(0), rtol=1e-14)
    np.testing.assert_allclose(cs.numpy()[:3], st[:, :3, 0].std(0, ddof=1), rtol=1e-12)
    np.testing.assert_allclose(rm.numpy()[:3], ((st[:, :3, 2] - st[:, :3, 1]) / st[:, :3, 2]).mean(0), rtol=1e-14)
    assert np.isnan(cm.numpy()[3]) and np.isnan(rm.numpy()[3]) and m.defined.tolist() == [6, 6, 6, 0]


# ------------------------------------------------------------------------------------------------------------ summary / eval loop
class FixedModel(object):
    """Stands in for a Segmentator in ``summarize``: the k-th call of ``predict`` returns the k-th of a fixed list of predictions."""

    def __init__(self, preds, C):
        self.preds, self.calls, self.arch_params = preds, 0, {"num_classes": C}

    def to(self, device):
        return self

    def eval(self):
        return self

    def predict(self, img, logit=False):
        self.calls += 1
        return self.preds[(self.calls - 1) % len(self.preds)].to(img.device)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return a == b or (a != a and b != b)


def _nchw(logits_bhwc):
    return torch.from_numpy(np.ascontiguousarray(logits_bhwc)).permute(0, 3, 1, 2).contiguous()


def test_summarize_lcc_tables():
    from dct_amd import summary
    C, n, B, H, W = 3, 3, 4, 32, 40
    rng = np.random.default_rng(33)
    fields = [[blob_field(rng, B, H, W, C) for _ in range(n)] for _ in range(2)]
    val = FakeLoader(batches(91, n, B, H, C, W), B)
    kw = dict(report_axises=[1, 2], hausdorff=True, kappa=True, iou=True)
    models = lambda fs: [FixedModel([_nchw(f) for f in per_model], C) for per_model in fs]       # noqa: E731
    plain = summary.summarize(models(fields), val, DEV, "soft", **kw)
    res = summary.summarize(models(fields), val, DEV, "soft", largest_component='3d', **kw)
    base = ["2d", "3d", "hd_2d", "hd_3d", "kappa_2d", "kappa_3d", "iou_2d", "iou_3d"]
    assert sorted(plain) == sorted(base) and sorted(res) == sorted(base + [b + "_lcc" for b in base] + ["components"])
    assert _same({k: res[k] for k in plain}, plain)
    # the same tables from reference-cleaned predictions: the soft vote of the raw predictions is cleaned, not re-voted
    votes = [(fields[0][k] + fields[1][k]) / 2 for k in range(n)]
    cleaned = [[onehot(reference_lcc(f, True, False)[0], C) for f in per_model] for per_model in fields + [votes]]
    ref = summary.summarize(models(cleaned[:2]), val, DEV, "soft", **kw)
    for b in ("2d", "3d", "hd_2d", "hd_3d"):
        for who in ("model_0", "model_1"):
            assert _same(res[b + "_lcc"][who], ref[b][who]), (b, who)
    ens = summary.summarize(models([cleaned[2]]), val, DEV, "soft", **kw)      # a single model: the vote is its prediction
    for b in ("2d", "3d", "hd_2d", "hd_3d", "iou_2d", "iou_3d"):
        assert _same(res[b + "_lcc"]["ensemble"], ens[b]["ensemble"]) and _same(res[b + "_lcc"]["ensemble_std"], ens[b]["ensemble_std"]), b
    for b in ("kappa_2d", "kappa_3d"):
        assert res[b + "_lcc"]["mean"]["ensemble_gt"] == ens[b]["mean"]["S0_gt"]
        assert res[b + "_lcc"]["mean"]["S0_gt"] == ref[b]["mean"]["S0_gt"] and res[b + "_lcc"]["mean"]["S0_S1"] == ref[b]["mean"]["S0_S1"]
    assert list(res["components"]) == ["model_0", "model_1", "ensemble"]
    for who, per_model in zip(res["components"], fields + [votes]):
        st = np.concatenate([reference_lcc(f, True, False)[1] for f in per_model]).astype(np.float64)
        want = {f"CC{j}": st[:, j, 0].mean() for j in range(C)}
        want.update({f"removed{j}": ((st[:, j, 2] - st[:, j, 1]) / st[:, j, 2]).mean() for j in range(C)})
        assert list(res["components"][who]) == list(want)
        np.testing.assert_allclose(list(res["components"][who].values()), list(want.values()), rtol=1e-14)
    two = summary.summarize(models(fields), val, DEV, "soft", report_axises=[1, 2], largest_component='2d', lcc_classes=[2], lcc_full=True)
    assert sorted(two) == ["2d", "2d_lcc", "3d", "3d_lcc", "components"]
    ref2 = summary.summarize(models([[onehot(reference_lcc(f, False, True, [2], 0)[0], C) for f in fields[0]]]), val, DEV, "soft", report_axises=[1, 2])
    assert _same(two["2d_lcc"]["model_0"], ref2["2d"]["model_0"]) and _same(two["3d_lcc"]["model_0"], ref2["3d"]["model_0"])


def test_a_planted_pixel_sets_the_hausdorff_distance_and_the_filter_removes_it():
    """The reason the filter exists: one stray pixel of class 1 far from the organ IS the Hausdorff distance of the raw prediction."""
    from dct_amd import summary
    C, H, W = 3, 48, 64
    rng = np.random.default_rng(41)
    field = blob_field(rng, 1, H, W, C)
    clean = reference_lcc(field)[0]                                     # every foreground class in one piece
    gt = reference_lcc(field + 0.02 * rng.standard_normal(field.shape).astype(np.float32))[0]     # a gt a few pixels off the prediction
    ys, xs = np.nonzero((clean[0] == 1) | (gt[0] == 1))
    far = max(((y, x) for y in range(H) for x in range(W) if clean[0, y, x] == 0),
              key=lambda p: ((ys - p[0]) ** 2 + (xs - p[1]) ** 2).min())
    gy, gx = np.nonzero(gt[0] == 1)
    d_planted = np.sqrt(((gy - far[0]) ** 2 + (gx - far[1]) ** 2).min())
    planted = clean.copy()
    planted[0][far] = 1
    assert np.array_equal(reference_lcc(onehot(planted, C))[0], clean) and (clean == 1).sum() > 1
    val = FakeLoader([[[torch.zeros(1, 1, H, W), torch.from_numpy(gt).unsqueeze(1)], None, ["s"]]], 1)
    run_ = lambda m, **k: summary.summarize([FixedModel([_nchw(onehot(m, C))], C)], val, DEV, "soft", hausdorff=True, **k)     # noqa: E731
    unplanted = run_(clean)["hd_2d"]["model_0"]
    res = run_(planted, largest_component='2d')
    hd_ref = np.sqrt(reference_hd2(onehot(clean, C), gt)[0, 1])
    print("planted at", far, "distance", d_planted, "hd_2d", res["hd_2d"]["model_0"]["HD1"], "hd_2d_lcc", res["hd_2d_lcc"]["model_0"]["HD1"])
    # (the tables hold the meter's fp32 square root of the exact integer hd2: 1e-6 covers its rounding, nothing else is rounded)
    assert d_planted > 2 * hd_ref and res["hd_2d"]["model_0"]["HD1"] >= d_planted * (1 - 1e-6)
    assert _same(res["hd_2d_lcc"]["model_0"], unplanted) and abs(res["hd_2d_lcc"]["model_0"]["HD1"] - hd_ref) <= 1e-6 * hd_ref
    assert res["components"]["model_0"]["CC1"] == 2.0


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def add_scalars(self, tag, values, epoch):
        self.calls.append((tag, dict(values), epoch))


def test_eval_loop_uploads_val_lcc_only_on_request(tmp_path):
    from dct_amd import ModelMode
    from dct_amd.loss import get_loss_fn
    from dct_amd.metrics import DiceMeter, HausdorffMeter, keep_largest_component
    from dct_amd.models import Segmentator
    from dct_amd.trainer import CoTrainer
    C, H = 3, 32
    segs = []
    for seed in range(2):
        torch.manual_seed(40 + seed)
        segs.append(Segmentator({"name": "enet", "num_classes": C, "compute_dtype": torch.float32}, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                                {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    val = FakeLoader(batches(95, 3, 2, H, C), 2)
    lab = [FakeLoader(batches(31 + i, 1, 2, H, C), 2) for i in range(2)]
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    kw = dict(max_epoch=1, device=DEV, axises=[1, 2], cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
              adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05}, adv_training_dict={"eplision": 0.03},
              use_tqdm=False)
    plain = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "a"), **kw)
    lcc = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "b"), val_largest_component=True, **kw)
    both = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "c"), val_largest_component=True, val_hausdorff=True, **kw)
    plain.writer, lcc.writer, both.writer = _Recorder(), _Recorder(), _Recorder()
    with torch.no_grad():
        a2, a3 = plain._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
        b2, b3 = lcc._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
        c2, c3 = both._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
    assert torch.equal(a2, b2) and torch.equal(a3, b3) and torch.equal(a2, c2) and torch.equal(a3, c3)
    tags = lambda t: sorted({c[0].split("/")[0] for c in t.writer.calls})       # noqa: E731
    assert tags(plain) == ["val_data"] and tags(lcc) == ["val_data", "val_lcc"] and tags(both) == ["val_data", "val_hd", "val_hd_lcc", "val_lcc"]
    assert [c for c in plain.writer.calls if c[0].startswith("val_data")] == [c for c in lcc.writer.calls if c[0].startswith("val_data")]
    up = {c[0]: c[1] for c in both.writer.calls}
    assert {c[0]: c[1] for c in lcc.writer.calls if c[0].startswith("val_lcc/")} == {k: v for k, v in up.items() if k.startswith("val_lcc/")}
    for i, seg in enumerate(segs):
        dice, hd = DiceMeter(method="3d", report_axises=[1, 2], C=C), HausdorffMeter(method="3d", report_axises=[1, 2], C=C)
        with torch.no_grad():
            for (img, gt), _, _ in val:
                kept = keep_largest_component(seg.predict(img.to(DEV), logit=True), method="3d", classes=[1, 2])
                dice.add(kept, gt.to(DEV))
                hd.add(kept, gt.to(DEV))
        assert _same(up[f"val_lcc/S{i}"], {f"DSC{n}": float(dice.value()[1][0][n]) for n in (1, 2)})
        assert _same(up[f"val_hd_lcc/S{i}"], {f"HD{n}": float(hd.value()[1][0][n]) for n in (1, 2)})
