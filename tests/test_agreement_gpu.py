"""``dct_confusion_counts`` / ``AgreementMeter`` / the kappa and IoU tables of ``summary.summarize`` / ``CoTrainer``'s ``val_kappa``
on the GPU, against the numpy references of test_agreement_cpu.py.  Everything the kernel does is integer counting: every count
comparison is ``np.array_equal``.  kappa and IoU are float64 host arithmetic over those integers on both sides, compared at
rtol 1e-12 (the order of the sums differs)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_agreement_cpu import iou_from_matrix, kappa_from_matrix, onehot, pair_list, reference_counts  # noqa: E402
from test_hausdorff_cpu import blob_field  # noqa: E402

DEV = "cuda:0"


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(logits_list, gt):
    from dct_amd import hip_ops as K
    out = K.confusion_counts([dev(l, np.float32) for l in logits_list], dev(gt, np.int64) if gt is not None else None)
    S, (B, C) = len(logits_list), (logits_list[0].shape[0], logits_list[0].shape[-1])
    R = S + (gt is not None)
    assert out.dtype == torch.int32 and tuple(out.shape) == (B, R * (R - 1) // 2, C, C)
    return out.cpu().numpy()


def blob_case(seed, B, H, W, C, S):
    rng = np.random.default_rng(seed)
    return [blob_field(rng, B, H, W, C) for _ in range(S)], blob_field(rng, B, H, W, C).argmax(-1)


def check(logits_list, gt, what=""):
    C = logits_list[0].shape[-1]
    ref = reference_counts(logits_list, gt, C)
    got = run(logits_list, gt)
    print(what, "pairs", ref.shape[1], "non-zero cells", int((ref != 0).sum()), "of", ref.size, "largest", int(ref.max()))
    assert np.array_equal(got, ref), (what, np.argwhere(got != ref)[:10])
    return got


# --------------------------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("B,H,W,C,S", [(3, 37, 53, 3, 2), (2, 5, 7, 4, 1), (1, 1, 1, 2, 2), (4, 200, 200, 2, 2), (8, 256, 256, 4, 2),
                                       (1, 512, 512, 2, 3)])
def test_blobs(B, H, W, C, S):
    """5x7: an image smaller than a wave; 256x256: the eval shape; 512x512: more pixels than one pass of the grid (64 blocks of
    256), so the grid-stride loop runs."""
    logits, gt = blob_case(B * 1000 + W, B, H, W, C, S)
    got = check(logits, gt, f"blobs {B}x{H}x{W}x{C} S={S}")
    for p, (i, j) in enumerate(pair_list(S + 1)):
        if j < S:                                   # a prediction pair counts every pixel
            assert (got[:, p].sum((1, 2)) == H * W).all()


@pytest.mark.parametrize("C", [5, 8])
def test_scalar_load_classes(C):
    logits, gt = blob_case(C, 2, 33, 31, C, 2)
    check(logits, gt, f"C={C}")


def test_eight_models_and_gt_fill_the_histogram():
    """S = 8 with gt at C = 8: P = 36 pairs, the full 9 KiB histogram, on noise."""
    rng = np.random.default_rng(8)
    logits = [rng.standard_normal((2, 24, 24, 8)).astype(np.float32) for _ in range(8)]
    gt = rng.integers(0, 8, (2, 24, 24))
    got = check(logits, gt, "S=8 C=8")
    assert got.shape[1] == 36 and (got != 0).mean() > 0.9


def test_noise_every_lane_another_cell():
    rng = np.random.default_rng(3)
    logits = [rng.standard_normal((4, 128, 128, 4)).astype(np.float32) for _ in range(3)]
    gt = rng.integers(0, 4, (4, 128, 128))
    got = check(logits, gt, "noise")
    assert (got != 0).all()


def test_uniform_batch_lands_in_one_cell():
    B, H, W, C = 2, 96, 80, 4
    logits = [np.full((B, H, W, C), 0.25, np.float32) for _ in range(2)]
    gt = np.zeros((B, H, W), np.int64)
    got = check(logits, gt, "uniform")
    assert (got[:, :, 0, 0] == H * W).all() and got.sum() == B * 3 * H * W


def test_gt_outside_the_classes_is_skipped_by_the_gt_pairs_only():
    B, H, W, C = 3, 40, 36, 3
    logits, clean = blob_case(21, B, H, W, C, 2)
    gt = clean.copy()
    gt[0, :3, :] = 255
    gt[0, 10, 10] = -1
    gt[1, 5:9, 7:30] = C
    gt[1, 20, :] = -1
    gt[2, 39, 35] = 255
    bad = (gt < 0) | (gt >= C)
    got, base = check(logits, gt, "gt with 255 / -1 / C"), check(logits, clean, "clean gt")
    assert np.array_equal(got[:, 0], base[:, 0])                                 # S0 against S1: unchanged
    for p in (1, 2):
        assert np.array_equal(got[:, p].sum((1, 2)), H * W - bad.reshape(B, -1).sum(1))
    all_bad = np.full((B, H, W), 255, np.int64)
    got = check(logits, all_bad, "no valid gt at all")
    assert got[:, 1:].sum() == 0 and (got[:, 0].sum((1, 2)) == H * W).all()


def test_without_gt():
    logits, _ = blob_case(5, 2, 37, 53, 3, 2)
    got = check(logits, None, "gt=None")
    assert got.shape[1] == 1
    logits, _ = blob_case(6, 2, 20, 20, 4, 4)
    assert check(logits, None, "gt=None, S=4").shape[1] == 6


def test_exact_logit_ties_go_to_the_first_class():
    C, H, W = 3, 16, 20
    logits = np.zeros((3, H, W, C), np.float32)          # image 0: all equal everywhere -> class 0 fills the image
    logits[1, 4:9, 5:12, 1] = logits[1, 4:9, 5:12, 2] = 1.0          # image 1: classes 1 and 2 tie above class 0 -> class 1
    logits[2, :, :, 0] = -1.0                                          # image 2: 1 and 2 tie everywhere -> class 1 fills the image
    gt = np.zeros((3, H, W), np.int64)
    gt[1, 4:9, 5:12] = 1
    gt[2] = 1
    got = check([logits, logits[::-1].copy()], gt, "ties")
    sgt = got[:, 1]                                       # S0 against gt: the prediction equals gt on every image
    assert sgt[0, 0, 0] == H * W and sgt[1, 1, 1] == 5 * 7 and sgt[1, 0, 0] == H * W - 35 and sgt[2, 1, 1] == H * W
    assert (sgt.sum((1, 2)) == np.trace(sgt, axis1=1, axis2=2)).all() and sgt[:, :, 2].sum() == 0 and sgt[:, 2, :].sum() == 0


# ------------------------------------------------------------------------------------------------------------- further checks
@pytest.mark.parametrize("C", [3, 4])
def test_gt_pairs_give_back_dice_counts(C):
    from dct_amd import hip_ops as K
    B, H, W = 3, 45, 50
    logits, gt = blob_case(60 + C, B, H, W, C, 2)
    got = run(logits, gt)
    for s in range(2):
        inter, ps, gs = K.dice_counts(dev(logits[s], np.float32).reshape(B, -1, C), dev(gt, np.int64).reshape(B, -1), B, C)
        M = got[:, pair_list(3).index((s, 2))]
        assert np.array_equal(np.diagonal(M, axis1=1, axis2=2), inter.cpu().numpy())
        assert np.array_equal(M.sum(2), ps.cpu().numpy())
        assert np.array_equal(M.sum(1), gs.cpu().numpy())


@pytest.mark.parametrize("C", [3, 2])
def test_views_that_start_inside_their_storage(C):
    """A dense slice of a larger batch is not 16-byte aligned when H * W is odd: the op takes it all the same."""
    from dct_amd import hip_ops as K
    logits, gt = blob_case(4, 3, 15, 13, C, 2)
    lg, g = [dev(l, np.float32) for l in logits], dev(gt, np.int64)
    assert lg[0][1:].data_ptr() % 16 != 0 and lg[0][1:].is_contiguous()
    ref = reference_counts([l[1:] for l in logits], gt[1:], C)
    assert np.array_equal(K.confusion_counts([l[1:] for l in lg], g[1:]).cpu().numpy(), ref)
    # [B, pix, C] and a channels-first view are taken too
    assert np.array_equal(K.confusion_counts([l.reshape(3, -1, C) for l in lg], g.reshape(3, -1))[1:].cpu().numpy(), ref)
    nchw = [l.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) for l in lg]
    assert not nchw[0].is_contiguous()
    assert np.array_equal(K.confusion_counts(nchw, g)[1:].cpu().numpy(), ref)


def test_counts_accumulate():
    from dct_amd import _lib
    from dct_amd import hip_ops as K
    B, H, W, C = 2, 30, 34, 4
    logits, gt = blob_case(7, B, H, W, C, 2)
    lg, g = [dev(l, np.float32) for l in logits], dev(gt, np.int64)
    once = K.confusion_counts(lg, g)
    buf = torch.zeros_like(once)
    for _ in range(2):
        _lib.call("dct_confusion_counts", K._ptr_array(lg), 2, g.data_ptr(), B, H * W, C, buf.data_ptr(), _lib.stream())
    assert torch.equal(buf, 2 * once)


def test_bit_identical_from_run_to_run_and_beside_a_convolution():
    from dct_amd import hip_ops as K
    rng = np.random.default_rng(9)
    B, H, W, C = 4, 128, 128, 4
    lg = [dev(rng.standard_normal((B, H, W, C)), np.float32) for _ in range(2)]
    gt = dev(rng.integers(0, C, (B, H, W)), np.int64)
    a = K.confusion_counts(lg, gt)
    b = K.confusion_counts(lg, gt)
    assert torch.equal(a, b)
    # on a side stream while convolutions run on the current one
    x = torch.randn(4, 128, 128, 64, device=DEV).to(torch.bfloat16)
    w = (torch.randn(64, 3, 3, 64, device=DEV) / 24).to(torch.bfloat16)
    y = torch.empty(4, 128, 128, 64, device=DEV, dtype=torch.bfloat16)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(20):
        K.conv2d(x, w, None, y, R=3, S=3, pad_h=1, pad_w=1)
    with torch.cuda.stream(side):
        c = K.confusion_counts(lg, gt)
    for _ in range(20):
        K.conv2d(x, w, None, y, R=3, S=3, pad_h=1, pad_w=1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(a, c)


def test_status_codes_surface_as_runtime_errors():
    import ctypes
    from dct_amd import _lib
    B, pix = 2, 64
    lg = torch.zeros(B, pix, 9, device=DEV)
    gt = torch.zeros(B, pix, dtype=torch.int64, device=DEV)
    out = torch.zeros(B * 36 * 81, dtype=torch.int32, device=DEV)
    arr = lambda n, first=True: (ctypes.c_void_p * n)(*([lg.data_ptr() if first else None] * min(n, 1) + [lg.data_ptr()] * (n - 1)))   # noqa: E731
    args = lambda **k: [k.get("arr", arr(k.get("S", 2))), k.get("S", 2), k.get("gt", gt.data_ptr()), B, pix, k.get("C", 3),    # noqa: E731
                        k.get("out", out.data_ptr()), _lib.stream()]
    _lib.call("dct_confusion_counts", *args())
    for bad in (dict(arr=None), dict(arr=arr(2, first=False)), dict(out=None), dict(S=1, gt=None), dict(S=0)):
        with pytest.raises(RuntimeError, match=r"status -1"):
            _lib.call("dct_confusion_counts", *args(**bad))
    for bad in (dict(C=9), dict(S=9), dict(C=0)):
        with pytest.raises(RuntimeError, match=r"status -2"):
            _lib.call("dct_confusion_counts", *args(**bad))
    _lib.call("dct_confusion_counts", *args(S=1))              # one model against gt is a pair
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------- meter
def _nan_stats(v):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n = (~np.isnan(v)).sum(0)
        mean = np.nanmean(v, 0)
        std = np.where(n > 1, np.nanstd(v, 0, ddof=1), np.nan)
    return mean, std, n


@pytest.mark.parametrize("method", ["2d", "3d"])
@pytest.mark.parametrize("classes", [None, [1, 2, 3]])
def test_meter_against_numpy_nan_statistics(method, classes):
    from dct_amd.metrics import AgreementMeter
    C, B, H, W = 4, 3, 48, 40
    m = AgreementMeter(method=method, C=C, n_models=2, with_gt=True, considered_classes=classes)
    assert m.pairs == ["S0_S1", "S0_gt", "S1_gt"]
    rows = []
    for k in range(3):
        logits, gt = blob_case(200 + k, B, H, W, C, 2)
        for l in logits:
            l[..., 3] = -10.0                   # class 3 is never predicted
        if k == 1:
            gt[0] = 0                           # one slice's gt is background only: its kappa restricted to 1..3 has no pixel
            if method == "3d":
                gt[:] = 0
        m.add([torch.from_numpy(l).permute(0, 3, 1, 2).to(DEV) for l in logits], torch.from_numpy(gt).unsqueeze(1).to(DEV))
        cnt = reference_counts(logits, gt, C)
        rows.append(cnt.sum(0, keepdims=True) if method == "3d" else cnt)
    ref = np.concatenate(rows)                  # [rows, 3, C, C]
    assert ref.shape[0] == (3 if method == "3d" else 9)
    conf = m.confusion()
    assert conf.dtype == torch.int64 and np.array_equal(conf.numpy(), ref.sum(0))
    kap = np.array([[kappa_from_matrix(M, classes) for M in row] for row in ref])
    if classes is not None:
        assert np.isnan(kap[:, 1:]).sum() == 2 and not np.isnan(kap[:, 0]).any()      # the background-only row, in both gt pairs
    mean, std, n = _nan_stats(kap)
    gm, gs, gn = m.kappa()
    assert gm.dtype == torch.float64
    np.testing.assert_allclose(gm.numpy(), mean, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(gs.numpy(), std, rtol=1e-12, equal_nan=True)
    assert gn.tolist() == n.tolist()
    iou = np.array([[iou_from_matrix(row[p]) for p in (1, 2)] for row in ref])          # [rows, 2, C]
    imean, istd, _ = _nan_stats(iou)
    im, istd_got = m.iou()
    assert tuple(im.shape) == (2, C) and (im[:, 3] == 0).all()        # never predicted, present in gt: IoU 0 where defined
    np.testing.assert_allclose(im.numpy(), imean, rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(istd_got.numpy(), istd, rtol=1e-12, equal_nan=True)
    rmean, rstd, _ = _nan_stats(_nan_stats(kap[:, 1:].T)[0][:, None])
    s, d = m.summary(), m.detailed_summary()
    assert set(s) == {"mKappa", "mVars"} and list(d) == m.pairs
    np.testing.assert_allclose([s["mKappa"], s["mVars"]], [rmean[0], rstd[0]], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose([d[k] for k in m.pairs], mean, rtol=1e-12, equal_nan=True)
    (vm, vs), (pm, _) = m.value()
    assert vm == s["mKappa"] and np.array_equal(pm.numpy(), gm.numpy(), equal_nan=True)
    m.reset()
    assert m.kappa()[2].tolist() == [0, 0, 0] and np.isnan(m.summary()["mKappa"]) and int(m.confusion().sum()) == 0


# ------------------------------------------------------------------------------------------------------- summary / eval loop
def _segmentators(C, n=2):
    from dct_amd.models import Segmentator
    segs = []
    for seed in range(n):
        torch.manual_seed(40 + seed)
        segs.append(Segmentator({"name": "enet", "num_classes": C, "compute_dtype": torch.float32}, {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4},
                                {"name": "StepLR", "step_size": 90, "gamma": 0.1}))
    return segs


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return a == b or (a != a and b != b)


def test_summarize_kappa_and_iou_tables():
    from dct_amd import summary
    from dct_amd.metrics import AgreementMeter
    C, H = 3, 32
    models = _segmentators(C)
    val = FakeLoader(batches(91, 4, 1, H, C), 1)
    plain = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2])
    assert sorted(plain) == ["2d", "3d"]
    res = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2], kappa=True, iou=True, kappa_classes=[1, 2])
    assert sorted(res) == ["2d", "3d", "iou_2d", "iou_3d", "kappa_2d", "kappa_3d"]
    assert _same({k: res[k] for k in ("2d", "3d")}, plain)
    only = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2], kappa=True, kappa_classes=[1, 2])
    assert sorted(only) == ["2d", "3d", "kappa_2d", "kappa_3d"] and _same(only["kappa_2d"], res["kappa_2d"])
    ens = summary.Ensembleway("soft", C)
    names = ["S0", "S1", "ensemble"]
    pairs = ["S0_S1", "S0_ensemble", "S0_gt", "S1_ensemble", "S1_gt", "ensemble_gt"]
    for method in ("2d", "3d"):
        meter = AgreementMeter(method=method, C=C, n_models=3, with_gt=True, considered_classes=[1, 2], rater_names=names)
        with torch.no_grad():
            for (img, gt), _, _ in val:
                preds = [m.predict(img.to(DEV), logit=False) for m in models]
                meter.add(preds + [ens(preds)], gt.to(DEV))
        assert meter.pairs == pairs
        mean, std, n = meter.kappa()
        t = res["kappa_" + method]
        assert list(t) == ["mean", "std", "defined"] and all(list(t[k]) == pairs for k in t)
        assert _same(t["mean"], {k: float(mean[p]) for p, k in enumerate(pairs)})
        assert _same(t["std"], {k: float(std[p]) for p, k in enumerate(pairs)})
        assert t["defined"] == {k: int(n[p]) for p, k in enumerate(pairs)}
        im, istd = meter.iou()
        t = res["iou_" + method]
        assert list(t) == ["model_0", "model_1", "ensemble", "ensemble_std"]
        for i in range(2):
            assert _same(t[f"model_{i}"], {f"IoU{j}": float(im[i][j]) for j in range(C)})
        assert _same(t["ensemble"], {f"IoU{j}": float(im[2][j]) for j in range(C)})
        assert _same(t["ensemble_std"], {f"IoU{j}": float(istd[2][j]) for j in range(C)})
        print(method, res["kappa_" + method], t)


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def add_scalars(self, tag, values, epoch):
        self.calls.append((tag, dict(values), epoch))


def test_eval_loop_uploads_val_kappa_only_on_request(tmp_path):
    from dct_amd import ModelMode
    from dct_amd.loss import get_loss_fn
    from dct_amd.metrics import AgreementMeter
    from dct_amd.trainer import CoTrainer
    C, H = 3, 32
    segs = _segmentators(C)
    val = FakeLoader(batches(95, 3, 2, H, C), 2)
    lab = [FakeLoader(batches(31 + i, 1, 2, H, C), 2) for i in range(2)]
    crit = {"sup": get_loss_fn("cross_entropy"), "jsd": get_loss_fn("jsd"), "adv": get_loss_fn("jsd")}
    kw = dict(max_epoch=1, device=DEV, axises=[1, 2], cot_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.5},
              adv_scheduler_dict={"name": "ConstantScheduler", "begin_epoch": 0, "max_value": 0.05}, adv_training_dict={"eplision": 0.03},
              use_tqdm=False)
    plain = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "a"), **kw)
    withk = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "b"), val_kappa=True, **kw)
    plain.writer, withk.writer = _Recorder(), _Recorder()
    with torch.no_grad():
        a2, a3 = plain._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
        b2, b3 = withk._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
    assert torch.equal(a2, b2) and torch.equal(a3, b3)
    assert not [c for c in plain.writer.calls if c[0].startswith("val_kappa")]
    assert [c for c in plain.writer.calls if c[0].startswith("val_data")] == [c for c in withk.writer.calls if c[0].startswith("val_data")]
    assert [c[0] for c in plain.writer.calls] == [c[0] for c in withk.writer.calls if not c[0].startswith("val_kappa")]
    kap = {c[0]: c[1] for c in withk.writer.calls if c[0].startswith("val_kappa/")}
    assert sorted(kap) == ["val_kappa/S0_S1", "val_kappa/S0_gt", "val_kappa/S1_gt"]
    meter = AgreementMeter(method="3d", C=C, n_models=2, with_gt=True, considered_classes=[1, 2])
    with torch.no_grad():
        for (img, gt), _, _ in val:
            meter.add([seg.predict(img.to(DEV), logit=True) for seg in segs], gt.to(DEV))
    mean = meter.kappa()[0]
    for p, pair in enumerate(meter.pairs):
        assert _same(kap[f"val_kappa/{pair}"], {"kappa": float(mean[p])})
    print(kap)
