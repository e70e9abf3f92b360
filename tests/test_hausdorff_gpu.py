"""``dct_hausdorff`` / ``HausdorffMeter`` / the Hausdorff tables of ``summary.summarize`` / ``CoTrainer``'s ``val_hd`` on the GPU,
against the numpy references of test_hausdorff_cpu.py.  With unit spacing the kernel works on integers below 2^24 in fp32, so the
comparison is ``==``; with real spacing each candidate squared distance is at most three rounded products and two rounded sums in
fp32 (< 8 * 2^-24 ~ 5e-7 relative), so the bound against float64 is 1e-6 on hd2."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import FakeLoader, batches  # noqa: E402
from test_hausdorff_cpu import blob_field, hd2_all_pairs, reference_hd2  # noqa: E402

DEV = "cuda:0"


def run(logits, gt, method3d=False, spacing=(1., 1., 1.)):
    from dct_amd import hip_ops as K
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(DEV)
    g = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.int64)).to(DEV)
    out = K.hausdorff(lg, g, method3d, spacing)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1 if method3d else logits.shape[0], logits.shape[3])
    return out.cpu().numpy()


def check_exact(got, ref, what=""):
    print(what, "defined", int((~np.isnan(ref)).sum()), "of", ref.size, "max hd2", np.nanmax(ref) if (~np.isnan(ref)).any() else None)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok].astype(np.float64), ref[ok]), (what, got, ref)


def onehot(cls, C):
    """class map [B, H, W] -> logits whose argmax it is"""
    return (np.asarray(cls)[..., None] == np.arange(C)).astype(np.float32)


def blob_case(seed, B, H, W, C):
    rng = np.random.default_rng(seed)
    return blob_field(rng, B, H, W, C), blob_field(rng, B, H, W, C).argmax(-1)


# ------------------------------------------------------------------------------------------------------ exact, unit spacing, 2-D
@pytest.mark.parametrize("B,H,W,C", [(8, 256, 256, 4), (4, 200, 200, 2), (2, 37, 53, 3)])
def test_2d_blobs_exact(B, H, W, C):
    logits, gt = blob_case(B * 1000 + W, B, H, W, C)
    ref = reference_hd2(logits, gt)
    assert (~np.isnan(ref)).sum() >= ref.size // 2
    check_exact(run(logits, gt), ref, f"blobs {B}x{H}x{W}x{C}")


def test_2d_rows_wider_than_one_block():
    """W > 256: a thread of the row pass stands on up to four pixels (x, x + 256, ...), up to the 1024 the ABI accepts."""
    for seed, shape in ((1, (1, 40, 700, 2)), (2, (2, 12, 1024, 3)), (3, (1, 1024, 9, 2))):
        logits, gt = blob_case(seed, *shape)
        ref = reference_hd2(logits, gt)
        assert not np.isnan(ref).all()
        check_exact(run(logits, gt), ref, f"wide {shape}")


def test_views_that_start_inside_their_storage():
    """A dense slice of a larger batch is not 16-byte aligned when H * W is odd: the op and the meter take it all the same."""
    from dct_amd import hip_ops as K
    from dct_amd.metrics import HausdorffMeter
    logits, gt = blob_case(4, 3, 15, 13, 3)
    lg, g = torch.from_numpy(logits).to(DEV), torch.from_numpy(gt).to(DEV)
    assert lg[1:].data_ptr() % 16 != 0 and lg[1:].is_contiguous()
    ref = reference_hd2(logits[1:], gt[1:])
    check_exact(K.hausdorff(lg[1:], g[1:]).cpu().numpy(), ref, "offset view")
    m = HausdorffMeter(method='2d', C=3)
    m.add(lg.permute(0, 3, 1, 2)[1:], g.unsqueeze(1)[1:])
    np.testing.assert_allclose(m.log.cpu().numpy(), np.sqrt(ref), rtol=1e-6, equal_nan=True)


def test_2d_small_case_against_all_pairs():
    logits, gt = blob_case(5, 2, 37, 53, 3)
    check_exact(run(logits, gt), reference_hd2(logits, gt, fn=hd2_all_pairs), "all pairs")


def test_2d_noise_exact():
    """i.i.d. logits and labels: about half of all pixels are surface pixels (an untrained network's predictions)."""
    rng = np.random.default_rng(3)
    B, H, W, C = 16, 256, 256, 4
    logits = rng.standard_normal((B, H, W, C)).astype(np.float32)
    gt = rng.integers(0, C, (B, H, W))
    ref = reference_hd2(logits, gt)
    assert not np.isnan(ref).any()
    check_exact(run(logits, gt), ref, "noise")


def test_2d_hand_built_maps():
    C, H, W = 4, 24, 31
    z = lambda: np.zeros((H, W), np.int64)      # noqa: E731
    cases = {}
    a = z(); a[5:12, 7:20] = 1; a[15:20, 3:9] = 2
    cases["identical"] = (a, a.copy())
    p, g = z(), z(); p[3, 4] = 1; g[20, 29] = 1
    cases["pixel_vs_pixel"] = (p, g)
    p, g = z() + 1, z() + 1
    cases["both_fill_the_image"] = (p, g)
    p, g = z() + 1, z(); g[11, 17] = 1
    cases["full_vs_pixel"] = (p, g)
    p, g = z(), z()
    p[0, 0] = p[0, W - 1] = p[H - 1, 0] = p[H - 1, W - 1] = 1          # the four corners
    g[0, 5:20] = 1; g[H - 1, 8:12] = 1; g[4:19, 0] = 1; g[6:9, W - 1] = 1   # one run on each edge
    p[0, 10:14] = 2; g[H - 3:, W - 4:] = 2                            # class 2: top edge against the bottom-right corner block
    cases["edges_and_corners"] = (p, g)
    p, g = z(), z(); p[2:9, 2:9] = 1; g[4:14, 4:14] = 2                # 1 absent from gt, 2 absent from the prediction, 3 from both
    cases["absent_classes"] = (p, g)
    p, g = z(), z(); p[6:16, 6:16] = 1; g[5:15, 8:18] = 1; g[0:3, :] = 255; g[10, 10] = 255; g[20:, 20:] = 7
    cases["gt_holds_255"] = (p, g)
    names = list(cases)
    pred = np.stack([cases[n][0] for n in names])
    gt = np.stack([cases[n][1] for n in names])
    logits = onehot(pred, C)
    ref = reference_hd2(logits, gt)
    got = run(logits, gt)
    check_exact(got, ref, "hand-built")
    k = {n: i for i, n in enumerate(names)}
    assert got[k["identical"], 0] == 0 and got[k["identical"], 1] == 0 and got[k["identical"], 2] == 0 and np.isnan(got[k["identical"], 3])
    assert got[k["pixel_vs_pixel"], 1] == 17 ** 2 + 25 ** 2
    assert got[k["both_fill_the_image"], 1] == 0 and np.isnan(got[k["both_fill_the_image"], 0])
    assert got[k["full_vs_pixel"], 1] == max(11, H - 1 - 11) ** 2 + max(17, W - 1 - 17) ** 2      # the frame's farthest corner
    assert np.isnan(got[k["absent_classes"], 1:]).all() and not np.isnan(got[k["absent_classes"], 0])
    assert not np.isnan(got[k["gt_holds_255"], :2]).any() and np.isnan(got[k["gt_holds_255"], 2:]).all()


def test_exact_logit_ties_go_to_the_first_class():
    C, H, W = 3, 16, 20
    logits = np.zeros((3, H, W, C), np.float32)          # image 0: all equal everywhere -> class 0 fills the image
    logits[1, 4:9, 5:12, 1] = logits[1, 4:9, 5:12, 2] = 1.0          # image 1: classes 1 and 2 tie above class 0 -> class 1
    logits[2, :, :, 0] = -1.0                                          # image 2: 1 and 2 tie everywhere -> class 1 fills the image
    gt = np.zeros((3, H, W), np.int64)
    gt[1, 4:9, 5:12] = 1
    gt[2] = 1
    got = run(logits, gt)
    check_exact(got, reference_hd2(logits, gt), "ties")
    assert got[0, 0] == 0 and np.isnan(got[0, 1:]).all()
    assert got[1, 0] == 0 and got[1, 1] == 0 and np.isnan(got[1, 2])
    assert got[2, 1] == 0 and np.isnan(got[2, 0]) and np.isnan(got[2, 2])


# --------------------------------------------------------------------------------------------------------------------------- 3-D
def test_3d_blobs_exact():
    logits, gt = blob_case(77, 10, 256, 256, 4)
    ref = reference_hd2(logits, gt, method3d=True)
    assert not np.isnan(ref).any()
    check_exact(run(logits, gt, method3d=True), ref, "3-D blobs")


def test_3d_hand_built():
    C, B, H, W = 2, 3, 24, 24
    pred, gt = np.zeros((B, H, W), np.int64), np.zeros((B, H, W), np.int64)
    pred[:, 4:12, 4:12] = 1                     # a column through all three slices (its middle slice has an interior)
    gt[1, 15:18, 16:22] = 1                     # a structure present in one slice only
    logits = onehot(pred, C)
    ref = reference_hd2(logits, gt, method3d=True)
    check_exact(run(logits, gt, method3d=True), ref, "3-D hand-built")
    check_exact(run(logits, gt, method3d=True), reference_hd2(logits, gt, method3d=True, fn=hd2_all_pairs), "3-D hand-built, all pairs")
    # the slice-wise view differs: in 2-D slices 0 and 2 have no gt structure at all
    got2 = run(logits, gt)
    assert np.isnan(got2[0, 1]) and np.isnan(got2[2, 1]) and not np.isnan(got2[1, 1])
    only3 = np.zeros((B, H, W), np.int64)
    only3[1, 5:10, 5:10] = 1                    # a full block in the middle slice only: every pixel of it is 3-D surface
    got = run(onehot(only3, C), only3, method3d=True)
    assert got[0, 1] == 0 and got[0, 0] == 0


@pytest.mark.parametrize("method3d,spacing,shape", [(True, (10., 1.25, 1.25), (6, 96, 80, 3)), (False, (1., 1.5, 0.75), (4, 120, 100, 4))])
def test_spacing_against_float64(method3d, spacing, shape):
    logits, gt = blob_case(31 + shape[0], *shape)
    ref = reference_hd2(logits, gt, method3d=method3d, spacing=spacing)
    got = run(logits, gt, method3d=method3d, spacing=spacing)
    print("spacing", spacing, "max relative error", np.nanmax(np.abs(got - ref) / ref))
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and (~np.isnan(ref)).sum() >= ref.size // 2
    ok = ~np.isnan(ref)
    assert np.all(np.abs(got[ok] - ref[ok]) <= 1e-6 * ref[ok]), (got, ref)
    if not method3d:                            # 2-D ignores sz
        assert np.array_equal(run(logits, gt, spacing=(7.0,) + spacing[1:]), got, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------- determinism
def test_bit_identical_from_run_to_run_and_beside_a_convolution():
    from dct_amd import hip_ops as K
    rng = np.random.default_rng(9)
    B, H, W, C = 8, 256, 256, 4
    lg = torch.from_numpy(rng.standard_normal((B, H, W, C)).astype(np.float32)).to(DEV)
    gt = torch.from_numpy(rng.integers(0, C, (B, H, W))).to(DEV)
    for m3 in (False, True):
        a = K.hausdorff(lg, gt, m3)
        b = K.hausdorff(lg, gt, m3)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
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
            c = K.hausdorff(lg, gt, m3)
        for _ in range(20):
            K.conv2d(x, w, None, y, R=3, S=3, pad_h=1, pad_w=1)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes_surface_as_runtime_errors():
    from dct_amd import _lib
    B, H, W, C = 2, 16, 16, 3
    lg = torch.zeros(B, H, W, 9, device=DEV)
    gt = torch.zeros(B, H, W, dtype=torch.int64, device=DEV)
    out = torch.zeros(B, 9, device=DEV)
    need = _lib.load().dct_hausdorff_workspace_bytes(B, H, W, C, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = lambda **k: [k.get("lg", lg.data_ptr()), gt.data_ptr(), B, H, W, k.get("C", C), 0, 1.0, k.get("sy", 1.0), 1.0,     # noqa: E731
                        out.data_ptr(), ws.data_ptr(), k.get("n", ws.numel()), _lib.stream()]
    _lib.call("dct_hausdorff", *args())
    with pytest.raises(RuntimeError, match=r"status -1"):
        _lib.call("dct_hausdorff", *args(lg=None))
    with pytest.raises(RuntimeError, match=r"status -1"):
        _lib.call("dct_hausdorff", *args(sy=0.0))
    with pytest.raises(RuntimeError, match=r"status -2"):
        _lib.call("dct_hausdorff", *args(C=9))
    with pytest.raises(RuntimeError, match=r"status -4"):
        _lib.call("dct_hausdorff", *args(n=need - 1))
    torch.cuda.synchronize()
    assert _lib.load().dct_hausdorff_workspace_bytes(2, 2048, 16, 3, 0) == 0 and _lib.load().dct_hausdorff_workspace_bytes(257, 16, 16, 3, 1) == 0


# ------------------------------------------------------------------------------------------------------------------------- meter
def _nan_stats(v):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        n = (~np.isnan(v)).sum(0)
        mean = np.nanmean(v, 0)
        std = np.where(n > 1, np.nanstd(v, 0, ddof=1), np.nan)
    return mean, std, n


@pytest.mark.parametrize("method", ["2d", "3d"])
def test_meter_against_numpy_nan_statistics(method):
    from dct_amd.metrics import HausdorffMeter
    C, axes = 4, [1, 2, 3]
    m = HausdorffMeter(method=method, report_axises=axes, C=C)
    rows = []
    for k in range(3):
        logits, gt = blob_case(200 + k, 3, 48, 40, C)
        logits[..., 3] = -10.0                  # class 3 is never predicted: undefined everywhere
        if k == 1:
            gt[0][gt[0] == 2] = 0               # and class 2 is missing from one slice's gt
        m.add(torch.from_numpy(logits).permute(0, 3, 1, 2).to(DEV), torch.from_numpy(gt).unsqueeze(1).to(DEV))
        rows.append(np.sqrt(reference_hd2(logits, gt, method3d=method == "3d")))
    ref = np.concatenate(rows)
    assert tuple(m.log.shape) == ref.shape
    np.testing.assert_allclose(m.log.cpu().numpy(), ref, rtol=1e-6, equal_nan=True)
    mean, std, n = _nan_stats(ref)
    rmean, rstd, _ = _nan_stats(_nan_stats(ref[:, axes].T)[0][:, None])
    (gm, gs), (cm, cs) = m.value()
    np.testing.assert_allclose(cm.numpy(), mean, rtol=1e-6, equal_nan=True)
    np.testing.assert_allclose(cs.numpy(), std, rtol=1e-6, equal_nan=True)
    np.testing.assert_allclose([float(gm), float(gs)], [rmean[0], rstd[0]], rtol=1e-6, equal_nan=True)
    assert m.defined.tolist() == n.tolist() and n[3] == 0 and np.isnan(float(cm[3])) and np.isnan(float(cs[3]))
    s, d = m.summary(), m.detailed_summary()
    assert set(s) == {"mHD", "mVars"} and list(d) == [f"HD{j}" for j in range(C)]
    np.testing.assert_allclose([s["mHD"], s["mVars"]], [rmean[0], rstd[0]], rtol=1e-6, equal_nan=True)
    np.testing.assert_allclose([d[f"HD{j}"] for j in range(C)], mean, rtol=1e-6, equal_nan=True)
    m.reset()
    assert m.defined.tolist() == [0] * C and np.isnan(m.summary()["mHD"]) and bool(torch.isnan(m.log).all())


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


def test_summarize_hausdorff_tables():
    from dct_amd import summary
    from dct_amd.metrics import HausdorffMeter
    C, H = 3, 32
    models = _segmentators(C)
    val = FakeLoader(batches(91, 4, 1, H, C), 1)
    plain = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2])
    again = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2])
    assert sorted(plain) == ["2d", "3d"] and _same(plain, again)
    sp = (2.0, 1.5, 1.0)
    res = summary.summarize(models, val, DEV, "soft", report_axises=[1, 2], hausdorff=True, spacing=sp)
    assert sorted(res) == ["2d", "3d", "hd_2d", "hd_3d"]
    assert _same({k: res[k] for k in ("2d", "3d")}, plain)
    ens = summary.Ensembleway("soft", C)
    for method in ("2d", "3d"):
        meter = HausdorffMeter(method=method, report_axises=[1, 2], C=C, spacing=sp)
        own = [HausdorffMeter(method=method, report_axises=[1, 2], C=C, spacing=sp) for _ in models]
        with torch.no_grad():
            for (img, gt), _, _ in val:
                preds = [m.predict(img.to(DEV), logit=False) for m in models]
                meter.add(ens(preds), gt.to(DEV))
                for o, p in zip(own, preds):
                    o.add(p, gt.to(DEV))
        t = res["hd_" + method]
        assert list(t) == ["model_0", "model_1", "ensemble", "ensemble_std"]
        (_, _), (means, stds) = meter.value()
        assert _same(t["ensemble"], {f"HD{j}": float(means[j]) for j in range(C)})
        assert _same(t["ensemble_std"], {f"HD{j}": float(stds[j]) for j in range(C)})
        for i, o in enumerate(own):
            assert _same(t[f"model_{i}"], {f"HD{j}": float(o.value()[1][0][j]) for j in range(C)})
        print(method, t)


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def add_scalars(self, tag, values, epoch):
        self.calls.append((tag, dict(values), epoch))


def test_eval_loop_uploads_val_hd_only_on_request(tmp_path):
    from dct_amd import ModelMode
    from dct_amd.loss import get_loss_fn
    from dct_amd.metrics import HausdorffMeter
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
    withhd = CoTrainer(segs, lab, val, val, crit, save_dir=str(tmp_path / "b"), val_hausdorff=True, val_spacing=(5.0, 1.0, 1.0), **kw)
    plain.writer, withhd.writer = _Recorder(), _Recorder()
    with torch.no_grad():
        a2, a3 = plain._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
        b2, b3 = withhd._eval_loop(val, epoch=0, mode=ModelMode.EVAL, save=False)
    assert torch.equal(a2, b2) and torch.equal(a3, b3)
    assert not [c for c in plain.writer.calls if c[0].startswith("val_hd")]
    assert [c for c in plain.writer.calls if c[0].startswith("val_data")] == [c for c in withhd.writer.calls if c[0].startswith("val_data")]
    hd = {c[0]: c[1] for c in withhd.writer.calls if c[0].startswith("val_hd/")}
    assert sorted(hd) == ["val_hd/S0", "val_hd/S1"]
    for i, seg in enumerate(segs):
        meter = HausdorffMeter(method="3d", report_axises=[1, 2], C=C, spacing=(5.0, 1.0, 1.0))
        with torch.no_grad():
            for (img, gt), _, _ in val:
                meter.add(seg.predict(img.to(DEV), logit=True), gt.to(DEV))
        means = meter.value()[1][0]
        assert _same(hd[f"val_hd/S{i}"], {f"HD{n}": float(means[n]) for n in (1, 2)})
